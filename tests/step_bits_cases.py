"""The launches whose output BITS are pinned (tests/golden/step_bits.json,
written by tools/make_step_bits.py, compared by tests/test_step_bits_gpu.py).

The recurrence frame (RecurH::step_seq), the frame head (frame_head,
attn_weights) and the prediction item loop (pred_tile, load_targets) of
csrc/g2k_scene.hip are shared by the fixed, general, split, loop-invariant
and train builds of the scene kernel.  A change that only re-schedules or
re-registers them must leave every output bit where it was: each case below
is the smallest launch at which one of those code paths can go wrong, and
its digests are the sha256 of the raw bytes of every output array.

Every case has 3 or 4 scenes, but for "fixed-frames": the six per-scene
frame counts 0, 1, 2, 3, 19 and 20 of the fixed build belong in ONE launch
(scenes of one launch share CUs and their frame counts select the peeled
last frame and the two-frame unroll per workgroup), so that case has six.

Inputs are synthetic.make_batch(..., h0_scale = 1.0) with the case's seed;
outputs are allocated zero-filled, so what a launch does not write (frames
past n_frames, columns past n_active) hashes the same in every run.
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass

import numpy as np

from multimodaltraj_2_amd import frame_step as fs
from multimodaltraj_2_amd.synthetic import make_batch

# rows 0..3 of the fallback case's G are -FALLBACK_K u, rows 4..15 +FALLBACK_K u
# (u = 1 / sqrt(T) in every entry): A[r][c] = lam G[r] . (E * Rm)[:, c] is then
# -a_c in the four leading rows and +a_c below, and a column with a_c > 45 has
# its leading rows more than 90 under its maximum, so exp(A - max) is 0 there,
# the first prefix sums are 0 and attn_weights takes its running (max, sum)
# branch.  Columns with a_c < 0 have the maximum in the leading rows (no
# underflow).  test_fallback_case_reaches_fallback checks a_c on the oracle.
FALLBACK_K = 200.0      # |A| stays under 500 with the seeded N(0, 1) weights
FALLBACK_MIN_SPREAD = 90.0


@dataclass(frozen=True)
class Case:
    id: str
    reaches: str
    H: int = 128
    Nmax: int = 32
    F: int = 20
    stride: int = 1
    n_active: tuple = (32, 17, 1, 16)
    n_frames: tuple | None = None
    layout: str = "ped"
    masked: tuple = ()              # (scene, column) pairs with ped_mask 0
    targets_shared: bool = False
    coresident: bool = True
    split: int = 0
    want_attn: bool = False
    train: str | None = None        # None (forward) / "l2" / "nll"
    fallback: bool = False
    seed: int = 11

    @property
    def S(self):
        return len(self.n_active)


CASES = [
    # --- the fixed 20-frame build (co-resident, stride 1, F = 20) ---------
    Case("fixed-frames", "peeled last frame and the two-frame unroll: n_frames 0, 1, 2, 3, 19, 20",
         n_active=(32, 17, 1, 16, 32, 5), n_frames=(0, 1, 2, 3, 19, 20)),
    Case("fixed-h64", "TPW 1", H=64, n_active=(32, 0, 17), n_frames=(20, 20, 7)),
    Case("fixed-h256", "TPW 4", H=256, n_active=(32, 16, 1), n_frames=(20, 9, 20)),
    Case("fixed-n17-band", "one full and one partial tile, band stores",
         Nmax=17, n_active=(0, 1, 16, 17), layout="band", masked=((3, 2), (3, 16))),
    Case("fixed-n17-ped", "one full and one partial tile, pedestrian-major stores",
         Nmax=17, n_active=(0, 1, 16, 17), layout="ped", masked=((3, 2), (3, 16))),
    Case("fixed-n32-band", "two full tiles, band stores, two masked pedestrians",
         n_active=(1, 16, 17, 32), layout="band", masked=((3, 5), (3, 23))),
    Case("fixed-n33-ped", "three tiles (the item loop wraps), the last holds one column",
         Nmax=33, n_active=(0, 17, 33, 16), layout="ped", masked=((2, 5), (2, 32))),
    Case("fixed-n33-band", "three tiles, band stores", Nmax=33, n_active=(1, 17, 33, 32),
         layout="band", masked=((2, 5), (2, 32))),
    Case("fixed-shared", "fixed build with one target set for every frame",
         n_active=(32, 17, 16), n_frames=(20, 13, 2), targets_shared=True),
    Case("fixed-fallback", "attn_weights' running (max, sum) branch", n_active=(32, 17, 16),
         n_frames=(20, 3, 1), fallback=True, want_attn=True),
    # --- the general build -------------------------------------------------
    Case("general-f21", "general co-resident build, one frame past the fixed build's", F=21,
         n_active=(32, 17, 1), want_attn=True),
    Case("general-f21-single", "general build, one workgroup per CU", F=21, coresident=False,
         split=1, n_active=(32, 17, 16), layout="band"),
    Case("general-f40", "chunk boundary: n_frames 32 and 33", F=40, n_active=(32, 17, 16, 1),
         n_frames=(32, 33, 40, 7)),
    Case("general-f40-single", "chunk boundary, one workgroup per CU", F=40, coresident=False,
         split=1, n_active=(32, 17, 16, 1), n_frames=(32, 33, 40, 7), layout="band"),
    Case("general-h512", "TPW 8", H=512, n_active=(32, 1, 17), n_frames=(20, 20, 5)),
    Case("general-h64-n33", "TPW 1, three tiles, general build", H=64, Nmax=33, F=7,
         n_active=(33, 0, 17, 16), masked=((0, 1), (0, 32))),
    # --- loop-invariant frames (stride 0, shared targets) -------------------
    Case("inv", "INV loop", stride=0, targets_shared=True, coresident=False,
         n_active=(32, 17, 16, 1), n_frames=(1, 5, 20, 12), want_attn=True),
    Case("inv-cores", "INV loop, co-resident geometry", stride=0, targets_shared=True,
         n_active=(32, 17, 16, 1), n_frames=(20, 2, 3, 0), layout="band"),
    Case("stride0", "stride 0 with a target set per frame", stride=0, coresident=False,
         n_active=(32, 17, 16), n_frames=(20, 4, 1)),
    # --- scenes without a chain: two workgroups per scene ------------------
    Case("split2", "split 2", coresident=False, split=2, n_active=(32, 17, 16, 1),
         n_frames=(20, 3, 0, 13), want_attn=True),
    Case("split2-n33-band", "split 2, three tiles, band stores", Nmax=33, coresident=False, split=2,
         n_active=(33, 17, 16), n_frames=(20, 1, 2), layout="band", masked=((0, 3), (0, 32))),
    # --- train builds ------------------------------------------------------
    Case("train-l2", "train build, L2", H=64, Nmax=17, F=5, coresident=False,
         n_active=(17, 16, 1), n_frames=(5, 4, 0), masked=((0, 3), (0, 16)), train="l2"),
    Case("train-nll", "train build, NLL", H=128, Nmax=33, F=4, coresident=False,
         n_active=(33, 17, 0), n_frames=(4, 1, 4), masked=((0, 3), (0, 32)), train="nll"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def inputs(case):
    """The case's host inputs: (SceneBatch, n_frames [S] int32 or None,
    ped_mask [S, Nmax] uint8 or None)."""
    b = make_batch(case.S, case.Nmax, case.H, F=case.F, seed=case.seed,
                   n_active=np.array(case.n_active, np.int32), h0_scale=1.0)
    if case.stride == 0:
        b.pos = np.ascontiguousarray(b.pos[:, :fs.OBS_LEN])
    if case.targets_shared:
        b.targets = np.ascontiguousarray(b.targets[:, :1])
    if case.fallback:
        sgn = np.where(np.arange(fs.HIDDEN_LEN) < 4, -1.0, 1.0)
        u = np.full(fs.OBS_LEN, 1.0 / np.sqrt(fs.OBS_LEN))
        b.G = np.ascontiguousarray(np.broadcast_to(
            (FALLBACK_K * np.outer(sgn, u)).astype(np.float32), b.G.shape))
    nfr = None if case.n_frames is None else np.array(case.n_frames, np.int32)
    mask = None
    if case.masked:
        mask = np.ones((case.S, case.Nmax), np.uint8)
        for s, col in case.masked:
            mask[s, col] = 0
    return b, nfr, mask


def params_for(case, device="cpu"):
    import torch
    p = fs.init_params(case.Nmax, seed=0, device=device)
    if case.train == "nll":
        p.Wo.mul_(0.05)                                   # predictions of O(1): a sane NLL
        head = (0.3 * np.random.default_rng(1).standard_normal((3, 12))).astype(np.float32)
        p.head = torch.from_numpy(head).to(device)
    return p


def digest(t) -> str:
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return hashlib.sha256(a.tobytes()).hexdigest()


def run_case(case, device) -> dict:
    """Launch the case through the library; {output name: sha256 of its bytes}."""
    import torch
    b, nfr, mask = inputs(case)
    t = b.to_device(device)
    S, F, Nmax, H = case.S, case.F, case.Nmax, case.H
    z = lambda *shape: torch.zeros(shape, device=device, dtype=torch.float32)  # noqa: E731
    out = fs.StepOutputs(pred=z(*fs.pred_shape(S, F, Nmax, case.layout)), h=z(S, fs.HIDDEN_LEN, H),
                         metrics=z(S, 8),
                         attn=z(S, F, fs.HIDDEN_LEN, fs.HIDDEN_LEN) if case.want_attn else None,
                         cost=z(S, F, fs.OBS_LEN, fs.OBS_LEN) if case.want_attn else None)
    kw = dict(n_frames=None if nfr is None else torch.from_numpy(nfr).to(device),
              ped_mask=None if mask is None else torch.from_numpy(mask).to(device),
              stride=case.stride, out=out, pred_layout=case.layout,
              targets_shared=case.targets_shared,
              frames=F if case.targets_shared else None, split=case.split)
    params = params_for(case, device)
    got = {}
    if case.train is None:
        fs.step_fused(params, t["pos"], t["vislet"], t["G"], t["targets"], t["n_active"], t["h0"],
                      want_attn=case.want_attn, coresident=case.coresident, **kw)
    else:
        from multimodaltraj_2_amd import train_step as ts
        plan = ts.TrainPlan(params, t["pos"], t["vislet"], t["G"], t["targets"], t["n_active"],
                            t["h0"], loss=case.train, lam=0.05, **kw)
        plan.grad.zero_()
        g = plan.run()
        torch.cuda.synchronize(device)
        got["grad"] = digest(g)
    torch.cuda.synchronize(device)
    got.update(pred=digest(out.pred), h=digest(out.h), metrics=digest(out.metrics))
    if case.want_attn:
        got.update(A=digest(out.attn), cost=digest(out.cost))
    return got
