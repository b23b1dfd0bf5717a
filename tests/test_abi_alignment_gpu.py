"""GPU: every entry point of include/g2k_hip.h, include/g2k_mix.h and
include/g2k_scores.h at the weakest pointer alignment its validator accepts
(tests/abi_alignment.py), through the raw C ABI.

Each case launches twice from the same host arrays, every buffer — inputs,
outputs, in/out state and workspaces — an ``Arena`` payload between poisoned
guards: once with every buffer on a 16-byte boundary (+0), once with the
case's buffers moved to their minimum (float32 / int32 +4, +8 where the
minimum is 8; float64 / int64 +8; ped_mask +1, +2, +3; an argument whose
minimum is 16 stays at +0 — ``offsets_at_minimum`` reads them from the
table, so no case can pass a pointer its validator rejects; the EM step and
the sample scores run with ped_mask at all three, ``every_mask``).  It asserts

* the minimum-alignment outputs are BIT-IDENTICAL to the +0 outputs (the
  poison of the elements that are not written included): alignment changes how
  bytes reach LDS or registers, never the arithmetic or the order of a sum;
* the +0 outputs meet the float64 oracle at the bound the existing test of
  that entry point uses (tests/test_step_cells_gpu.py, tests/test_train_gpu.py,
  tests/test_ops_domain_gpu.py: close 1e-4, close_h, attn and the gradient
  blocks normwise 1e-4, the update 1e-6 / 1e-5) — no new bound here;
* ``check_guards()`` and the documented write footprint, for both launches.

The scene kernel's cases are S = 3, H = 64, F = 5 (one chunk), the n_active /
n_frames / ped_mask of tests/step_cells.py's defaults, and each asserts the
build it reaches (g2k_step_geometry).  What each moves:

  pos8           pos +8, Nmax 32 (the per-row 4-byte window DMA at an EVEN
                 width: scene_pos_dma's `wide` false through the pointer) and
                 30 (rows of 240 bytes, never all on 16)
  weights4       Wi Wii Wv bv Wr Wc Wo, G, vislet +4, each its own buffer: the
                 4-byte path of every small prologue segment
  mask1/2/3      ped_mask at every residue, Nmax 32 (the byte-wise mask read
                 at Nmax % 4 == 0, reached only through the pointer) and 30
  outputs4       pred metrics A_out cost_out n_active n_frames +4, band
                 layout; pedestrian-major: the same with pred at +0 (its
                 16-byte stores are validated, see DESIGN.md 6a'')
  split2         G2K_STEP_SPLIT(2), the workspace (tickets, metric rows) +4
  all            everything above at once: the train, gradient, loop-invariant
                 and co-resident launches
Every case prints bit-identity and its worst oracle error over its bound
before it asserts.

MEASURED on an MI355X.  Bit-identity to the +0 launch held in EVERY case
below (every output, the poison of the unwritten elements included); the
figure is the worst oracle error of the +0 launch over its bound (1 = at the
bound) and the quantity that gives it:

  pos8-n32 0.44, weights4 0.44, mask1/2/3-n32 0.44, outputs4-band 0.44 (all
  the same +0 launch: h after one frame; pred 0.43), pos8-n30 / mask1/3-n30
  0.53 (h after one frame), outputs4-ped 0.42, split2-workspace4 0.41,
  inv-all 0.38, coresident-all 0.27 (pred)
  train-l2-all 0.33 (pred; gradient blocks <= 0.0023, update 0.03),
  train-nll-all 0.29 (h; dhead 0.0021), grad-l2-all 0.0025 (dWc),
  grad-update-l2-all 0.030 (the update's params; ms 0.019)
  frame_embed 0.054 (X), frame_recurrence D = 10 / 16 0.017 (h), mcr_forward
  0.024 (pred), ade_fde 4.9e-4 / 1.2e-5, nll 0.067 (dpred), gauss_sample
  0.023, update P = 8192 / 8193 0.031 / 0.033, gridlstm 0.0028, context_conv
  0.0012, encoder_chain 0.022 (h), scene_gather exact, nri ops 0.0013
  best_of_k 0.0079, fullcov_best_of_k 0.014, joint_eval 0.0011,
  fullcov_joint_eval 0.0014, kde_nll 0.0018 and fullcov_kde_nll 0.0021 (of
  tests/kde_ref.py's gate; each of the 2 x 8 sampler draws bit-identical too),
  fullcov_sample 0.018, head_stats 0.030 (fit; sums 1.9e-4 of 1e-11 sum|term|),
  fullcov_stats 0.0039 (moments, of 1e-12)
  mix_em 5.8e-4 with mix_out (the factors' backward error of 1e-4; moments
  1.4e-5 and total 1.2e-4 of EM_TOL) and 1.2e-4 without (total), ped_mask at
  +1, +2 and +3 alike; mix_sample 0.0039, comp the checker's, the in-place call
  (out == pred at +4) the separate output's bits; mix_best_of_k 0.0027,
  mix_joint_eval 0.0015, mix_kde_nll 5.8e-4 (of tests/mix_eval_ref.py's gate;
  each of the 8 sampler draws bit-identical too); the sample scores, F = 3 /
  F = 20 (two workgroups a scene: the workspace's rows at +4), ped_mask at +1,
  +2 and +3: per-step 0.0022 / 0.0042, fullcov 0.0020 / 0.0036, mix 0.0021 /
  0.0038 (a pair's column, of tests/scores_ref.py's TOL)
The wrapper test (views at 4 mod 16 of one padded flat buffer): bit-identical.
"""
import ctypes

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib
from multimodaltraj_2_amd import frame_step as fs
from multimodaltraj_2_amd import train_step as ts
from oracle import g2k_ref as ref
from tests import abi_alignment as al
from tests import step_cells as sc
from tests.abi_arena import Arena, all_written, bits, untouched
from tests.conftest import close, close_h
from tests.test_step_cells import KEYS, geometry

pytestmark = pytest.mark.gpu
TOL = 1e-4
LAM = 0.05
U8 = torch.uint8
WEIGHTS = ("Wi", "Wii", "Wv", "bv", "Wr", "Wc", "Wo")


@pytest.fixture
def lib(gpu):
    """The library with all three headers' symbols bound (one handle)."""
    from multimodaltraj_2_amd import mixture, scores
    assert mixture.load() is _lib.load() and scores.load() is _lib.load()
    return _lib.load()


def ptr(t):
    return None if t is None else t.data_ptr()


def host(t):
    return t.cpu().numpy()


def ok(lib, rc):
    assert rc == 0, lib.g2k_last_error()
    torch.cuda.synchronize()


def offsets_at_minimum(entry, cond=None, mask=1):
    """{argument: byte offset past a 16-byte boundary} that puts every pointer
    of `entry` at exactly the minimum the table gives (16 -> +0)."""
    out = {}
    e = al.BY_NAME[entry]
    for a in e.args:
        need = a.cond[2] if a.cond and a.cond[0] == cond else a.min
        out[a.name] = mask if a.elem == "u8" else need % 16
        assert out[a.name] % need == 0 and out[a.name] % al.ELEM_BYTES[a.elem] == 0, (entry, a.name)
    return out


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def compare(name, base, moved):
    """Bit-identity of two launches' outputs (dicts of device tensors)."""
    assert base.keys() == moved.keys()
    differ = [k for k in base if base[k] is not None and not same_bits(base[k], moved[k])]
    print(f"{name}: minimum-alignment launch bit-identical to the +0 launch: "
          f"{'yes' if not differ else 'NO: ' + ', '.join(differ)} ({len(base)} outputs)")
    assert not differ, (name, differ)


def report(name, ratios):
    worst = max(ratios, key=ratios.get)
    print(f"{name}: worst oracle error / bound = {ratios[worst]:.3g} ({worst}); "
          + ", ".join(f"{k} {v:.2g}" for k, v in sorted(ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (name, bad)


def up(r, key, value):
    r[key] = max(r.get(key, 0.0), float(value))


def rel(got, want):
    return close(got, want) if np.size(got) else 0.0


def normwise(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / (TOL * max(1.0, np.abs(want).max()))) if got.size else 0.0


# ---------------------------------------------------------------------------
# the scene kernel: g2k_step_fused_f32, g2k_train_step_f32, g2k_step_grad_f32,
# g2k_step_grad_update_f32
# ---------------------------------------------------------------------------
def _cell(id_, entry, Nmax=32, variant="general", np_=12, **kw):
    split = kw.get("split", 1)
    return sc.Cell(id_, entry, 64, Nmax, 5, claim=dict(variant=variant, tpw=1, np=np_, fc=5, chunks=1,
                                                      dwo_seq=0, own0=0, split=split or 1), **kw)


FWD32 = _cell("align-fwd-n32", "fwd")
FWD30 = _cell("align-fwd-n30", "fwd", Nmax=30)
FWD32_PED = _cell("align-fwd-n32-ped", "fwd", layout="ped")
FWD32_SPLIT2 = _cell("align-fwd-n32-split2", "fwd", split=2)
FWD_INV = _cell("align-fwd-inv", "fwd", variant="inv", stride=0, shared=True, split=0)
FWD_CORES = _cell("align-fwd-coresident", "fwd", np_=4, split=0, coresident=True)
TRAIN_L2 = _cell("align-train-l2", "train", np_=8)
TRAIN_NLL = _cell("align-train-nll", "train", variant="nll", np_=8, loss="nll")
GRAD_L2 = _cell("align-grad-l2", "grad", np_=8)
GRAD_UPD = _cell("align-grad-update-l2", "grad", np_=8)
ENTRY = {"fwd": "g2k_step_fused_f32", "train": "g2k_train_step_f32", "grad": "g2k_step_grad_f32"}
LR, DECAY, CLIP = 5e-3, 0.95, 10.0

_inputs = {}


def inputs(c):
    """The cell's host arrays (tests/test_step_cells_gpu.py's Inputs, on the
    host: every launch places its own copies), made once per cell."""
    if c.id not in _inputs:
        from tests.test_step_cells_gpu import Inputs
        _inputs[c.id] = Inputs(c, "cpu")
    return _inputs[c.id]


def scene_launch(lib, c, x, offs, update=False):
    """One raw-ABI launch of cell `c` with the buffers named in `offs` that
    many bytes past a 16-byte boundary (the others on one).  Returns the
    outputs and the arena (guards checked)."""
    S, F, H, Nmax, D = c.S, c.F, c.H, c.Nmax, 16
    o = lambda n: offs.get(n, 0)     # noqa: E731
    flags = fs.step_flags(c.layout, c.shared, c.loss, c.split, c.coresident)
    d = _lib.G2KDims(S, F, 8, 12, D, H, Nmax, x.pos.shape[1], c.stride, flags)
    ar = Arena("cuda")
    wt = {k: ar.put(x.w[k], "w." + k, o(k)) for k in WEIGHTS}
    head = ar.put(x.w["head"], "w.head", o("head")) if c.loss == "nll" else None
    w = _lib.G2KWeights(*[ptr(wt[k]) for k in WEIGHTS], ptr(head))
    ins = [ar.put(x.pos, "pos", o("pos")), ar.put(x.vislet, "vislet", o("vislet")),
           ar.put(x.G, "G", o("G")), ar.put(x.targets, "targets", o("targets")),
           ar.put(x.n_active, "n_active", o("n_active")), ar.put(x.n_frames, "n_frames", o("n_frames")),
           ar.put(x.mask.astype(np.uint8), "ped_mask", o("ped_mask"))]
    out = {}
    if c.entry != "grad":
        h_in = ar.put(x.h0, "h_in", o("h_in"))
        out["h_out"] = ar.alloc((S, D, H), name="h_out", offset=o("h_out"))
        out["pred"] = ar.alloc(fs.pred_shape(S, F, Nmax, c.layout), name="pred", offset=o("pred"))
        out["metrics"] = ar.alloc((S, 8), name="metrics", offset=o("metrics"))
    if c.entry == "fwd":
        out["A_out"] = ar.alloc((S, F, D, D), name="A_out", offset=o("A_out"))
        out["cost_out"] = ar.alloc((S, F, 8, 8), name="cost_out", offset=o("cost_out"))
        nws = int(lib.g2k_step_workspace_bytes(ctypes.byref(d)))
        assert (nws > 0) == (c.claim["split"] > 1)
        ws = ar.alloc((max(nws, 4),), U8, name="workspace", offset=o("workspace"))
        ok(lib, lib.g2k_step_fused_f32(ctypes.byref(d), ctypes.byref(w), *[ptr(t) for t in ins],
                                       ptr(h_in), ptr(out["h_out"]), ptr(out["pred"]),
                                       ptr(out["metrics"]), ptr(out["A_out"]), ptr(out["cost_out"]), LAM,
                                       ptr(ws), nws, None))
    else:
        P = int(lib.g2k_grad_size(ctypes.byref(d)))
        out["grad"] = ar.alloc((P + 2,), name="grad", offset=o("grad"))
        nws = int(lib.g2k_train_workspace_bytes(ctypes.byref(d)))
        assert nws == int(lib.g2k_grad_workspace_bytes(ctypes.byref(d)))
        ws = ar.alloc((nws,), U8, name="workspace", offset=o("workspace"))
        out["params"] = out["ms"] = None
        if update:
            flat = np.concatenate([x.w[k].reshape(-1) for k in WEIGHTS + (("head",) if head is not None else ())])
            assert flat.size == P
            out["params"] = ar.put(flat, "params", o("params"))
            out["ms"] = ar.put(np.full(P, 0.25, np.float32), "ms", o("ms"))
        upd = (ptr(out["params"]), ptr(out["ms"]), LR, DECAY, CLIP)
        if c.entry == "train":
            ok(lib, lib.g2k_train_step_f32(ctypes.byref(d), ctypes.byref(w), *[ptr(t) for t in ins],
                                           ptr(h_in), ptr(out["h_out"]), ptr(out["pred"]),
                                           ptr(out["metrics"]), LAM, ptr(out["grad"]), ptr(ws), nws, *upd,
                                           None))
        elif update:
            ok(lib, lib.g2k_step_grad_update_f32(ctypes.byref(d), ctypes.byref(w),
                                                 *[ptr(t) for t in ins], LAM, ptr(out["grad"]), ptr(ws),
                                                 nws, *upd, None))
        else:
            ok(lib, lib.g2k_step_grad_f32(ctypes.byref(d), ctypes.byref(w), *[ptr(t) for t in ins], LAM,
                                          ptr(out["grad"]), ptr(ws), nws, None))
    ar.check_guards()
    for k, t in list(wt.items()) + [("head", head)] + list(zip(("pos", "vislet", "G", "targets"), ins)):
        if t is not None:                                  # inputs are read only
            want = x.w[k] if k in x.w else getattr(x, k)
            assert np.array_equal(host(t).view(np.int32), np.ascontiguousarray(want).view(np.int32)), k
    return out, ar


def forward_reference(c, x):
    if "fwd" not in x.__dict__:
        x.fwd = [ref.scene_step(x.pos[s], x.vislet[s], x.G[s], x.w, x.scene_targets(c, s),
                                int(x.n_active[s]), x.h0[s], n_frames=int(x.n_frames[s]), stride=c.stride,
                                lam=LAM, ped_mask=x.mask[s], keep=True) for s in range(c.S)]
    return x.fwd


def check_forward(c, x, out, r):
    """pred / h / metrics (and attn / cost) of one launch: the write footprint
    of include/g2k_hip.h and the oracle, as tests/test_step_cells_gpu.py and
    tests/test_ops_domain_gpu.py hold them."""
    S, F, Nmax = c.S, c.F, c.Nmax
    assert all_written(out["metrics"]) and all_written(out["h_out"])
    keep_p, got_p = host(untouched(out["pred"])), host(out["pred"])
    hh, met = host(out["h_out"]), host(out["metrics"])
    for s in range(S):
        n, nf = int(x.n_active[s]), int(x.n_frames[s])
        pr, h, m, ex = forward_reference(c, x)[s]
        assert keep_p[s, nf:].all(), (c.id, s, "pred frames >= n_frames")
        if c.layout == "band":
            lim = min(Nmax, 16 * ((n + 15) // 16))
            assert not keep_p[s, :nf, :, :lim].any() and keep_p[s, :nf, :, lim:].all(), (c.id, s)
            assert np.all(got_p[s, :nf, :, n:lim].view(np.int32) == 0), (c.id, s)
            band = got_p[s, :nf, :, :n]
        else:
            assert not keep_p[s, :nf, :n].any() and keep_p[s, :nf, n:].all(), (c.id, s)
            band = np.transpose(got_p[s, :nf, :n], (0, 3, 2, 1)).reshape(nf, 24, n)
        got = band.reshape(nf, 2, 12, n)
        up(r, "pred", rel(got, pr) / c.pred_tol)
        up(r, "metrics", rel(met[s, :6], m[:6]) / TOL)
        assert met[s, 1] == m[1] and met[s, 5] == nf and np.all(met[s, 6:] == 0), (c.id, s)
        up(r, "h after one frame" if nf == 1 else "h", (np.abs(hh[s] - h) / (1e-5 * np.abs(h) + 1e-8)).max())
        assert close_h(hh[s], h), (c.id, s)
        for key, name in (("A_out", "A"), ("cost_out", "cost")):
            if key in out:
                keep_t = host(untouched(out[key]))[s]
                assert keep_t[nf:].all() and not keep_t[:nf].any(), (c.id, s, key)
                want = np.stack(ex[name]) if nf else np.zeros((0,) + keep_t.shape[1:])
                if key == "A_out":
                    up(r, "attn", normwise(host(out[key])[s, :nf], want))
                else:
                    up(r, "cost", rel(host(out[key])[s, :nf], want) / TOL)


def check_gradient(c, x, out, r, update):
    from tests.test_step_cells_gpu import grad_reference
    if "grd" not in x.__dict__:
        x.grd = grad_reference(c, x)
    order, R, loss, cnt, _ = x.grd
    assert all_written(out["grad"])
    g = host(out["grad"]).astype(np.float64)
    P, off = g.size - 2, 0
    for k in order:
        want = np.asarray(R[k], np.float64).reshape(-1)
        got = g[off:off + want.size]
        off += want.size
        if k == "Wr":
            assert np.all(got == 0), (c.id, "Wr")
        else:
            up(r, "d" + k, np.abs(got - want).max() / (TOL * np.abs(want).max()))
    assert off == P
    up(r, "loss", abs(g[P] - loss) / (TOL * abs(loss)))
    assert g[P + 1] == cnt, (c.id, "pair count")
    if update:
        gh = host(out["grad"])
        p0 = np.concatenate([x.w[k].reshape(-1) for k in order])
        rp, rm = ref.optimizer_update(p0, np.full(P, 0.25, np.float32), gh[:P], gh[P + 1], LR, DECAY, CLIP)
        up(r, "update-params", np.abs(host(out["params"]) - rp).max() / (1e-6 * max(1.0, np.abs(rp).max())))
        up(r, "update-ms", np.abs(host(out["ms"]) - rm).max() / (1e-5 * np.abs(rm).max()))


def scene_case(lib, gpu, c, offs, name, update=False):
    g = geometry(c, cus=fs.device_cus(gpu))
    assert {k: g[k] for k in KEYS} == c.claim, (c.id, g)        # the build this case is for
    assert g["ped_major"] == (c.layout == "ped")
    entry = "g2k_step_grad_update_f32" if (c.entry == "grad" and update) else ENTRY[c.entry]
    cond = "ped_major" if c.layout == "ped" else None
    legal = offsets_at_minimum(entry, cond, mask=offs.get("ped_mask", 1))
    for k, v in offs.items():                                     # nothing the validator may reject
        assert v in (0, legal[k]), (name, k, v, legal[k])
    x = inputs(c)
    base, _ = scene_launch(lib, c, x, {}, update)
    moved, _ = scene_launch(lib, c, x, offs, update)
    compare(name, base, moved)
    r = {}
    if c.entry != "grad":
        check_forward(c, x, base, r)
    if c.entry != "fwd":
        check_gradient(c, x, base, r, update)
    report(name, r)


def group(entry, names, cond=None, mask=1):
    at = offsets_at_minimum(entry, cond, mask)
    return {k: at[k] for k in names}


STEP = "g2k_step_fused_f32"
SCENE_CASES = [
    ("pos8-n32", FWD32, group(STEP, ["pos"])),
    ("pos8-n30", FWD30, group(STEP, ["pos"])),
    ("weights4", FWD32, group(STEP, list(WEIGHTS) + ["G", "vislet"])),
    ("mask1-n32", FWD32, group(STEP, ["ped_mask"], mask=1)),
    ("mask2-n32", FWD32, group(STEP, ["ped_mask"], mask=2)),
    ("mask3-n32", FWD32, group(STEP, ["ped_mask"], mask=3)),
    ("mask1-n30", FWD30, group(STEP, ["ped_mask"], mask=1)),
    ("mask3-n30", FWD30, group(STEP, ["ped_mask"], mask=3)),
    ("outputs4-band", FWD32, group(STEP, ["pred", "metrics", "A_out", "cost_out", "n_active", "n_frames"])),
    ("outputs4-ped", FWD32_PED, group(STEP, ["pred", "metrics", "A_out", "cost_out", "n_active", "n_frames"],
                                      cond="ped_major")),
    ("split2-workspace4", FWD32_SPLIT2, group(STEP, ["workspace"])),
    ("inv-all", FWD_INV, offsets_at_minimum(STEP)),
    ("coresident-all", FWD_CORES, offsets_at_minimum(STEP, mask=3)),
]


@pytest.mark.parametrize("name,cell,offs", SCENE_CASES, ids=[c[0] for c in SCENE_CASES])
def test_forward_step_at_minimum_alignment(lib, gpu, name, cell, offs):
    """MEASURED on an MI355X: see the module's closing table (every case
    bit-identical to its +0 launch)."""
    if name.startswith("pos8"):
        assert offs == {"pos": 8}
    if name == "outputs4-ped":
        assert offs["pred"] == 0 and offs["metrics"] == 4     # the 16-byte stores: validated, not moved
    scene_case(lib, gpu, cell, offs, name)


TRAIN_CASES = [
    ("train-l2-all", TRAIN_L2, "g2k_train_step_f32", True),
    ("train-nll-all", TRAIN_NLL, "g2k_train_step_f32", True),
    ("grad-l2-all", GRAD_L2, "g2k_step_grad_f32", False),
    ("grad-update-l2-all", GRAD_UPD, "g2k_step_grad_update_f32", True),
]


@pytest.mark.parametrize("name,cell,entry,update", TRAIN_CASES, ids=[c[0] for c in TRAIN_CASES])
def test_train_entry_points_at_minimum_alignment(lib, gpu, name, cell, entry, update):
    """Every buffer at its minimum: weights (NLL: the head, segment 10), G,
    vislet, grad, params, ms +4, pos +8, ped_mask +1, the workspace +4."""
    offs = offsets_at_minimum(entry)
    assert offs["workspace"] == 4 and offs["grad"] == 4 and offs["head"] == 4 and offs["pos"] == 8
    assert offs.get("params", 4) == 4 and offs.get("ms", 4) == 4
    scene_case(lib, gpu, cell, offs, name, update)


def test_wrappers_on_views_of_one_padded_flat_buffer(gpu):
    """The Python route of a caller that packs its weights itself: views into
    one flat buffer behind a single padding float, so every view starts 4
    bytes past a 16-byte boundary.  fs.step_fused and ts.GradPlan(...).run()
    on the views equal the same calls on separately allocated copies, bit for
    bit."""
    c = FWD32
    x = inputs(c)
    own = fs.init_params(c.Nmax, seed=0, device=gpu)
    parts = [getattr(own, k) for k in WEIGHTS]
    flat = torch.empty(1 + sum(t.numel() for t in parts), device=gpu, dtype=torch.float32)
    assert flat.data_ptr() % 16 == 0
    views, off = {}, 1
    for k, t in zip(WEIGHTS, parts):
        views[k] = flat[off:off + t.numel()].view(t.shape)
        views[k].copy_(t)
        assert views[k].data_ptr() % 16 == 4, k
        off += t.numel()
    packed = fs.G2KParams(**views)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)   # noqa: E731
    t = [dev(a) for a in (x.pos, x.vislet, x.G, x.targets, x.n_active)]
    kw = dict(n_frames=dev(x.n_frames), ped_mask=dev(x.mask.astype(np.uint8)), stride=c.stride, lam=LAM)
    a = fs.step_fused(own, *t, dev(x.h0), want_attn=True, split=1, **kw)
    b = fs.step_fused(packed, *t, dev(x.h0), want_attn=True, split=1, **kw)
    torch.cuda.synchronize()
    for k in ("pred", "h", "metrics"):
        assert same_bits(getattr(a, k), getattr(b, k)), k
    for s_, nf in enumerate(x.n_frames):       # attn / cost: allocated empty, written for frames < n_frames
        for k in ("attn", "cost"):
            assert same_bits(getattr(a, k)[s_, :nf], getattr(b, k)[s_, :nf]), (k, s_)
    ga = ts.GradPlan(own, *t, split=1, **kw).run().clone()
    gb = ts.GradPlan(packed, *t, split=1, **kw).run().clone()
    torch.cuda.synchronize()
    assert same_bits(ga, gb)
    print("wrappers on 4-mod-16 views: step_fused and GradPlan bit-identical to separate allocations")


# ---------------------------------------------------------------------------
# the other entry points: one small case each, at the smallest shape of
# tests/test_ops_domain_gpu.py that still has a partial tile or a second trip
# ---------------------------------------------------------------------------
class Bufs:
    """The buffers of one launch of `entry`, every one an Arena payload: on a
    16-byte boundary, or (`at_min`) at the table's minimum for its argument."""

    def __init__(self, entry, at_min, cond=None, mask=1):
        self.ar = Arena("cuda")
        self.off = offsets_at_minimum(entry, cond, mask) if at_min else {}
        self.names = {a.name for a in al.BY_NAME[entry].args}

    def put(self, name, array, dtype=None):
        assert name in self.names, name
        a = np.ascontiguousarray(array if dtype is None else np.asarray(array, dtype))
        return self.ar.put(a, name, self.off.get(name, 0))

    def out(self, name, shape, dtype=torch.float32):
        assert name in self.names, name
        return self.ar.alloc(shape, dtype, name, self.off.get(name, 0))

    def weights(self, w):
        t = {k: self.put(k, v) for k, v in w.items() if k in self.names}
        return _lib.G2KWeights(**{k: ptr(v) for k, v in t.items()}), t


def twice(name, entry, run, cond=None, mask=1):
    """`run(bufs)` launches and returns its outputs; +0, then at the minimum;
    bit-identity; the +0 outputs are returned for the oracle."""
    base = run(Bufs(entry, False))
    moved = run(Bufs(entry, True, cond, mask))
    compare(name, base, moved)
    return base


def every_mask(name, entry, run):
    """`twice` with ped_mask at +1, then the minimum launch again with it at +2
    and +3, each against the same +0 launch."""
    base = twice(f"{name} mask+1", entry, run, mask=1)
    for mask in (2, 3):
        compare(f"{name} mask+{mask}", base, run(Bufs(entry, True, None, mask)))
    return base


from tests.test_ops_domain_gpu import (LAM as OPS_LAM, dims, draw_head, error_inputs, f32, f64,  # noqa: E402
                                       pairs_metrics, recurrence_ref, weights)


def test_frame_embed_at_minimum_alignment(lib):
    """pos +8 (its float2 reads), everything else +4; Nmax 30: rows of 240
    bytes."""
    rng = np.random.default_rng(3100)
    S, F, D, Nmax, stride = 3, 3, 16, 30, 1
    W = (F - 1) * stride + 8
    n_active = [Nmax, 0, Nmax // 2]
    w = weights(rng, D, Nmax)
    pos, vis = f32(rng, S, W, Nmax, 2), f32(rng, S, 2, Nmax)
    for s, n in enumerate(n_active):
        pos[s, :, n:] = np.nan
        vis[s, :, n:] = np.nan
    d = dims(S=S, F=F, Nmax=Nmax, W=W, stride=stride)

    def run(b):
        ws, keep = b.weights(w)
        ins = [b.put("pos", pos), b.put("vislet", vis), b.put("n_active", n_active, np.int32)]
        X, Rel = b.out("X", (S, F, D + 2, D)), b.out("Rel", (S, 2, D))
        ok(lib, lib.g2k_frame_embed_f32(ctypes.byref(d), ctypes.byref(ws), *[ptr(t) for t in ins],
                                        ptr(X), ptr(Rel), None))
        b.ar.check_guards()
        assert all_written(X) and all_written(Rel)
        return dict(X=X, Rel=Rel)

    assert offsets_at_minimum("g2k_frame_embed_f32")["pos"] == 8
    o = twice("frame_embed", "g2k_frame_embed_f32", run)
    X, Relh, r = host(o["X"]), host(o["Rel"]), {}
    for s, n in enumerate(n_active):
        Wi = w["Wi"][:n].astype(np.float64)
        Ve, R = ref.vislet_embed(vis[s][:, :n].astype(np.float64), Wi)
        up(r, "Rel", close(Relh[s], R) / TOL)
        for f in range(F):
            Bv = ref.window_norms(pos[s][f * stride:f * stride + 8, :n].astype(np.float64))
            X0 = ref.input_embed(Bv, Wi, w["Wii"].astype(np.float64))
            up(r, "X", close(X[s, f], np.concatenate((X0, Ve), axis=0)) / TOL)
    report("frame_embed", r)


@pytest.mark.parametrize("D", [10, 16])
def test_frame_recurrence_at_minimum_alignment(lib, D):
    """D = 10: A and h +4 (the element-wise staging); D = 16: both validated
    at 16 and left at +0.  33 frames: a second chunk."""
    rng = np.random.default_rng(1100 + D)
    S, frames, H = 2, 33, 64
    A, h0 = f32(rng, S, frames, D, D, scale=2.0), f32(rng, S, D, H)
    cond = "D16" if D == 16 else None
    assert offsets_at_minimum("g2k_frame_recurrence_f32", cond) == (dict(A=0, h=0) if D == 16 else dict(A=4, h=4))

    def run(b):
        At, h = b.put("A", A), b.put("h", h0)
        ok(lib, lib.g2k_frame_recurrence_f32(ctypes.byref(dims(S=S, D=D, H=H)), ptr(At), ptr(h), frames,
                                             None))
        b.ar.check_guards()
        return dict(h=h)

    o = twice(f"frame_recurrence D={D}", "g2k_frame_recurrence_f32", run, cond)
    got, want = host(o["h"]), recurrence_ref(A, h0)
    report(f"frame_recurrence D={D}", {"h": float(np.max(np.abs(got - want) / (1e-5 * np.abs(want) + 1e-8)))})
    assert close_h(got, want)


def test_mcr_forward_at_minimum_alignment(lib):
    rng = np.random.default_rng(2100)
    S, D, Nmax = 3, 10, 17
    w = weights(rng, D, Nmax)
    X, Rel, G = f32(rng, S, D + 2, D), f32(rng, S, 2, D) ** 2, f32(rng, S, D, 8)
    n_active = [Nmax, 1, 0]

    def run(b):
        ws, keep = b.weights(w)
        ins = [b.put("X", X), b.put("Rel", Rel), b.put("G", G), b.put("n_active", n_active, np.int32)]
        A, cost, pred = b.out("A_out", (S, D, D)), b.out("cost_out", (S, 8, 8)), b.out("pred", (S, 24, Nmax))
        ok(lib, lib.g2k_mcr_forward_f32(ctypes.byref(dims(S=S, D=D, Nmax=Nmax)), ctypes.byref(ws),
                                        *[ptr(t) for t in ins], ptr(A), ptr(cost), ptr(pred), OPS_LAM, None))
        b.ar.check_guards()
        assert all_written(A) and all_written(cost) and all_written(pred)
        return dict(A_out=A, cost_out=cost, pred=pred)

    o = twice("mcr_forward", "g2k_mcr_forward_f32", run)
    A, cost, pred, r = host(o["A_out"]), host(o["cost_out"]), host(o["pred"]), {}
    for s, n in enumerate(n_active):
        q = ref.mcr_forward(*map(f64, (X[s], Rel[s], G[s], w["Wv"], w["bv"], w["Wr"], w["Wc"],
                                       w["Wo"][:, :n])), OPS_LAM)
        up(r, "attn", normwise(A[s], q["attn"]))
        up(r, "cost", close(cost[s], q["cost"]) / TOL)
        up(r, "pred", rel(pred[s, :, :n], q["pred_path_band"].reshape(24, n)) / TOL)
        assert np.all(pred[s, :, n:].view(np.int32) == 0)
    report("mcr_forward", r)


@pytest.mark.parametrize("variant", [0, 1])
def test_ade_fde_at_minimum_alignment(lib, variant):
    """pred, n_active, n_frames, out +4, ped_mask +1, targets (float4 reads) +0."""
    rng = np.random.default_rng(4200 + variant)
    S, F, Nmax = (4, 5, 30) if variant == 0 else (3, 1, 65)
    n_active = [Nmax, 0, Nmax // 2, 17][:S]
    n_frames = [F, 1, F, 0] if variant == 0 else None
    mask = None
    if variant == 0:
        mask = (rng.random((S, Nmax)) > 0.3).astype(np.uint8)
        mask[0, 0] = 1
    pred, tgt = error_inputs(rng, S, F, Nmax, n_active, n_frames)

    def run(b):
        ins = [b.put("pred", pred), b.put("targets", tgt), b.put("n_active", n_active, np.int32),
               None if n_frames is None else b.put("n_frames", n_frames, np.int32),
               None if mask is None else b.put("ped_mask", mask)]
        out = b.out("out", (S, 8))
        ok(lib, lib.g2k_ade_fde_f32(ctypes.byref(dims(S=S, F=F, Nmax=Nmax)), *[ptr(t) for t in ins],
                                    variant, ptr(out), None))
        b.ar.check_guards()
        assert all_written(out)
        return dict(out=out)

    assert offsets_at_minimum("g2k_ade_fde_f32")["targets"] == 0
    got, r = host(twice(f"ade_fde variant {variant}", "g2k_ade_fde_f32", run)["out"]), {}
    for s, n in enumerate(n_active):
        if variant == 0:
            m = pairs_metrics(pred[s], tgt[s], n, n_frames[s], mask[s])
            up(r, "sums", close(got[s, :5], m[:5]) / TOL)
            assert got[s, 1] == m[1] and got[s, 5] == n_frames[s] and np.all(got[s, 6:8].view(np.int32) == 0)
        elif n == 0:
            assert np.all(got[s].view(np.int32) == 0)
        else:
            p = np.transpose(pred[s, 0, :, :n].reshape(2, 12, n), (2, 1, 0))
            ade, fde, counter = ref.get_mean_error(p, tgt[s, 0, :n], 8, n)
            up(r, "ade", close(got[s, 0], ade) / TOL)
            up(r, "fde", close(got[s, 1], fde) / TOL)
            assert int(got[s, 2]) == counter and np.all(got[s, 3:].view(np.int32) == 0)
    report(f"ade_fde variant {variant}", r)


def test_nll_and_sampler_at_minimum_alignment(lib):
    """g2k_nll_f32: targets +8 (float2 reads), pred, head, out, dpred, the
    workspace +4, ped_mask +1; g2k_gauss_sample_f32: everything +4."""
    rng = np.random.default_rng(8300)
    S, F, Nmax = 4, 3, 7
    n_active, n_frames = [Nmax, 0, 3, 5], [3, 0, 2, 1]
    mask = (rng.random((S, Nmax)) > 0.3).astype(np.uint8)
    mask[3, 0] = 1
    pred, tgt = error_inputs(rng, S, F, Nmax, n_active, n_frames)
    head = draw_head(rng)
    d = dims(S=S, F=F, Nmax=Nmax)
    nws = int(lib.g2k_nll_workspace_bytes(ctypes.byref(d)))

    def run(b):
        ins = [b.put("pred", pred), b.put("targets", tgt), b.put("n_active", n_active, np.int32),
               b.put("n_frames", n_frames, np.int32), b.put("ped_mask", mask), b.put("head", head)]
        out, dpred = b.out("out", (38,)), b.out("dpred", pred.shape)
        ws = b.out("workspace", (S, 38))
        ok(lib, lib.g2k_nll_f32(ctypes.byref(d), *[ptr(t) for t in ins], ptr(out), ptr(dpred), ptr(ws), nws,
                                None))
        b.ar.check_guards()
        assert all_written(out) and all_written(ws)
        return dict(out=out, dpred=dpred)

    at = offsets_at_minimum("g2k_nll_f32")
    assert at["targets"] == 8 and at["workspace"] == 4 and at["ped_mask"] == 1
    o = twice("nll", "g2k_nll_f32", run)
    out, dp, keep = host(o["out"]), host(o["dpred"]), host(untouched(o["dpred"]))
    R_nll, R_pairs, R_dh, r = 0.0, 0, np.zeros((3, 12)), {}
    for s in range(S):
        n, nf = n_active[s], n_frames[s]
        l_, p_, h_, d_ = ref.bivariate_nll(pred[s], tgt[s], head, n, nf, mask[s].astype(bool))
        R_nll, R_pairs, R_dh = R_nll + l_, R_pairs + p_, R_dh + h_
        assert keep[s, nf:].all() and keep[s, :nf, :, n:].all() and not keep[s, :nf, :, :n].any(), s
        on = mask[s, :n].astype(bool)
        assert np.all(dp[s, :nf][:, :, :n][:, :, ~on].view(np.int32) == 0), s
        if nf and on.any():
            up(r, "dpred", close(dp[s, :nf][:, :, :n][:, :, on], d_[:nf][:, :, :n][:, :, on]) / TOL)
    up(r, "nll", abs(float(out[36]) - R_nll) / abs(R_nll) / TOL)
    up(r, "dhead", np.abs(out[:36].reshape(3, 12) - R_dh).max() / np.abs(R_dh).max() / TOL)
    assert int(out[37]) == R_pairs
    report("nll", r)

    seed, head2 = 2 ** 32 + 5, draw_head(rng, edge=False)
    clean = f32(rng, S, F, 24, Nmax)

    def draw(b):
        ins = [b.put("pred", clean), b.put("head", head2)]
        out = b.out("out", clean.shape)
        ok(lib, lib.g2k_gauss_sample_f32(ctypes.byref(d), ptr(ins[0]), ptr(ins[1]), ctypes.c_uint64(seed),
                                         ptr(out), None))
        b.ar.check_guards()
        assert all_written(out)
        return dict(out=out)

    o = twice("gauss_sample", "g2k_gauss_sample_f32", draw)
    report("gauss_sample", {"draw": close(host(o["out"]), ref.gauss_sample(clean, head2, seed)) / TOL})


@pytest.mark.parametrize("P", [8192, 8193])
def test_update_at_minimum_alignment(lib, P):
    """Both paths (<= 8192: the register-held one; above: the loop), RMSProp
    with clipping; params, ms, grad +4."""
    rng = np.random.default_rng(9500 + P)
    p, g, ms0 = f32(rng, P), f32(rng, P + 2, scale=5.0), np.abs(f32(rng, P))
    g[P + 1] = 7

    def run(b):
        flat, ms, grad = b.put("params", p), b.put("ms", ms0), b.put("grad", g)
        ok(lib, lib.g2k_update_f32(ptr(flat), ptr(ms), ptr(grad), P, 5e-3, 0.95, 0.5, None))
        b.ar.check_guards()
        assert np.array_equal(host(grad).view(np.int32), g.view(np.int32))
        return dict(params=flat, ms=ms)

    o = twice(f"update P={P}", "g2k_update_f32", run)
    rp, rm = ref.optimizer_update(p, ms0, g[:P], g[P + 1], 5e-3, 0.95, 0.5)
    report(f"update P={P}", {"params": np.abs(host(o["params"]) - rp).max() / (1e-6 * max(1.0, np.abs(rp).max())),
                             "ms": np.abs(host(o["ms"]) - rm).max() / (1e-5 * np.abs(rm).max())})


def test_gridlstm_at_minimum_alignment(lib):
    rng = np.random.default_rng(6100)
    u, fs_, K, R = 2, 4, 4, 257
    wd = 2 * u * K
    ld = wd + 3
    x, st = f32(rng, R, K * fs_), f32(rng, R, ld)
    W, bb, P = f32(rng, fs_ + 2 * u, 3 * u, scale=0.7), f32(rng, 3 * u, scale=0.3), f32(rng, 4, u)

    def run(b):
        ins = [b.put("in", x), b.put("state", st), b.put("W", W), b.put("b", bb), b.put("peep", P)]
        out, so = b.out("out", (R, wd)), b.out("state_out", (R, wd))
        ok(lib, lib.g2k_gridlstm_f32(ptr(ins[0]), K * fs_, ptr(ins[1]), ld, ptr(ins[2]), ptr(ins[3]),
                                     ptr(ins[4]), ptr(out), ptr(so), R, K, fs_, u, None))
        b.ar.check_guards()
        assert all_written(out) and all_written(so)
        return dict(out=out, state_out=so)

    o = twice("gridlstm", "g2k_gridlstm_f32", run)
    ro, rs = ref.gridlstm_cell(x, st, W, bb, tuple(P), feature_size=fs_, num_units=u)
    report("gridlstm", {"out": close(host(o["out"]), ro) / TOL, "state": close(host(o["state_out"]), rs) / TOL})


def test_context_conv_at_minimum_alignment(lib):
    rng = np.random.default_rng(7100)
    C, D = 2, 7
    Hh = Ww = D + 1
    img = rng.uniform(0, 255, size=(Hh, Ww, C)).astype(np.float32)
    filt = f32(rng, Hh + 3 - D, Ww + 2 - D, C)
    nws = int(lib.g2k_context_conv_workspace_bytes(Hh, Ww, D))

    def run(b):
        ins = [b.put("img", img), b.put("filt", filt)]
        out, G, ws = b.out("out", (D, D)), b.out("G", (D, 8)), b.out("workspace", (nws // 4,))
        ok(lib, lib.g2k_context_conv_f32(ptr(ins[0]), Hh, Ww, C, ptr(ins[1]), D, 5e-4, ptr(out), ptr(G),
                                         ptr(ws), nws, None))
        b.ar.check_guards()
        assert all_written(out) and all_written(G) and all_written(ws)
        return dict(out=out, G=G)

    o = twice("context_conv", "g2k_context_conv_f32", run)
    rc = ref.context_conv(img, filt, D, 5e-4)
    rG = ref.context_input(rc, ref.static_mask(D, 8))
    report("context_conv", {"out": np.abs(host(o["out"]) - rc).max() / (1e-4 * np.abs(rc).max()),
                            "G": np.abs(host(o["G"]) - rG).max() / (1e-4 * np.abs(rG).max())})


def test_encoder_chain_at_minimum_alignment(lib):
    """h and attn (validated at 16) +0, everything else +4."""
    rng = np.random.default_rng(9350)
    S, F, H, u, fs_, D, Nmax = 2, 3, 64, 2, 4, 16, 7
    n_active, n_frames = [5, 7], [2, 3]
    w = weights(rng, D, Nmax)
    X, Rel, G = f32(rng, S, F, D + 2, D, scale=0.5), f32(rng, S, 2, D) ** 2, f32(rng, S, D, 8)
    cW, cb, cP = f32(rng, fs_ + 2 * u, 3 * u, scale=0.7), f32(rng, 3 * u, scale=0.3), f32(rng, 4, u)
    h0 = f32(rng, D, H)

    def run(b):
        ws, keep = b.weights(w)
        ins = [b.put("X", X), b.put("Rel", Rel), b.put("G", G), b.put("n_active", n_active, np.int32),
               b.put("n_frames", n_frames, np.int32), b.put("cell_W", cW), b.put("cell_b", cb),
               b.put("cell_peep", cP)]
        Xe, cs = b.out("Xe", (S, F, D + 2, D)), b.out("cell_state", (D, D))
        attn, cost = b.out("attn", (S, F, D, D)), b.out("cost", (S, F, 8, 8))
        pred, h = b.out("pred", (S, F, 24, Nmax)), b.put("h", h0)
        ok(lib, lib.g2k_encoder_chain_f32(ctypes.byref(dims(S=S, F=F, H=H, Nmax=Nmax)), ctypes.byref(ws),
                                          *[ptr(t) for t in ins], fs_, u, ptr(Xe), ptr(cs), ptr(attn),
                                          ptr(cost), ptr(pred), ptr(h), OPS_LAM, None))
        b.ar.check_guards()
        assert all_written(Xe) and all_written(cs) and all_written(h)
        return dict(Xe=Xe, cell_state=cs, attn=attn, cost=cost, pred=pred, h=h)

    at = offsets_at_minimum("g2k_encoder_chain_f32")
    assert at["h"] == 0 and at["attn"] == 0 and at["X"] == 4
    o = twice("encoder_chain", "g2k_encoder_chain_f32", run)
    Xe_h, r, hh = host(o["Xe"]), {}, h0.astype(np.float64)
    for s in range(S):
        n = n_active[s]
        for t in ("attn", "cost", "pred"):
            keep_t = host(untouched(o[t]))[s].reshape(F, -1)
            assert keep_t[n_frames[s]:].all() and not keep_t[:n_frames[s]].any(), (s, t)
        for f in range(n_frames[s]):
            x0 = ref.gridlstm_cell(X[s, f, :D], hh, cW, cb, tuple(cP), feature_size=fs_, num_units=u)[0]
            up(r, "Xe", close(Xe_h[s, f, :D], x0) / TOL)
            q = ref.mcr_forward(*map(f64, (np.concatenate((x0, X[s, f, D:])), Rel[s], G[s], w["Wv"], w["bv"],
                                           w["Wr"], w["Wc"], w["Wo"][:, :n])), OPS_LAM)
            up(r, "attn", normwise(host(o["attn"][s, f]), q["attn"]))
            up(r, "cost", close(host(o["cost"][s, f]), q["cost"]) / TOL)
            p = host(o["pred"][s, f])
            up(r, "pred", close(p[:, :n], q["pred_path_band"].reshape(24, n)) / TOL)
            assert np.all(p[:, n:] == 0)
            hh = ref.recurrence_step(q["attn"], hh)
    up(r, "h", np.max(np.abs(host(o["h"]) - hh) / (1e-5 * np.abs(hh) + 1e-8)))
    report("encoder_chain", r)


def test_scene_gather_at_minimum_alignment(lib):
    """xy, pos, targets +8 (float2 accesses), the index arrays and vislet +4,
    ped_mask +1.  A gather: exact."""
    rng = np.random.default_rng(9250)
    cols, S, F, Nmax = 40, 2, 2, 5
    n_active = [3, 5]
    xy, vis = f32(rng, cols, 2), f32(rng, 2, cols)
    pos_col = rng.integers(0, cols, size=(S, 8, Nmax)).astype(np.int32)
    pos_col[0, 0, 1] = pos_col[1, 3, 4] = -1
    tgt_col = rng.integers(0, cols, size=(S, Nmax, 12)).astype(np.int32)
    tgt_col[1, 2, 11] = -1
    vis_off = np.array([4, 33], np.int32)

    def run(b):
        ins = [b.put("xy", xy), b.put("vis", vis), b.put("pos_col", pos_col), b.put("tgt_col", tgt_col),
               b.put("vis_off", vis_off), b.put("n_active", n_active, np.int32)]
        pos, vislet = b.out("pos", (S, 8, Nmax, 2)), b.out("vislet", (S, 2, Nmax))
        targets, pm = b.out("targets", (S, F, Nmax, 12, 2)), b.out("ped_mask", (S, Nmax), U8)
        ok(lib, lib.g2k_scene_gather_f32(ptr(ins[0]), ptr(ins[1]), cols, ptr(ins[2]), ptr(ins[3]),
                                         ptr(ins[4]), ptr(ins[5]), S, F, Nmax, ptr(pos), ptr(vislet),
                                         ptr(targets), ptr(pm), None))
        b.ar.check_guards()
        out = dict(pos=pos, vislet=vislet, targets=targets, ped_mask=pm)
        assert all(all_written(t) for t in out.values())
        return out

    at = offsets_at_minimum("g2k_scene_gather_f32")
    assert (at["xy"], at["pos"], at["targets"], at["pos_col"], at["ped_mask"]) == (8, 8, 8, 4, 1)
    o = twice("scene_gather", "g2k_scene_gather_f32", run)
    col = lambda c: xy[c] if c >= 0 else np.zeros(2, np.float32)          # noqa: E731
    e_pos, e_vis = np.zeros((S, 8, Nmax, 2), np.float32), np.zeros((S, 2, Nmax), np.float32)
    e_tgt, e_pm = np.zeros((S, F, Nmax, 12, 2), np.float32), np.zeros((S, Nmax), np.uint8)
    for s, n in enumerate(n_active):
        for j in range(n):
            for t in range(8):
                e_pos[s, t, j] = col(pos_col[s, t, j])
            e_vis[s, :, j] = vis[:, int(vis_off[s]) + j]
            for step in range(12):
                e_tgt[s, :, j, step] = col(tgt_col[s, j, step])
            e_pm[s, j] = int((tgt_col[s, j] >= 0).all())
    for k, want in (("pos", e_pos), ("vislet", e_vis), ("targets", e_tgt), ("ped_mask", e_pm)):
        assert np.array_equal(host(o[k]), want), k
    print("scene_gather: exact")


def test_nri_ops_at_minimum_alignment(lib):
    rng = np.random.default_rng(5100)
    rows, cols = 2, 65
    adj = f32(rng, rows, cols, scale=4.0)
    r = {}
    for entry, fn, want in (("g2k_infer_rlns_f32", lib.g2k_infer_rlns_f32, ref.infer_rlns(adj)),
                            ("g2k_eval_rln_ngh_f32", lib.g2k_eval_rln_ngh_f32, ref.eval_rln_ngh(adj))):
        def run(b):
            a, out = b.put("adj", adj), b.out("out", adj.shape)
            ok(lib, fn(ptr(a), ptr(out), rows, cols, None))
            b.ar.check_guards()
            assert all_written(out)
            return dict(out=out)
        up(r, entry, close(host(twice(entry, entry, run)["out"]), want) / TOL)
    report("nri ops", r)


# ---------------------------------------------------------------------------
# the heads' evaluations, both heads: targets +8, pred / head / chol and the
# float outputs +4, ped_mask +1, sums_i and the doubles +8, per_ped (float4
# stores) +0, the workspace at its minimum
# ---------------------------------------------------------------------------
from tests import bestk_ref, calib_ref, fullcov_joint_ref, joint_ref, kde_ref  # noqa: E402
from tests import fullcov_ref as fr  # noqa: E402
from tests import mix_eval_ref as me  # noqa: E402
from tests import mixture_ref as mr  # noqa: E402
from tests import scores_ref  # noqa: E402

MASK64 = (1 << 64) - 1


def eval_inputs(S=3, F=3, Nmax=7, seed=8400):
    rng = np.random.default_rng(seed)
    n_active = ([Nmax, 0, max(1, Nmax // 2)] + [Nmax] * S)[:S]
    n_frames = ([F, 2, 1] + [F] * S)[:S]
    mask = (rng.random((S, Nmax)) > 0.3).astype(np.uint8)
    mask[:, 0] = 1
    pred = f32(rng, S, F, 24, Nmax)
    tgt = (np.transpose(pred.reshape(S, F, 2, 12, Nmax), (0, 1, 4, 3, 2))
           + f32(rng, S, F, Nmax, 12, 2, scale=0.5)).astype(np.float32)
    head = draw_head(rng, edge=False)
    head[2] = 0.5 * rng.standard_normal(12)
    chol = (fr.block_factor(head) + np.tril(0.05 * rng.standard_normal((24, 24)), -1)).astype(np.float32)
    # the mixture: live slots 0, 2, 5 with dead ones between them, NaN in the
    # dead slots, in floats 1..7 and above the diagonals (its own generators)
    mix = me.mix_block(0.3, seed)
    assert list(np.flatnonzero(mix[:, 0])) == [0, 2, 5] and np.isnan(mix[1, 8]) and np.isnan(mix[0, 1])
    return dict(S=S, F=F, Nmax=Nmax, n_active=n_active, n_frames=n_frames, mask=mask, pred=pred, tgt=tgt,
                head=head, chol=chol, mix=mix,
                pairs=bestk_ref.pair_mask(S, F, Nmax, n_active, n_frames, mask))


def pair_inputs(b, c, hname, harr):
    return [b.put("pred", c["pred"]), b.put("targets", c["tgt"]), b.put("n_active", c["n_active"], np.int32),
            b.put("n_frames", c["n_frames"], np.int32), b.put("ped_mask", c["mask"]), b.put(hname, harr)]


HEADS = [("head", ""), ("chol", "fullcov_"), ("mix", "mix_")]
HEAD_IDS = ["per-step", "fullcov", "mix"]


@pytest.mark.parametrize("hname,stem", HEADS, ids=HEAD_IDS)
def test_best_of_k_at_minimum_alignment(lib, hname, stem):
    c = eval_inputs()
    S, F, N, K, seed = c["S"], c["F"], c["Nmax"], 8, 2 ** 32 - 3
    entry = f"g2k_{stem}best_of_k_f32"
    d = dims(S=S, F=F, Nmax=N)
    nws = int(getattr(lib, f"g2k_{stem}best_of_k_workspace_bytes")(ctypes.byref(d)))
    assert nws > 0

    def run(b):
        ins = pair_inputs(b, c, hname, c[hname])
        per, best, out = b.out("per_ped", (S, F, N, 4)), b.out("best", (S, F, 24, N)), b.out("out", (S, 8))
        ws = b.out("workspace", (nws,), U8)
        ok(lib, getattr(lib, entry)(ctypes.byref(d), *[ptr(t) for t in ins], ctypes.c_uint64(seed), K,
                                    ptr(per), ptr(best), ptr(out), ptr(ws), nws, None))
        b.ar.check_guards()
        assert all_written(per) and all_written(best) and all_written(out)
        return dict(per_ped=per, best=best, out=out)

    at = offsets_at_minimum(entry)
    assert (at["targets"], at["per_ped"], at["workspace"], at["pred"], at[hname]) == (8, 0, 4, 4, 4)
    o = twice(entry, entry, run)
    R = {"head": bestk_ref, "chol": fr, "mix": mr}[hname].best_of_k_ref(
        c["pred"], c["tgt"], c["n_active"], c[hname], seed, K, c["n_frames"], c["mask"])
    per, out, best = host(o["per_ped"]).astype(np.float64), host(o["out"]).astype(np.float64), host(o["best"])
    m = c["pairs"]
    assert np.all(per[~m] == 0) and np.all(out[:, 6:] == 0)
    np.testing.assert_array_equal(out[:, 2], R["out"][:, 2])
    np.testing.assert_array_equal(out[:, 5], R["out"][:, 5])
    off = ~np.broadcast_to(m[:, :, None, :], best.shape)
    assert np.array_equal(best[off].view(np.int32), c["pred"][off].view(np.int32))    # pred elsewhere
    report(entry, {"per_ped": close(per[..., :2], R["per_ped"][..., :2]) / TOL,
                   "out": close(out[:, :5], R["out"][:, :5]) / TOL})


@pytest.mark.parametrize("hname,stem", HEADS, ids=HEAD_IDS)
def test_joint_eval_at_minimum_alignment(lib, hname, stem):
    c = eval_inputs(seed=8500)
    S, F, N, K, seed, radius = c["S"], c["F"], c["Nmax"], 8, 11, 0.3
    entry = f"g2k_{stem}joint_eval_f32"
    d = dims(S=S, F=F, Nmax=N)
    nws = int(getattr(lib, f"g2k_{stem}joint_eval_workspace_bytes")(ctypes.byref(d)))
    assert nws > 0

    def run(b):
        ins = pair_inputs(b, c, hname, c[hname])
        pf, pi = b.out("per_frame_f", (S, F, 4)), b.out("per_frame_i", (S, F, 6), torch.int32)
        sf, si = b.out("sums_f", (S, 4)), b.out("sums_i", (S, 6), torch.int64)
        ws = b.out("workspace", (nws,), U8)
        ok(lib, getattr(lib, entry)(ctypes.byref(d), *[ptr(t) for t in ins], ctypes.c_uint64(seed), K,
                                    radius, ptr(pf), ptr(pi), ptr(sf), ptr(si), ptr(ws), nws, None))
        b.ar.check_guards()
        out = dict(per_frame_f=pf, per_frame_i=pi, sums_f=sf, sums_i=si)
        assert all(all_written(t) for t in out.values())
        return out

    at = offsets_at_minimum(entry)
    assert (at["targets"], at["sums_i"], at["workspace"], at["per_frame_i"]) == (8, 8, 4, 4)
    o = twice(entry, entry, run)
    R = {"head": joint_ref, "chol": fullcov_joint_ref, "mix": me}[hname].joint_eval_ref(
        c["pred"], c["tgt"], c["n_active"], c[hname], seed, K, radius, c["n_frames"], c["mask"])
    pf, sf = host(o["per_frame_f"]).astype(np.float64), host(o["sums_f"]).astype(np.float64)
    pi, si = host(o["per_frame_i"]).astype(np.int64), host(o["sums_i"])
    np.testing.assert_array_equal(pi[..., :2], R["per_frame_i"][..., :2])                # P, PP
    np.testing.assert_array_equal(si, pi.sum(axis=1))
    assert np.all(sf[:, 2] == K) and np.all(sf[:, 3] == 0)
    empty = R["per_frame_i"][..., 0] == 0
    assert np.all(pf[empty] == 0) and np.all(pi[empty] == 0)
    lo_k, hi_k = R["col_lo"].sum(axis=0), R["col_hi"].sum(axis=0)
    for col, lo, hi in ((2, R["pred_lo"], R["pred_hi"]), (3, R["gt_lo"], R["gt_hi"]), (4, lo_k, hi_k)):
        assert np.all((lo <= pi[..., col]) & (pi[..., col] <= hi)), col                  # the checker's bracket
    report(entry, {"per_frame_f": close(pf[..., :2], R["per_frame_f"][..., :2]) / TOL,
                   "sums_f": close(sf[:, :2], R["sums_f"][:, :2]) / TOL})


@pytest.mark.parametrize("hname,stem", HEADS, ids=HEAD_IDS)
def test_kde_nll_at_minimum_alignment(lib, hname, stem):
    """The float64 checker runs over the device's own K draws (the samplers at
    +0), held to tests/kde_ref.py's gate as tests/test_kde_nll_gpu.py does (the
    mixture head: tests/mix_eval_ref.py's, as tests/test_mix_eval_gpu.py);
    the samplers themselves at their minimum are compared with those draws."""
    c = eval_inputs(seed=8600)
    S, F, N, K, seed, floor = c["S"], c["F"], c["Nmax"], 8, 2 ** 64 - 3, -20.0
    entry, sampler = f"g2k_{stem}kde_nll_f32", f"g2k_{stem or 'gauss_'}sample_f32"
    d = dims(S=S, F=F, Nmax=N)
    nws = int(getattr(lib, f"g2k_{stem}kde_nll_workspace_bytes")(ctypes.byref(d)))
    assert nws == S * F * 32

    def draw(k):
        def run(b):
            ins = [b.put("pred", c["pred"]), b.put(hname, c[hname])]
            out = b.out("out", c["pred"].shape)
            tail = (None, None) if hname == "mix" else (None,)            # the mixture's: comp = NULL
            ok(lib, getattr(lib, sampler)(ctypes.byref(d), ptr(ins[0]), ptr(ins[1]),
                                          ctypes.c_uint64((seed + k) & MASK64), ptr(out), *tail))
            b.ar.check_guards()
            assert all_written(out)
            return dict(out=out)
        return run

    draws = np.stack([host(twice(f"{sampler} draw {k}", sampler, draw(k))["out"]) for k in range(K)])
    if hname == "chol":      # the full-covariance sampler against its float64 restatement
        report(sampler, {"draw": close(draws[0], fr.sample(c["pred"], c["chol"], seed & MASK64)) / TOL})

    def run(b):
        ins = pair_inputs(b, c, hname, c[hname])
        per, out, ws = b.out("per_ped", (S, F, N, 4)), b.out("out", (S, 8)), b.out("workspace", (nws,), U8)
        ok(lib, getattr(lib, entry)(ctypes.byref(d), *[ptr(t) for t in ins], ctypes.c_uint64(seed), K, floor,
                                    ptr(per), ptr(out), ptr(ws), nws, None))
        b.ar.check_guards()
        assert all_written(per) and all_written(out)
        return dict(per_ped=per, out=out)

    at = offsets_at_minimum(entry)
    assert (at["targets"], at["per_ped"], at["workspace"]) == (8, 0, 4)
    o = twice(entry, entry, run)
    if hname == "mix":
        R, gate = me.kde_nll_ref(draws, c["tgt"], c["pairs"], floor), me.GATE
    else:
        R, gate = kde_ref.kde_nll_ref(draws, c["tgt"], c["pairs"], floor), kde_ref.GATE
    per, out = host(o["per_ped"]).astype(np.float64), host(o["out"]).astype(np.float64)
    m, npairs = c["pairs"], R["out"][:, 2]
    assert np.all(per[~m] == 0)
    np.testing.assert_array_equal(out[:, 2], npairs)
    assert np.all(out[:, 4] == K) and np.all(out[:, 5] == floor) and np.all(out[:, 6:] == 0)
    report(entry, {"per pair": float(np.abs(per[..., :2] - R["per_ped"][..., :2]).max()) / gate,
                   "per scene": float((np.abs(out[:, :2] - R["out"][:, :2]).max(axis=1)
                                       / (gate * np.maximum(npairs, 1))).max())})


@pytest.mark.parametrize("hname,stem", [("head", "head_"), ("chol", "fullcov_")], ids=["per-step", "fullcov"])
def test_stats_at_minimum_alignment(lib, hname, stem):
    """1344 slots: more than one workgroup, so the workspace (+8) is used;
    r2, stats, moments, inside +8, fit +4."""
    c = eval_inputs(S=3, F=14, Nmax=32, seed=8700)
    S, F, N = c["S"], c["F"], c["Nmax"]
    entry = f"g2k_{stem}stats_f32"
    levels = (0.5, 0.9)
    full = hname == "chol"
    r2 = fr.levels_r2(levels) if full else calib_ref.levels_r2(levels)
    NL = len(levels)
    d = dims(S=S, F=F, Nmax=N)
    nws = int(getattr(lib, f"g2k_{stem}stats_workspace_bytes")(ctypes.byref(d), NL))
    assert nws > 0

    def run(b):
        ins = pair_inputs(b, c, hname, c[hname]) + [b.put("r2", np.asarray(r2, np.float64))]
        out = {}
        if full:
            out["moments"] = b.out("moments", (25, 24), torch.float64)
        out["stats"] = b.out("stats", (12, 4 if full else 8), torch.float64)
        out["inside"] = b.out("inside", (13 if full else 12, NL), torch.int64)
        out["fit"] = b.out("fit", (24, 24) if full else (3, 12))
        ws = b.out("workspace", (nws,), U8)
        ok(lib, getattr(lib, entry)(ctypes.byref(d), *[ptr(t) for t in ins], NL,
                                    *[ptr(out[k]) for k in (("moments",) if full else ()) + ("stats", "inside", "fit")],
                                    ptr(ws), nws, None))
        b.ar.check_guards()
        assert all(all_written(t) for t in out.values())
        return out

    at = offsets_at_minimum(entry)
    assert (at["targets"], at["r2"], at["stats"], at["inside"], at["workspace"], at["fit"]) == (8, 8, 8, 8, 8, 4)
    o = twice(entry, entry, run)
    st, ins, fit, r = host(o["stats"]), host(o["inside"]), host(o["fit"]).astype(np.float64), {}
    n = int(c["pairs"].sum())
    np.testing.assert_array_equal(st[:, 0], np.full(12, n, np.float64))
    if full:
        R = fr.stats_ref(c["pred"], c["tgt"], c["n_active"], c["chol"], r2, c["n_frames"], c["mask"])
        mo = host(o["moments"])
        up(r, "moments", np.max(np.abs(mo - R["moments"]) / np.maximum(1.0, np.abs(R["moments"]))) / 1e-12)
        up(r, "stats", np.max(np.abs(st - R["stats"]) / np.maximum(1.0, np.abs(R["stats"]))) / 1e-12)
        up(r, "fit fit^T", np.abs(fit @ fit.T - R["C"]).max() / np.abs(R["C"]).max() / 1e-4)
    else:
        R = calib_ref.head_stats_ref(c["pred"], c["tgt"], c["n_active"], c["head"], r2, c["n_frames"], c["mask"])
        for col in range(1, 6):
            up(r, "moment sums", np.max(np.abs(st[:, col] - R["stats"][:, col]) / R["abs"][:, col]) / 1e-11)
        for col in (6, 7):
            up(r, "nll / q sums", np.max(np.abs(st[:, col] - R["stats"][:, col])
                                         / np.maximum(1.0, np.abs(R["stats"][:, col]))) / 1e-9)
        up(r, "fit", np.max(np.abs(fit - R["fit"]) / np.maximum(1.0, np.abs(R["fit"]))) / 1e-6)
    np.testing.assert_array_equal(ins, R["inside"])
    report(entry, r)


def test_workspace_init_at_minimum_alignment(lib):
    """A memset: any address.  The workspace one byte past a 16-byte boundary,
    an odd byte count: exactly those bytes are zero, the guards keep theirs."""
    n = 77

    def run(b):
        ws = b.out("workspace", (n,), U8)
        ok(lib, lib.g2k_workspace_init(ptr(ws), n, None))
        b.ar.check_guards()
        return dict(workspace=ws)

    assert offsets_at_minimum("g2k_workspace_init") == {"workspace": 1}
    o = twice("workspace_init", "g2k_workspace_init", run)
    assert not host(o["workspace"]).any()
    print("workspace_init: exact")


# ---------------------------------------------------------------------------
# include/g2k_mix.h and include/g2k_scores.h: the EM step, the mixture's
# sampler and the three heads' sample scores (the mixture's best-of-K, joint
# evaluation and KDE-NLL are the third case of the head tests above)
# ---------------------------------------------------------------------------
def em_inputs():
    """eval_inputs' scenes (a mask, an empty and a short scene) with targets a
    few component sigma from pred + b_m, as tests/test_mixture_gpu.py draws
    them (its 0.05 scale: a component's covariance is then well inside what two
    float64 evaluations agree on), the three components dealt in turn, and NaN
    in every non-pair of pred and targets."""
    from tests.test_mixture_gpu import _block
    c = dict(eval_inputs(seed=8800))
    S, F, N = c["S"], c["F"], c["Nmax"]
    rng = np.random.default_rng(8801)
    slots = (0, 2, 5)
    mix = _block(rng, slots)
    k = np.asarray(slots)[np.arange(S * F * N).reshape(S, F, N) % 3]
    r = np.empty((S, F, N, 24))
    for m in slots:
        Lm = np.tril(np.nan_to_num(mix[m, 32:].reshape(24, 24).astype(np.float64)))
        r[k == m] = 1.3 * mix[m, 8:32] + rng.standard_normal((int((k == m).sum()), 24)) @ (1.2 * Lm).T
    pred = c["pred"].copy()
    tg = np.empty((S, F, N, 12, 2))
    tg[..., 0] = np.transpose(pred[:, :, :12], (0, 1, 3, 2)) + r[..., 0::2]
    tg[..., 1] = np.transpose(pred[:, :, 12:], (0, 1, 3, 2)) + r[..., 1::2]
    tg = np.ascontiguousarray(tg.astype(np.float32))
    m = c["pairs"]
    np.transpose(pred, (0, 1, 3, 2))[~m] = np.nan
    tg[~m] = np.nan
    c.update(pred=pred, tgt=tg, mix=mix, slots=slots)
    return c


@pytest.mark.parametrize("with_out", [True, False], ids=["mix_out", "e-step-only"])
def test_mix_em_at_minimum_alignment(lib, with_out):
    """targets, moments, resp, total and the workspace +8, pred, the block in
    and out, n_active, n_frames +4, ped_mask +1, +2, +3.  The bounds are
    tests/test_mixture_gpu.py's (its _check_em_step)."""
    from tests.test_mixture_gpu import _check_em_step
    c = em_inputs()
    S, F, N = c["S"], c["F"], c["Nmax"]
    entry = "g2k_mix_em_f32"
    d = dims(S=S, F=F, Nmax=N)
    nws = int(lib.g2k_mix_em_workspace_bytes(ctypes.byref(d)))
    assert nws == 8 * (8 * S * F * N + 10 + 8 * 448)
    R = mr.em_ref(c["pred"], c["tgt"], c["n_active"], c["mix"], c["n_frames"], c["mask"])
    g = np.sort(R["gamma"], axis=1)
    assert R["total"][0] == c["pairs"].sum() > 12 and (g[:, -1] - g[:, -2]).min() > 1e-9
    assert np.all(R["resp"][list(c["slots"]), 0] > 2.0)

    def run(b):
        ins = pair_inputs(b, c, "mix_in", c["mix"])
        mo, rs = b.out("moments", (8, 25, 24), torch.float64), b.out("resp", (8, 2), torch.float64)
        tt, out = b.out("total", (4,), torch.float64), b.out("mix_out", (8, 608))
        ws = b.out("workspace", (nws,), U8)
        ok(lib, lib.g2k_mix_em_f32(ctypes.byref(d), *[ptr(t) for t in ins], ptr(mo), ptr(rs), ptr(tt),
                                   ptr(out) if with_out else None, ptr(ws), nws, None))
        b.ar.check_guards()
        assert all_written(mo) and all_written(rs) and all_written(tt)
        assert all_written(out) if with_out else bool(untouched(out).all())
        assert np.array_equal(bits(ins[5]).cpu().numpy(), c["mix"].view(np.int32))       # the block: read only
        return dict(moments=mo, resp=rs, total=tt, mix_out=out)

    at = offsets_at_minimum(entry)
    assert (at["targets"], at["moments"], at["resp"], at["total"], at["workspace"]) == (8, 8, 8, 8, 8)
    assert (at["pred"], at["mix_in"], at["mix_out"], at["n_active"], at["ped_mask"]) == (4, 4, 4, 4, 1)
    name = entry + ("" if with_out else " (mix_out NULL)")
    o = every_mask(name, entry, run)
    out = host(o["mix_out"]) if with_out else R["mix_out"]          # NULL: the E-step's outputs only
    r = _check_em_step(name, host(o["moments"]), host(o["resp"]), host(o["total"]), out, R, list(c["slots"]))
    if not with_out:
        r = {k: r[k] for k in ("moments", "resp", "total")}
    report(name, r)


def test_mix_sample_at_minimum_alignment(lib):
    """pred, mix, out and comp +4; then in place (out == pred) at +4: the bits
    of the separate output."""
    c = eval_inputs(seed=8900)
    S, F, N, seed = c["S"], c["F"], c["Nmax"], 2 ** 64 - 5
    entry = "g2k_mix_sample_f32"
    d = dims(S=S, F=F, Nmax=N)

    def run(b):
        pred, mix = b.put("pred", c["pred"]), b.put("mix", c["mix"])
        out, comp = b.out("out", c["pred"].shape), b.out("comp", (S, F, N), torch.int32)
        ok(lib, lib.g2k_mix_sample_f32(ctypes.byref(d), ptr(pred), ptr(mix), ctypes.c_uint64(seed), ptr(out),
                                       ptr(comp), None))
        b.ar.check_guards()
        assert all_written(out) and all_written(comp)
        assert np.array_equal(host(pred).view(np.int32), c["pred"].view(np.int32))       # read only
        return dict(out=out, comp=comp)

    def in_place(b):
        pred, mix = b.put("pred", c["pred"]), b.put("mix", c["mix"])
        ok(lib, lib.g2k_mix_sample_f32(ctypes.byref(d), ptr(pred), ptr(mix), ctypes.c_uint64(seed), ptr(pred),
                                       None, None))
        b.ar.check_guards()
        return dict(out=pred)

    at = offsets_at_minimum(entry)
    assert at == dict(pred=4, mix=4, out=4, comp=4)
    o = twice(entry, entry, run)
    ip = twice(entry + " in place", entry, in_place)
    compare(entry + " in place against the separate output", dict(out=o["out"]), ip)
    ref, rcomp = mr.sample(c["pred"], c["mix"], seed)
    np.testing.assert_array_equal(host(o["comp"]), rcomp)
    assert set(np.unique(rcomp)) == {0, 2, 5} and np.all(np.isfinite(host(o["out"])))
    report(entry, {"draw": close(host(o["out"]), ref) / TOL})


SCORE_SAMPLERS = {"head": "g2k_gauss_sample_f32", "chol": "g2k_fullcov_sample_f32", "mix": "g2k_mix_sample_f32"}


@pytest.mark.parametrize("F", [3, 20], ids=["f3", "f20-rows"])
@pytest.mark.parametrize("hname,stem", HEADS, ids=HEAD_IDS)
def test_sample_scores_at_minimum_alignment(lib, hname, stem, F):
    """targets +8, per_ped (two float4 stores a pair) +0, the workspace, pred,
    the head's parameters, out, n_active and n_frames +4, ped_mask +1, +2, +3;
    K = 5.  F = 3 is one workgroup a scene; F = 20 two (18 frames, then 2), so
    the workspace at +4 holds the rows that g2k_scores_rows_kernel adds.  The
    float64 checker runs over the device's own K draws (the head's sampler at
    +0), held to tests/scores_ref.py's TOL as tests/test_sample_scores_gpu.py
    does."""
    c = eval_inputs(F=F, seed=9000)
    S, N, K, seed = c["S"], c["Nmax"], 5, 2 ** 32 - 2
    entry = f"g2k_{stem}sample_scores_f32"
    d = dims(S=S, F=F, Nmax=N)
    nws = int(lib.g2k_sample_scores_workspace_bytes(ctypes.byref(d)))
    assert nws == S * F * 32
    geom = (ctypes.c_int32 * 5)()
    assert lib.g2k_sample_scores_geometry(ctypes.byref(d), K, geom) == 0
    assert (geom[2], geom[3]) == ((3, 1) if F == 3 else (18, 2))      # FC, C

    def run(b):
        ins = pair_inputs(b, c, hname, c[hname])
        per, out, ws = b.out("per_ped", (S, F, N, 8)), b.out("out", (S, 8)), b.out("workspace", (nws,), U8)
        ok(lib, getattr(lib, entry)(ctypes.byref(d), *[ptr(t) for t in ins], ctypes.c_uint64(seed), K, ptr(per),
                                    ptr(out), ptr(ws), nws, None))
        b.ar.check_guards()
        assert all_written(per) and all_written(out)
        return dict(per_ped=per, out=out)

    at = offsets_at_minimum(entry)
    assert (at["targets"], at["per_ped"], at["workspace"], at["pred"], at[hname], at["out"]) == (8, 0, 4, 4, 4, 4)
    o = every_mask(f"{entry} F={F}", entry, run)

    def draw(k):
        ar = Arena("cuda")
        pred, prm, out = ar.put(c["pred"], "pred"), ar.put(c[hname], hname), ar.alloc(c["pred"].shape, name="out")
        tail = (None, None) if hname == "mix" else (None,)
        ok(lib, getattr(lib, SCORE_SAMPLERS[hname])(ctypes.byref(d), ptr(pred), ptr(prm),
                                                    ctypes.c_uint64((seed + k) & MASK64), ptr(out), *tail))
        ar.check_guards()
        return host(out)

    R = scores_ref.sample_scores_ref(np.stack([draw(k) for k in range(K)]), c["tgt"], c["pairs"])
    per, out = host(o["per_ped"]).astype(np.float64), host(o["out"]).astype(np.float64)
    m, npairs = c["pairs"], R["out"][:, 7]
    assert np.all(per[~m] == 0) and np.all(per[..., 7] == 0) and m.sum() > 12
    np.testing.assert_array_equal(out[:, 7], npairs)
    gate = lambda ref: scores_ref.TOL * np.maximum(1.0, np.abs(ref))      # noqa: E731
    report(f"{entry} F={F}", {"per pair": float((np.abs(per[..., :7] - R["per_ped"][..., :7])
                                                 / gate(R["per_ped"][..., :7])).max()),
                              "per scene": float((np.abs(out[:, :7] - R["out"][:, :7])
                                                  / (gate(R["out"][:, :7])
                                                     * np.maximum(npairs, 1)[:, None])).max())})
