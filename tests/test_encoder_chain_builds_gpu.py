"""GPU: every build of g2k_encoder_chain_kernel<TPW, U, FS> against the float64
oracle (tests/chain_cases.py: the case table and chain_ref), through the raw C
ABI with every output in a guarded, poisoned arena.

The twelve builds (H 64 / 128 / 256 / 512 x num_units 1 / 2 / 4), each with
and without peepholes, each in a launch of its own from an O(1) h0 (only the
first frame of a launch sees the cell's state wiring: chain_cases.py), over
batches that are skipped before, between and after the running ones, a
one-frame batch, both parities of the X double buffer and a pred that is
formed after a batch boundary and after the last frame.  Then the edges:
Nmax 1 and 256, n_frames outside [0, F], a launch without frames, NaN in
every inactive input, the attention tile's widest main-path columns and its
fallback, a wide h0, repeated calls; and EncoderChain.run at strides 1 and 2
against oracle.scene_step(encoder=) chained batch after batch.

Bounds: Xe, cost, pred and cell_state |d| <= 1e-4 max(1, |ref|) (close); attn
normwise, |dA| <= 1e-4 max(1, max |A|); h by close_h; pred's columns >=
n_active exact zeros; everything a launch does not run untouched.

XE_BOUND, a tighter bound on Xe.  The cell is three dot products of at most
16 terms, two sigmoids and three tanh per unit (each ~2e-7, csrc/g2k_ops.hip)
on values in (-1, 1), so |Xe - oracle| has no reason to come near 1e-4; at
1e-4 frames 1 and 2 of a launch would say nothing about the LDS hand-off of
h (a state error moves them by 1e-2 .. 1e-4 only).  MEASURED on an MI355X
over the 24 launches of test_build_matches_oracle (each prints its figure):
worst |Xe - oracle| = 1.444e-07 (build-h256-u4-peep; the 24 lie in 4.7e-08 ..
1.45e-07, and no build, H or peephole setting stands out), which agrees with
the kernel's claim.  XE_BOUND = 6e-07 is 4 x that, rounded up to one digit
(the margin is for compiler and box-to-box spread).  The edge launches from an
O(1) h0 are held to the same bound (their worst: 1.74e-07, nan-h64-u4); the
h0 = 10 N(0, 1) launch, whose cell state is ten times wider than what the
bound was measured on, stays at 1e-4 (measured 3.5e-07).
"""
import ctypes

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib
from multimodaltraj_2_amd import frame_step as fs
from multimodaltraj_2_amd.encoder_step import EncoderChain
from multimodaltraj_2_amd.helper import neighborhood_vis_loc_encoder
from multimodaltraj_2_amd.synthetic import make_batch
from oracle import g2k_ref as ref
from tests import chain_cases as cc
from tests.abi_arena import Arena, untouched
from tests.conftest import close, close_h
from tests.test_ops_domain_gpu import abi_weights, dev, dims, host, ok, ptr

pytestmark = pytest.mark.gpu
TOL = 1e-4
D = cc.D
NAN = np.float32("nan")
MEASURED_XE = 1.444e-7    # worst |Xe - oracle| of the 24 build launches on an MI355X
XE_BOUND = 6e-7           # 4 x MEASURED_XE, rounded up to one digit
OUTS = ("Xe", "cell_state", "attn", "cost", "pred", "h")


@pytest.fixture
def lib(gpu):
    return _lib.load()


def launch(lib, case, inp):
    """One g2k_encoder_chain_f32 call on the case's inputs; every output from a
    poisoned arena (h: h0 between guards).  Returns device views by name."""
    S, F, N = case.S, case.F, case.Nmax
    inp = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in inp.items()}   # shared ones are read-only
    inp["w"] = {k: v.copy() for k, v in inp["w"].items()}
    ar = Arena("cuda")
    o = dict(Xe=ar.alloc((S, F, D + 2, D), name="Xe"), cell_state=ar.alloc((D, D), name="cell_state"),
             attn=ar.alloc((S, F, D, D), name="attn"), cost=ar.alloc((S, F, 8, 8), name="cost"),
             pred=ar.alloc((S, F, 24, N), name="pred"), h=ar.put(inp["h0"], "h"))
    ws, keep = abi_weights(inp["w"])
    ins = [dev(inp["X"]), dev(inp["Rel"]), dev(inp["G"]), dev(inp["n_active"], np.int32),
           dev(inp["n_frames"], np.int32), dev(inp["cW"]), dev(inp["cb"]),
           None if inp["cP"] is None else dev(inp["cP"])]
    ok(lib, lib.g2k_encoder_chain_f32(ctypes.byref(dims(S=S, F=F, H=case.H, Nmax=N)), ctypes.byref(ws),
                                      *[ptr(t) for t in ins], case.fs, case.u, ptr(o["Xe"]),
                                      ptr(o["cell_state"]), ptr(o["attn"]), ptr(o["cost"]),
                                      ptr(o["pred"]), ptr(o["h"]), cc.LAM, None))
    ar.check_guards()
    return o


def bits(o):
    """Every output's bits on the host (NaN patterns compare)."""
    return {k: host(o[k]).view(np.int32) for k in OUTS}


def check_footprint(case, inp, o):
    """What a launch may write: Xe = X outside rows 0..D-1 of the run frames;
    attn, cost and pred of the run frames and nothing else; cell_state iff a
    frame ran; pred's columns >= n_active exact zeros."""
    run, X = case.run, inp["X"]
    Xe = host(o["Xe"])
    assert np.array_equal(Xe[~run].view(np.int32), X[~run].view(np.int32))
    assert np.array_equal(Xe[:, :, D:].view(np.int32), X[:, :, D:].view(np.int32))
    for k in ("attn", "cost", "pred"):
        keep = host(untouched(o[k])).reshape(case.S, case.F, -1)
        assert keep[~run].all() and not keep[run].any(), k
    cs_kept = host(untouched(o["cell_state"]))
    assert cs_kept.all() if not run.any() else not cs_kept.any()
    assert not host(untouched(o["h"])).any()
    pred = host(o["pred"])
    for s, nf in enumerate(case.frames):
        n = min(max(int(case.n_active[s]), 0), case.Nmax)
        assert np.all(pred[s, :nf, :, n:].view(np.int32) == 0)               # exactly +0


def check_parity(case, inp, want, o):
    """The run frames against chain_ref; returns the worst |Xe - oracle|."""
    run = case.run
    Xe, attn, cost, pred = (host(o[k]) for k in ("Xe", "attn", "cost", "pred"))
    assert all(np.isfinite(a[run]).all() for a in (Xe, attn, cost, pred))
    worst = 0.0
    for s, f in zip(*np.nonzero(run)):
        assert close(Xe[s, f, :D], want["Xe"][s, f]) <= TOL
        worst = max(worst, float(np.abs(Xe[s, f, :D] - want["Xe"][s, f]).max()))
        A = want["attn"][s, f]
        assert np.abs(attn[s, f] - A).max() <= TOL * max(1.0, np.abs(A).max())
        assert close(cost[s, f], want["cost"][s, f]) <= TOL
        assert close(pred[s, f], want["pred"][s, f]) <= TOL
    assert close(host(o["cell_state"]), want["state"]) <= TOL
    assert close_h(host(o["h"]), want["h"])
    return worst


def run_case(lib, case, xe_bound=XE_BOUND):
    inp, want = cc.reference(case)
    o = launch(lib, case, inp)
    check_footprint(case, inp, o)
    worst = check_parity(case, inp, want, o)
    print(f"{case.id}: worst |Xe - oracle| = {worst:.3e} (bound {xe_bound:.0e})")
    assert worst <= xe_bound
    return inp, want, o


# ---------------------------------------------------------------------------
# every build
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.BUILD_CASES, ids=lambda c: c.id)
def test_build_matches_oracle(lib, case):
    assert 4 * MEASURED_XE <= XE_BOUND < 1e-5
    run_case(lib, case)


# ---------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.NMAX_CASES, ids=lambda c: c.id)
def test_nmax_1_and_256(lib, case):
    run_case(lib, case)


@pytest.mark.parametrize("case", cc.CLAMP_CASES, ids=lambda c: c.id)
def test_n_frames_outside_the_range_are_clamped(lib, case):
    _, _, o = run_case(lib, case)
    twin = cc.clamped_twin(case)
    o2 = launch(lib, twin, cc.build(twin))
    a, b = bits(o), bits(o2)
    for k in OUTS:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("case", cc.NONE_CASES, ids=lambda c: c.id)
def test_launch_without_frames(lib, case):
    inp, _ = cc.reference(case)
    o = launch(lib, case, inp)
    check_footprint(case, inp, o)          # Xe == X; attn, cost, pred, cell_state untouched
    assert np.array_equal(host(o["h"]).view(np.int32), inp["h0"].view(np.int32))   # bit-unchanged


def poisoned(case, inp, wo_from):
    """The inputs with NaN in everything the launch must not read."""
    p = dict(inp, w=dict(inp["w"]))
    X, Rel, G, Wo = inp["X"].copy(), inp["Rel"].copy(), inp["G"].copy(), inp["w"]["Wo"].copy()
    X[~case.run] = NAN
    for s, nf in enumerate(case.frames):
        if nf == 0:
            Rel[s], G[s] = NAN, NAN
    Wo[:, wo_from:] = NAN
    p.update(X=X, Rel=Rel, G=G)
    p["w"]["Wo"] = Wo
    return p


@pytest.mark.parametrize("case", cc.NAN_CASES, ids=lambda c: c.id)
def test_inactive_inputs_are_never_read(lib, case):
    inp, _, o = run_case(lib, case)
    widest = max(n for n, nf in zip(case.n_active, case.frames) if nf > 0)
    twin = cc.wo_twin(case)                # every n_active <= 1: Wo's columns >= 1 inactive
    for c, clean, wo_from in ((case, o, widest), (twin, None, 1)):
        ci = cc.build(c)
        if clean is None:
            clean = launch(lib, c, ci)
        pin = poisoned(c, ci, wo_from)
        dirty = launch(lib, c, pin)
        check_footprint(c, pin, dirty)     # Xe == the poisoned X where nothing ran
        a, b = bits(clean), bits(dirty)
        run = c.run
        for k in ("cell_state", "attn", "cost", "pred", "h"):
            assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a["Xe"][run][:, :D], b["Xe"][run][:, :D])
        assert np.isfinite(host(dirty["h"])).all() and np.isfinite(host(dirty["pred"])[run]).all()


@pytest.mark.parametrize("case", cc.LOGIT_CASES, ids=lambda c: c.id)
def test_large_logits_inside_the_chain(lib, case):
    run_case(lib, case)


def test_wide_h0(lib):
    run_case(lib, cc.WIDE_H0_CASE, xe_bound=TOL)


@pytest.mark.parametrize("case", cc.REPEAT_CASES, ids=lambda c: c.id)
def test_repeated_calls_are_bit_identical(lib, case):
    inp, _ = cc.reference(case)
    a, b = bits(launch(lib, case, inp)), bits(launch(lib, case, inp))
    for k in OUTS:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------
# through Python: EncoderChain.run at strides 1 and 2
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("u", [1, 4])
def test_encoder_chain_run_strided(gpu, u, stride):
    S, F, Nmax, H = 3, 3, 5, 64
    b = make_batch(S, Nmax, H, F=(F - 1) * stride + 1, seed=70 + u, n_active=[5, 3, 1])   # W = (F - 1) stride + T
    t = b.to_device(gpu)
    targets = t["targets"][:, :F].contiguous()
    n_frames = torch.tensor([3, 2, 3], dtype=torch.int32, device=gpu)
    params = fs.init_params(Nmax, seed=1, device=gpu)
    cell = neighborhood_vis_loc_encoder(hidden_size=H, hidden_len=16, num_layers=u, grid_size=2 * u,
                                        embedding_size=64, device=gpu, seed=3).rnn
    h0 = np.random.default_rng(80 + u).standard_normal((1, 16, H)).astype(np.float32)
    h = torch.from_numpy(h0).to(gpu)
    out, _ = EncoderChain(params, cell, lam=cc.LAM).run(t["pos"], t["vislet"], t["G"], targets,
                                                         t["n_active"], n_frames, h, stride=stride)
    torch.cuda.synchronize()
    enc = dict(W=cell.W.cpu().numpy().astype(np.float64), b=cell.b.cpu().numpy().astype(np.float64),
               peep=tuple(cell.peep.cpu().numpy().astype(np.float64)), feature_size=2 * u, num_units=u)
    w = params.numpy()
    pred, met = out.pred.cpu().numpy(), out.metrics.cpu().numpy()
    h_ref = h0[0].astype(np.float64)
    for s in range(S):
        n, nf = int(b.n_active[s]), int(n_frames[s])
        pr, h_ref, m, _ = ref.scene_step(b.pos[s], b.vislet[s], b.G[s], w, b.targets[s, :F], n, h_ref,
                                         n_frames=nf, stride=stride, lam=cc.LAM, encoder=enc)
        assert close(pred[s, :nf, :, :n].reshape(nf, 2, 12, n), pr) <= TOL
        assert np.all(pred[s, :, :, n:] == 0) and np.all(pred[s, nf:] == 0)
        assert close(met[s, :6], m[:6]) <= TOL
    assert close_h(h[0].cpu().numpy(), h_ref)
