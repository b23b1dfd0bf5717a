"""GPU: the stand-alone entry points of the C ABI over the domain
include/g2k_hip.h promises (D in 1..16, H in {64, 128, 256, 512}, Nmax in
1..256, nullable masks, frames >= 0, C in 1..4, out / G either NULL), against
the float64 oracle, with every output in a guarded, pattern-filled arena
(tests/abi_arena.py) so that the header's write footprints are checked too.

Every case calls the raw ABI through ctypes, draws its own weights, compares
with oracle/g2k_ref.py at the project's tolerances (close <= 1e-4, close_h for
h, normwise 1e-4 for A, 1e-6 / 1e-5 for the update) and ends with
check_guards().  Inputs of the ops whose oracle slices [:n] hold NaN in their
inactive parts (columns >= n_active, frames >= n_frames): every output must
be unaffected.  The fused step is exempt (its real-data path zero-fills).

Shapes, per entry point, and the branch each was chosen to reach:

g2k_frame_recurrence_f32
  frames 33 = kRecurChunk + 1: a second LDS chunk, of one frame.  H 64 / 128 /
  256 / 512 = the <1,4> <2,4> <4,4> <8,4> instantiations; D 16 = the DMA
  staging, D 10 / 1 = the scalar staging with padded rows and columns at zero.
  Frame 32 row min(5, D - 1) of scene 0 is raised by +60: a column spread of
  ~60, where exp(A - max) ~ 1e-26 as a rule still stays above the fallback's
  1e-30 threshold (the shifted main path at its widest).  Scene 1's row is
  raised by +100, where the prefix sums underflow for certain: the running
  (max, sum) fallback, in the second chunk (a build without the fallback
  fails these cases at D 16 and 10; D 1 has one row and no prefix).
  frames 0: h bit-unchanged (no step, adj = 1); frames 1: one chunk of one
  frame.
g2k_mcr_forward_f32
  D 16 / 10 / 1 (D 1: one-column E, a [1, 1] A) x Nmax 1 / 17 / 256 (one
  thread's column, an odd width, more than kNT columns per row block);
  n_active Nmax / 1 / 0.  A second launch with n_active <= 1 holds NaN in
  Wo's columns >= 1.  lambda 0.1 so that A, cost and pred are O(1) and the
  absolute floor of `close` does not hide a relative error.
g2k_frame_embed_f32
  Nmax 1 / 30 / 256 x stride 0 / 1 / 2, F 3; n_active Nmax / 0 / about half;
  Rel given and NULL.  n = 0: the pair loops run zero times, X = 0.
g2k_ade_fde_f32 variant 0
  (Nmax, F) (1, 3) / (30, 5) / (256, 2): one task, tasks < kNT, tasks > kNT
  (the task loop wraps); n_frames NULL / [F, 1, F, 0]; ped_mask NULL / one
  scene all masked.
g2k_ade_fde_f32 variant 1
  Nmax 1 / 65 / 256: one lane, the lane loop wrapping by one, four trips;
  n_active 0 -> {0, 0, 0}.
g2k_infer_rlns_f32 / g2k_eval_rln_ngh_f32
  cols 1, 63, 64, 65, 200: below / at / past one wave's width, four trips of
  the strided loops; plus rows of +/-100 (exp overflow without the max shift,
  saturation of the sigmoid) and constant rows.
g2k_gridlstm_f32
  rows 255 / 256 / 257 (the last workgroup's bound check), K = 1 (no
  frequency chain), state_out aliasing state at ld_state == blocks * 2u.
g2k_context_conv_f32
  C 2 / 4 x D 1 / 7 / 16 at Hh = Ww = D + 1 (D 1: 256 slices of one thread;
  D 7: 36 slices, 4 idle threads; D 16: 16 slices), one case at Hh = Ww = D;
  both outputs, out only, G only.
g2k_nll_f32
  Nmax 1 / 7 / 256, F 3, S 4; n_active Nmax / 0 / about half / <= 5; n_frames
  NULL / [3, 0, 2, 1]; ped_mask NULL / scene 0 all zero; head r in [-3, 3]
  with r[0] = 3, r[1] = -3 (c = 1 - rho^2 = 9.9e-3: the cancellation costs
  ~2 rho ulp(rho) / c ~ 1e-5 relative, inside 1e-4; measured below).  One
  launch without any pair.  S 257, F 1, Nmax 3 (tests/eval_cells.py
  "nll-rows257"): 257 rows, the second trip of g2k_grad_rows_kernel's r0 loop.
g2k_gauss_sample_f32
  (S, F, Nmax) (1, 1, 1) / (2, 3, 7) / (1, 2, 256) x seeds 0, 2^32 - 1, 2^32,
  2^64 - 1 (both halves of the 64-bit seed, carries between them).
g2k_update_f32
  P 520 / 1264 / 6676 (Nmax 1, 32, 256 + head: one to seven entries per
  thread of the 1024), 7169 (one entry in the eighth register slot), 8192 (the
  register path full: kPre * 1024), 8193 (the first size on the strided path:
  one thread takes a ninth trip) and 20000 (twenty trips, the last partial),
  pair count 0 (max(count, 1)) and 7, RMSProp / SGD with and without
  clipping; a zero gradient with ms = 0 at P 1264 and the four sizes above.
g2k_scene_gather_f32
  a hand-made plan with -1 slots, vis / vis_off given and NULL.
g2k_encoder_chain_f32
  n_frames [2, 0]: a batch without frames is skipped, its outputs untouched
  (every build and the kernel's other edges: test_encoder_chain_builds_gpu.py).
g2k_step_fused_f32 / g2k_train_step_f32
  n_active 1 / 16 / 17 / 30 at Nmax 30: one tile, a full tile, a second
  (clipped) tile; n_frames 5 / 0 / 3 / 5; band and ped-major; split 1 and 2.

MEASURED on an MI355X where a bound had not been measured before (each test
prints its figure before it asserts):
  stand-alone recurrence, frames 33, worst |dh| / (1e-5 |h| + 1e-8), i.e.
  close_h's bound = 1:   D 16     D 10     D 1
                 H  64   0.011    0.017    < 0.001
                 H 128   0.011    0.016    < 0.001
                 H 256   0.009    0.009    < 0.001
                 H 512   0.008    0.008    < 0.001
  (g2k_recur_kernel's chain is two orders inside the bound at every H; the
  fused step's margin at H = 512 is test_step_h512_long_chain_margin's)
  g2k_nll_f32 with |r| = 3 in the head (bound 1e-4): nll <= 4.4e-6, head
  gradient <= 5.9e-6 (normwise), dpred <= 1.8e-5 (Nmax 256; <= 7e-6 below).
"""
import ctypes

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib
from oracle import g2k_ref as ref
from tests import eval_cells as ec
from tests.abi_arena import Arena, all_written, untouched
from tests.conftest import close, close_h

pytestmark = pytest.mark.gpu
TOL = 1e-4
NAN = np.float32("nan")
U8 = torch.uint8


@pytest.fixture
def lib(gpu):
    return _lib.load()


def dev(a, dtype=None):
    """A host array as a contiguous device tensor (inputs)."""
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))
    return torch.from_numpy(a).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def f32(rng, *shape, scale=1.0):
    return (scale * rng.standard_normal(shape)).astype(np.float32)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def dims(S=1, F=1, D=16, H=64, Nmax=1, W=8, stride=0, flags=0):
    return _lib.G2KDims(S, F, 8, 12, D, H, Nmax, W, stride, flags)


def ok(lib, rc):
    assert rc == 0, lib.g2k_last_error()
    torch.cuda.synchronize()


def host(t):
    return t.cpu().numpy()


def weights(rng, D, Nmax):
    """Host weights of the model at hidden length D (fs.init_params is D = 16 only)."""
    return dict(Wi=f32(rng, Nmax, D), Wii=f32(rng, D, 8), Wv=f32(rng, 8, D + 2), bv=f32(rng, D),
                Wr=f32(rng, 8, 2), Wc=f32(rng, 24, 8), Wo=f32(rng, 8, Nmax))


def abi_weights(w):
    t = {k: dev(v) for k, v in w.items()}
    s = _lib.G2KWeights(*[t[k].data_ptr() for k in ("Wi", "Wii", "Wv", "bv", "Wr", "Wc", "Wo")], None)
    return s, t                     # keep t alive while s is in use


# ---------------------------------------------------------------------------
# g2k_frame_recurrence_f32
# ---------------------------------------------------------------------------
def run_recurrence(lib, A, h0, D, H):
    S, frames = A.shape[:2]
    ar = Arena("cuda")
    h = ar.put(h0, "h")
    At = dev(A) if frames else dev(np.zeros(4, np.float32))
    ok(lib, lib.g2k_frame_recurrence_f32(ctypes.byref(dims(S=S, D=D, H=H)), ptr(At), ptr(h),
                                         frames, None))
    ar.check_guards()
    return host(h)


def recurrence_ref(A, h0):
    out = []
    for s in range(A.shape[0]):
        h = h0[s].astype(np.float64)
        for f in range(A.shape[1]):
            h = ref.recurrence_step(A[s, f].astype(np.float64), h)
        out.append(h)
    return np.stack(out)


@pytest.mark.parametrize("D", [16, 10, 1])
@pytest.mark.parametrize("H", [64, 128, 256, 512])
def test_recurrence_two_chunks(lib, H, D):
    rng = np.random.default_rng(1000 + H + D)
    S, frames = 2, 33
    A = f32(rng, S, frames, D, D, scale=2.0)
    row = min(5, D - 1)
    A[0, 32, row] += 60.0           # the main path's widest column spread
    A[1, 32, row] += 100.0          # prefix sums underflow: the running-max fallback
    h0 = f32(rng, S, D, H)
    got = run_recurrence(lib, A, h0, D, H)
    want = recurrence_ref(A, h0)
    ratio = float(np.max(np.abs(got - want) / (1e-5 * np.abs(want) + 1e-8)))
    print(f"recurrence H={H} D={D} frames=33: worst |dh| / (1e-5 |h| + 1e-8) = {ratio:.3f} (bound 1)")
    assert np.isfinite(got).all()
    assert close_h(got, want)


@pytest.mark.parametrize("D", [16, 10])
@pytest.mark.parametrize("frames", [0, 1])
def test_recurrence_zero_and_one_frame(lib, frames, D):
    rng = np.random.default_rng(50 + D + frames)
    S, H = 2, 128
    A = f32(rng, S, frames, D, D, scale=2.0)
    h0 = f32(rng, S, D, H)
    got = run_recurrence(lib, A, h0, D, H)
    if frames == 0:
        assert np.array_equal(got.view(np.int32), h0.view(np.int32))      # bit-unchanged
    else:
        assert close_h(got, recurrence_ref(A, h0))


# ---------------------------------------------------------------------------
# g2k_mcr_forward_f32
# ---------------------------------------------------------------------------
LAM = 0.1


def run_mcr(lib, w, X, Rel, G, n_active, D, Nmax):
    S = X.shape[0]
    ar = Arena("cuda")
    A, cost, pred = ar.alloc((S, D, D), name="A"), ar.alloc((S, 8, 8), name="cost"), \
        ar.alloc((S, 24, Nmax), name="pred")
    ws, keep = abi_weights(w)
    ins = [dev(X), dev(Rel), dev(G), dev(n_active, np.int32)]
    ok(lib, lib.g2k_mcr_forward_f32(ctypes.byref(dims(S=S, D=D, Nmax=Nmax)), ctypes.byref(ws),
                                    *[ptr(t) for t in ins], ptr(A), ptr(cost), ptr(pred), LAM, None))
    ar.check_guards()
    assert all_written(A) and all_written(cost) and all_written(pred)
    return host(A), host(cost), host(pred)


def check_mcr(w, X, Rel, G, n_active, got):
    A, cost, pred = got
    for s, n in enumerate(n_active):
        o = ref.mcr_forward(*map(f64, (X[s], Rel[s], G[s], w["Wv"], w["bv"], w["Wr"], w["Wc"],
                                       w["Wo"][:, :n])), LAM)
        assert np.abs(A[s] - o["attn"]).max() <= TOL * max(1.0, np.abs(o["attn"]).max())
        assert close(cost[s], o["cost"]) <= TOL
        assert close(pred[s, :, :n], o["pred_path_band"].reshape(24, n)) <= TOL
        assert np.all(pred[s, :, n:].view(np.int32) == 0)                 # exactly +0
    assert np.isfinite(pred).all()


@pytest.mark.parametrize("Nmax", [1, 17, 256])
@pytest.mark.parametrize("D", [16, 10, 1])
def test_mcr_forward_domain(lib, D, Nmax):
    rng = np.random.default_rng(2000 + 17 * D + Nmax)
    S = 3
    w = weights(rng, D, Nmax)
    X, Rel, G = f32(rng, S, D + 2, D), f32(rng, S, 2, D) ** 2, f32(rng, S, D, 8)
    n_active = [1, 0, 1] if Nmax == 1 else [Nmax, 1, 0]
    check_mcr(w, X, Rel, G, n_active, run_mcr(lib, w, X, Rel, G, n_active, D, Nmax))
    if Nmax > 1:                     # Wo's inactive columns are never read
        w2 = dict(w, Wo=w["Wo"].copy())
        w2["Wo"][:, 1:] = NAN
        n2 = [1, 0, 1]
        check_mcr(w2, X, Rel, G, n2, run_mcr(lib, w2, X, Rel, G, n2, D, Nmax))


# ---------------------------------------------------------------------------
# g2k_frame_embed_f32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [0, 1, 2])
@pytest.mark.parametrize("Nmax", [1, 30, 256])
def test_frame_embed_domain(lib, Nmax, stride):
    rng = np.random.default_rng(3000 + 3 * Nmax + stride)
    S, F, D = 3, 3, 16
    W = (F - 1) * stride + 8
    n_active = [Nmax, 0, max(1, Nmax // 2)]
    w = weights(rng, D, Nmax)
    pos, vis = f32(rng, S, W, Nmax, 2), f32(rng, S, 2, Nmax)
    for s, n in enumerate(n_active):
        pos[s, :, n:] = NAN
        vis[s, :, n:] = NAN
    ws, keep = abi_weights(w)
    ins = [dev(pos), dev(vis), dev(n_active, np.int32)]
    d = dims(S=S, F=F, Nmax=Nmax, W=W, stride=stride)
    outs = []
    for with_rel in (True, False):
        ar = Arena("cuda")
        Xt = ar.alloc((S, F, D + 2, D), name="X")
        Rt = ar.alloc((S, 2, D), name="Rel") if with_rel else None
        ok(lib, lib.g2k_frame_embed_f32(ctypes.byref(d), ctypes.byref(ws), *[ptr(t) for t in ins],
                                        ptr(Xt), ptr(Rt), None))
        ar.check_guards()
        assert all_written(Xt) and (Rt is None or all_written(Rt))
        outs.append((host(Xt), None if Rt is None else host(Rt)))
    (X, Relh), (X2, _) = outs
    assert np.array_equal(X, X2)                          # Rel NULL: the same X
    for s, n in enumerate(n_active):
        Wi = w["Wi"][:n].astype(np.float64)
        Ve, R = ref.vislet_embed(vis[s][:, :n].astype(np.float64), Wi)
        assert close(Relh[s], R) <= TOL
        for f in range(F):
            Bv = ref.window_norms(pos[s][f * stride:f * stride + 8, :n].astype(np.float64))
            X0 = ref.input_embed(Bv, Wi, w["Wii"].astype(np.float64))
            assert close(X[s, f], np.concatenate((X0, Ve), axis=0)) <= TOL
        if n == 0:
            assert np.all(X[s] == 0) and np.all(Relh[s] == 0)


# ---------------------------------------------------------------------------
# g2k_ade_fde_f32
# ---------------------------------------------------------------------------
def pairs_metrics(pred, tgt, n, nf, mask):
    """Variant 0's sums for one scene from per-pair ref.validation_errors."""
    m = np.zeros(8)
    for f in range(nf):
        P_ = np.transpose(pred[f].astype(np.float64).reshape(2, 12, -1), (2, 1, 0))
        for i in range(n):
            if mask is not None and not mask[i]:
                continue
            t = tgt[f, i].astype(np.float64)
            ade, fde = ref.validation_errors(P_[i], t)
            m[0] += ade
            m[1] += 1.0
            m[2] += float(np.dot(fde, fde))
            m[3] += float(np.mean(np.linalg.norm(P_[i] - t, axis=1)))
            m[4] += float(np.linalg.norm(fde))
    m[5] = nf
    return m


def error_inputs(rng, S, F, Nmax, n_active, n_frames):
    pred = f32(rng, S, F, 24, Nmax)
    tgt = (np.transpose(pred.reshape(S, F, 2, 12, Nmax), (0, 1, 4, 3, 2))
           + f32(rng, S, F, Nmax, 12, 2, scale=0.5)).astype(np.float32)
    for s in range(S):
        pred[s, :, :, n_active[s]:] = NAN
        tgt[s, :, n_active[s]:] = NAN
        if n_frames is not None:
            pred[s, n_frames[s]:] = NAN
            tgt[s, n_frames[s]:] = NAN
    return pred, tgt


def scene_sizes(Nmax):
    return [Nmax, 0, max(1, Nmax // 2), min(Nmax, 17)]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("framed", [False, True])
@pytest.mark.parametrize("Nmax,F", [(1, 3), (30, 5), (256, 2)])
def test_ade_fde_variant0_domain(lib, Nmax, F, framed, masked):
    rng = np.random.default_rng(4000 + Nmax + F + 2 * framed + masked)
    S = 4
    n_active = scene_sizes(Nmax)
    n_frames = [F, 1, F, 0] if framed else None
    mask = None
    if masked:
        mask = (rng.random((S, Nmax)) > 0.3).astype(np.uint8)
        mask[2] = 0                                        # an active scene, every pedestrian masked
        mask[0, 0] = 1
    pred, tgt = error_inputs(rng, S, F, Nmax, n_active, n_frames)
    ar = Arena("cuda")
    out = ar.alloc((S, 8), name="out")
    ins = [dev(pred), dev(tgt), dev(n_active, np.int32),
           None if n_frames is None else dev(n_frames, np.int32), None if mask is None else dev(mask)]
    ok(lib, lib.g2k_ade_fde_f32(ctypes.byref(dims(S=S, F=F, Nmax=Nmax)), *[ptr(t) for t in ins], 0,
                                ptr(out), None))
    ar.check_guards()
    assert all_written(out)
    got = host(out)
    for s in range(S):
        nf = F if n_frames is None else n_frames[s]
        m = pairs_metrics(pred[s], tgt[s], n_active[s], nf, None if mask is None else mask[s])
        assert close(got[s, :5], m[:5]) <= TOL, s
        assert got[s, 1] == m[1] and got[s, 5] == nf
        assert np.all(got[s, 6:8].view(np.int32) == 0)


@pytest.mark.parametrize("Nmax", [1, 65, 256])
def test_ade_fde_variant1_domain(lib, Nmax):
    rng = np.random.default_rng(4100 + Nmax)
    n_active = [Nmax, 0, max(1, Nmax // 2)]
    S = len(n_active)
    pred, tgt = error_inputs(rng, S, 1, Nmax, n_active, None)
    ar = Arena("cuda")
    out = ar.alloc((S, 8), name="out")
    ins = [dev(pred), dev(tgt), dev(n_active, np.int32)]
    ok(lib, lib.g2k_ade_fde_f32(ctypes.byref(dims(S=S, F=1, Nmax=Nmax)), *[ptr(t) for t in ins], None,
                                None, 1, ptr(out), None))
    ar.check_guards()
    assert all_written(out)
    got = host(out)
    for s, n in enumerate(n_active):
        assert np.all(got[s, 3:].view(np.int32) == 0)
        if n == 0:                   # the reference raises here; the header says {0, 0, 0}
            assert np.all(got[s, :3].view(np.int32) == 0)
            continue
        p = np.transpose(pred[s, 0, :, :n].reshape(2, 12, n), (2, 1, 0))
        ade, fde, counter = ref.get_mean_error(p, tgt[s, 0, :n], 8, n)
        assert close(got[s, 0], ade) <= TOL and close(got[s, 1], fde) <= TOL
        assert int(got[s, 2]) == counter


# ---------------------------------------------------------------------------
# nri_learned relation ops
# ---------------------------------------------------------------------------
def special_rows(cols):
    x = np.empty((3, cols), np.float32)
    x[0] = np.where(np.arange(cols) % 2 == 0, 100.0, -100.0)
    x[1] = 7.5
    x[2] = -100.0
    x[2, cols // 2] = 100.0
    return x


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 63), (3, 64), (2, 65), (1, 200), (5, 16)])
def test_nri_ops_domain(lib, rows, cols):
    rng = np.random.default_rng(5000 + 7 * rows + cols)
    for adj in (f32(rng, rows, cols, scale=4.0), special_rows(cols)):
        ar = Arena("cuda")
        sg, sm = ar.alloc(adj.shape, name="sigmoid"), ar.alloc(adj.shape, name="softmax")
        a = dev(adj)
        ok(lib, lib.g2k_infer_rlns_f32(ptr(a), ptr(sg), adj.shape[0], cols, None))
        ok(lib, lib.g2k_eval_rln_ngh_f32(ptr(a), ptr(sm), adj.shape[0], cols, None))
        ar.check_guards()
        assert all_written(sg) and all_written(sm)
        sg, sm = host(sg), host(sm)
        assert np.isfinite(sg).all() and np.isfinite(sm).all()
        assert close(sg, ref.infer_rlns(adj)) <= TOL
        assert close(sm, ref.eval_rln_ngh(adj)) <= TOL
        assert np.abs(sm.astype(np.float64).sum(axis=-1) - 1.0).max() <= 1e-6


# ---------------------------------------------------------------------------
# g2k_gridlstm_f32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("u,fs,K,R,alias", [(2, 4, 4, 255, False), (2, 4, 4, 256, False),
                                            (2, 4, 4, 257, False), (2, 4, 1, 5, False),
                                            (4, 8, 1, 3, True), (2, 4, 4, 257, True)])
def test_gridlstm_domain(lib, u, fs, K, R, alias):
    rng = np.random.default_rng(6000 + 100 * u + 10 * K + R + alias)
    wd = 2 * u * K
    ld = wd if alias else wd + 3
    x, st = f32(rng, R, K * fs), f32(rng, R, ld)
    W, b, P = f32(rng, fs + 2 * u, 3 * u, scale=0.7), f32(rng, 3 * u, scale=0.3), f32(rng, 4, u)
    ar = Arena("cuda")
    out = ar.alloc((R, wd), name="out")
    state = ar.put(st, "state") if alias else dev(st)
    state_out = state if alias else ar.alloc((R, wd), name="state_out")
    ins = [dev(x), dev(W), dev(b), dev(P)]
    ok(lib, lib.g2k_gridlstm_f32(ptr(ins[0]), K * fs, ptr(state), ld, ptr(ins[1]), ptr(ins[2]),
                                 ptr(ins[3]), ptr(out), ptr(state_out), R, K, fs, u, None))
    ar.check_guards()
    assert all_written(out) and all_written(state_out)
    ro, rs = ref.gridlstm_cell(x, st, W, b, tuple(P), feature_size=fs, num_units=u)
    assert close(host(out), ro) <= TOL
    assert close(host(state_out), rs) <= TOL


# ---------------------------------------------------------------------------
# g2k_context_conv_f32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C,D,extra", [(c, d, 1) for c in (2, 4) for d in (1, 7, 16)] + [(2, 7, 0)])
def test_context_conv_domain(lib, C, D, extra):
    rng = np.random.default_rng(7000 + 20 * C + D + extra)
    Hh = Ww = D + extra
    img = rng.uniform(0, 255, size=(Hh, Ww, C)).astype(np.float32)
    filt = f32(rng, Hh + 3 - D, Ww + 2 - D, C)
    rc = ref.context_conv(img, filt, D, 5e-4)
    rG = ref.context_input(rc, ref.static_mask(D, 8))
    nws = int(lib.g2k_context_conv_workspace_bytes(Hh, Ww, D))
    assert nws == (Hh + 3 - D) * D * D * 4
    ins = [dev(img), dev(filt)]
    for want_out, want_G in ((True, True), (True, False), (False, True)):
        ar = Arena("cuda")
        out = ar.alloc((D, D), name="out") if want_out else None
        G = ar.alloc((D, 8), name="G") if want_G else None
        ws = ar.alloc((nws // 4,), name="workspace")
        ok(lib, lib.g2k_context_conv_f32(ptr(ins[0]), Hh, Ww, C, ptr(ins[1]), D, 5e-4, ptr(out), ptr(G),
                                         ptr(ws), nws, None))
        ar.check_guards()
        assert all_written(ws)
        if want_out:
            assert all_written(out)
            assert np.abs(host(out) - rc).max() <= 1e-4 * np.abs(rc).max()
        if want_G:
            assert all_written(G)
            assert np.abs(host(G) - rG).max() <= 1e-4 * np.abs(rG).max()


# ---------------------------------------------------------------------------
# g2k_nll_f32 / g2k_gauss_sample_f32
# ---------------------------------------------------------------------------
def draw_head(rng, edge=True):
    head = np.stack([0.3 * rng.standard_normal(12), 0.3 * rng.standard_normal(12),
                     rng.uniform(-3.0, 3.0, 12)]).astype(np.float32)
    if edge:
        head[2, 0], head[2, 1] = 3.0, -3.0
    return head


def run_nll(lib, pred, tgt, n_active, n_frames, mask, head, want_dpred=True):
    S, F, _, Nmax = pred.shape
    ar = Arena("cuda")
    out = ar.alloc((38,), name="out")
    dpred = ar.alloc(pred.shape, name="dpred") if want_dpred else None
    d = dims(S=S, F=F, Nmax=Nmax)
    nws = int(lib.g2k_nll_workspace_bytes(ctypes.byref(d)))
    assert nws == S * 38 * 4
    ws = ar.alloc((S, 38), name="workspace")
    ins = [dev(pred), dev(tgt), dev(n_active, np.int32),
           None if n_frames is None else dev(n_frames, np.int32), None if mask is None else dev(mask),
           dev(head)]
    ok(lib, lib.g2k_nll_f32(ctypes.byref(d), *[ptr(t) for t in ins], ptr(out), ptr(dpred), ptr(ws),
                            nws, None))
    ar.check_guards()
    assert all_written(out) and all_written(ws)
    return host(out), dpred


def check_dpred_footprint(dpred, R_dp, n_active, n_frames, mask):
    """Active columns of frames < n_frames are written, masked ones exactly 0;
    everything else still holds the pattern (include/g2k_hip.h)."""
    S, F, _, Nmax = dpred.shape
    keep = host(untouched(dpred))
    got = host(dpred)
    worst = 0.0
    for s in range(S):
        n, nf = n_active[s], F if n_frames is None else n_frames[s]
        assert keep[s, nf:].all() and keep[s, :nf, :, n:].all(), s
        assert not keep[s, :nf, :, :n].any(), s
        on = np.ones(n, bool) if mask is None else mask[s, :n].astype(bool)
        assert np.all(got[s, :nf][:, :, :n][:, :, ~on].view(np.int32) == 0), s
        if nf and on.any():
            worst = max(worst, close(got[s, :nf][:, :, :n][:, :, on], R_dp[s][:nf][:, :, :n][:, :, on]))
    return worst


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("framed", [False, True])
@pytest.mark.parametrize("Nmax", [1, 7, 256])
def test_nll_domain(lib, Nmax, framed, masked):
    rng = np.random.default_rng(8000 + Nmax + 2 * framed + masked)
    S, F = 4, 3
    n_active = [Nmax, 0, max(1, Nmax // 2), min(Nmax, 5)]
    n_frames = [3, 0, 2, 1] if framed else None
    mask = None
    if masked:
        mask = (rng.random((S, Nmax)) > 0.3).astype(np.uint8)
        mask[0] = 0
        mask[3, 0] = 1
    pred, tgt = error_inputs(rng, S, F, Nmax, n_active, n_frames)
    head = draw_head(rng)
    out, dpred = run_nll(lib, pred, tgt, n_active, n_frames, mask, head)
    out2, _ = run_nll(lib, pred, tgt, n_active, n_frames, mask, head, want_dpred=False)
    assert np.array_equal(out.view(np.int32), out2.view(np.int32))        # dpred NULL: same sums
    R_nll, R_pairs, R_dh, R_dp = 0.0, 0, np.zeros((3, 12)), []
    for s in range(S):
        nf = F if n_frames is None else n_frames[s]
        l_, p_, h_, d_ = ref.bivariate_nll(pred[s], tgt[s], head, n_active[s], nf,
                                           None if mask is None else mask[s].astype(bool))
        R_nll += l_
        R_pairs += p_
        R_dh += h_
        R_dp.append(d_)
    assert R_pairs > 0 and np.isfinite(out).all()
    e_nll = abs(float(out[36]) - R_nll) / abs(R_nll)
    e_dh = np.abs(out[:36].reshape(3, 12) - R_dh).max() / np.abs(R_dh).max()
    e_dp = check_dpred_footprint(dpred, R_dp, n_active, n_frames, mask)
    print(f"nll Nmax={Nmax} framed={framed} masked={masked}: nll {e_nll:.2e} dhead {e_dh:.2e} "
          f"dpred {e_dp:.2e} (bound 1e-4)")
    assert int(out[37]) == R_pairs
    assert e_nll <= TOL and e_dh <= TOL and e_dp <= TOL


def test_nll_rows_past_one_trip(lib):
    """tests/eval_cells.py "nll-rows257": S 257 scenes leave 257 rows [38], so
    g2k_grad_rows_kernel takes a second trip of its r0 loop with one real row
    and clamped loads past it (S 257 is the smallest that does; F 1 and Nmax 3
    keep the oracle quick).  n_active 0..3, a mask, the head of test_nll_domain.
    MEASURED on an MI355X, error / bound (1e-4): nll 0.037, head gradient 0.058
    (normwise), dpred 0.096; 281 pairs, the count exact."""
    c = ec.NLL
    S, F, Nmax = c.S, c.F, c.Nmax
    rng = np.random.default_rng(8200)
    n_active = [int(v) for v in rng.integers(0, Nmax + 1, S)]
    n_active[0], n_active[S - 1] = Nmax, Nmax            # the last row (the second trip's) counts
    mask = (rng.random((S, Nmax)) > 0.3).astype(np.uint8)
    mask[S - 1] = 1
    pred, tgt = error_inputs(rng, S, F, Nmax, n_active, None)
    head = draw_head(rng)
    out, dpred = run_nll(lib, pred, tgt, n_active, None, mask, head)
    R_nll, R_pairs, R_dh, R_dp = 0.0, 0, np.zeros((3, 12)), []
    last = None
    for s in range(S):
        l_, p_, h_, d_ = ref.bivariate_nll(pred[s], tgt[s], head, n_active[s], F, mask[s].astype(bool))
        R_nll += l_
        R_pairs += p_
        R_dh += h_
        R_dp.append(d_)
        last = (l_, p_)
    assert last[1] == Nmax and abs(last[0]) > 1e-3 * abs(R_nll) / S      # dropping row 256 would show
    e_nll = abs(float(out[36]) - R_nll) / abs(R_nll)
    e_dh = np.abs(out[:36].reshape(3, 12) - R_dh).max() / np.abs(R_dh).max()
    e_dp = check_dpred_footprint(dpred, R_dp, n_active, None, mask)
    print(f"nll-rows257: worst error / bound: nll {e_nll / TOL:.2g} dhead {e_dh / TOL:.2g} "
          f"dpred {e_dp / TOL:.2g}; {R_pairs} pairs")
    assert int(out[37]) == R_pairs                        # exact: one pair short shows a lost row
    assert e_nll <= TOL and e_dh <= TOL and e_dp <= TOL


def test_nll_without_any_pair(lib):
    """n_active 0, n_frames 0 and an all-masked scene: nll 0, count 0,
    gradients 0, nothing NaN; the all-masked scene's active columns get
    exact zeros in dpred, nothing else is written."""
    rng = np.random.default_rng(8100)
    S, F, Nmax = 3, 2, 7
    n_active, n_frames = [0, 4, 5], [2, 0, 2]
    mask = np.ones((S, Nmax), np.uint8)
    mask[2] = 0
    pred, tgt = error_inputs(rng, S, F, Nmax, n_active, n_frames)
    out, dpred = run_nll(lib, pred, tgt, n_active, n_frames, mask, draw_head(rng))
    assert np.all(out.view(np.int32) == 0)
    check_dpred_footprint(dpred, None, n_active, n_frames, mask)


@pytest.mark.parametrize("seed", [0, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1])
@pytest.mark.parametrize("S,F,Nmax", [(1, 1, 1), (2, 3, 7), (1, 2, 256)])
def test_gauss_sample_domain(lib, S, F, Nmax, seed):
    rng = np.random.default_rng(8200 + S + F + Nmax)
    pred = f32(rng, S, F, 24, Nmax)
    head = draw_head(rng, edge=False)
    head[2] = rng.standard_normal(12)
    ar = Arena("cuda")
    out = ar.alloc(pred.shape, name="out")
    ins = [dev(pred), dev(head)]
    ok(lib, lib.g2k_gauss_sample_f32(ctypes.byref(dims(S=S, F=F, Nmax=Nmax)), ptr(ins[0]), ptr(ins[1]),
                                     ctypes.c_uint64(seed), ptr(out), None))
    ar.check_guards()
    assert all_written(out)
    assert close(host(out), ref.gauss_sample(pred, head, seed)) <= TOL


# ---------------------------------------------------------------------------
# g2k_update_f32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rms,clip", [(False, 0.0), (True, 10.0), (True, 0.5), (False, 0.5)])
@pytest.mark.parametrize("count", [0, 7])
@pytest.mark.parametrize("P", [520, 1264, 6676, 7169, 8192, 8193, 20000])
def test_update_domain(lib, P, count, rms, clip):
    rng = np.random.default_rng(9000 + P + count)
    p = f32(rng, P)
    g = f32(rng, P + 2, scale=5.0)
    g[P + 1] = count
    ms0 = np.abs(f32(rng, P))
    ar = Arena("cuda")
    flat = ar.put(p, "params")
    ms = ar.put(ms0, "ms") if rms else None
    grad = dev(g)
    ok(lib, lib.g2k_update_f32(ptr(flat), ptr(ms), ptr(grad), P, 5e-3, 0.95, clip, None))
    ar.check_guards()
    assert np.array_equal(host(grad).view(np.int32), g.view(np.int32))    # grad is read only
    rp, rm = ref.optimizer_update(p, ms0 if rms else None, g[:P], g[P + 1], 5e-3, 0.95, clip)
    assert np.abs(host(flat) - rp).max() <= 1e-6 * max(1.0, np.abs(rp).max())
    if rms:
        assert np.abs(host(ms) - rm).max() <= 1e-5 * np.abs(rm).max()


@pytest.mark.parametrize("clip", [0.0, 10.0])
def test_update_zero_gradient_zero_ms(lib, clip):
    rng = np.random.default_rng(9100)
    for P in (1264, 7169, 8192, 8193, 20000):
        p = f32(rng, P)
        ar = Arena("cuda")
        flat, ms = ar.put(p, "params"), ar.put(np.zeros(P, np.float32), "ms")
        grad = dev(np.zeros(P + 2, np.float32))
        ok(lib, lib.g2k_update_f32(ptr(flat), ptr(ms), ptr(grad), P, 5e-3, 0.95, clip, None))
        ar.check_guards()
        assert np.array_equal(host(flat).view(np.int32), p.view(np.int32)), P    # bit-unchanged, finite
        assert np.all(host(ms) == 0), P


# ---------------------------------------------------------------------------
# g2k_scene_gather_f32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_off", [True, False])
@pytest.mark.parametrize("with_vis", [True, False])
def test_scene_gather_hand_made_plan(lib, with_vis, with_off):
    rng = np.random.default_rng(9200)
    cols, S, F, Nmax = 40, 2, 2, 5
    n_active = [3, 5]
    xy, vis = f32(rng, cols, 2), f32(rng, 2, cols)
    pos_col = rng.integers(0, cols, size=(S, 8, Nmax)).astype(np.int32)
    pos_col[0, 0, 1] = pos_col[0, 7, 2] = pos_col[1, 3, 4] = -1           # zero slots
    tgt_col = rng.integers(0, cols, size=(S, Nmax, 12)).astype(np.int32)
    tgt_col[1, 2, 11] = -1                                                # a short target list
    vis_off = np.array([4, 33], np.int32)
    ar = Arena("cuda")
    pos, vislet = ar.alloc((S, 8, Nmax, 2), name="pos"), ar.alloc((S, 2, Nmax), name="vislet")
    targets, pm = ar.alloc((S, F, Nmax, 12, 2), name="targets"), ar.alloc((S, Nmax), U8, name="ped_mask")
    ins = [dev(xy), dev(vis) if with_vis else None, dev(pos_col), dev(tgt_col),
           dev(vis_off) if with_off else None, dev(n_active, np.int32)]
    ok(lib, lib.g2k_scene_gather_f32(ptr(ins[0]), ptr(ins[1]), cols, ptr(ins[2]), ptr(ins[3]),
                                     ptr(ins[4]), ptr(ins[5]), S, F, Nmax, ptr(pos), ptr(vislet),
                                     ptr(targets), ptr(pm), None))
    ar.check_guards()
    for t in (pos, vislet, targets, pm):
        assert all_written(t)
    col = lambda c: xy[c] if c >= 0 else np.zeros(2, np.float32)          # noqa: E731
    e_pos, e_vis = np.zeros((S, 8, Nmax, 2), np.float32), np.zeros((S, 2, Nmax), np.float32)
    e_tgt, e_pm = np.zeros((S, F, Nmax, 12, 2), np.float32), np.zeros((S, Nmax), np.uint8)
    for s, n in enumerate(n_active):
        off = int(vis_off[s]) if with_off else 0
        for j in range(n):
            for t in range(8):
                e_pos[s, t, j] = col(pos_col[s, t, j])
            if with_vis:
                e_vis[s, :, j] = vis[:, off + j]
            for l in range(12):
                e_tgt[s, :, j, l] = col(tgt_col[s, j, l])
            e_pm[s, j] = int((tgt_col[s, j] >= 0).all())
    assert e_pm[1, 2] == 0 and e_pm.sum() == 3 + 4
    for got, want in ((pos, e_pos), (vislet, e_vis), (targets, e_tgt), (pm, e_pm)):
        assert np.array_equal(host(got), want)                            # a gather: exact


# ---------------------------------------------------------------------------
# g2k_encoder_chain_f32
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("peep", [True, False])
def test_encoder_chain_footprint(lib, peep):
    rng = np.random.default_rng(9300 + peep)
    S, F, H, u, fs_, D, Nmax = 2, 3, 64, 2, 4, 16, 7
    n_active, n_frames = [5, 7], [2, 0]
    w = weights(rng, D, Nmax)
    X, Rel, G = f32(rng, S, F, D + 2, D, scale=0.5), f32(rng, S, 2, D) ** 2, f32(rng, S, D, 8)
    cW, cb, cP = f32(rng, fs_ + 2 * u, 3 * u, scale=0.7), f32(rng, 3 * u, scale=0.3), f32(rng, 4, u)
    h0 = f32(rng, D, H)
    ar = Arena("cuda")
    Xe, cs = ar.alloc((S, F, D + 2, D), name="Xe"), ar.alloc((D, D), name="cell_state")
    attn, cost = ar.alloc((S, F, D, D), name="attn"), ar.alloc((S, F, 8, 8), name="cost")
    pred, h = ar.alloc((S, F, 24, Nmax), name="pred"), ar.put(h0, "h")
    ws, keep = abi_weights(w)
    ins = [dev(X), dev(Rel), dev(G), dev(n_active, np.int32), dev(n_frames, np.int32), dev(cW),
           dev(cb), dev(cP) if peep else None]
    ok(lib, lib.g2k_encoder_chain_f32(ctypes.byref(dims(S=S, F=F, H=H, Nmax=Nmax)), ctypes.byref(ws),
                                      *[ptr(t) for t in ins], fs_, u, ptr(Xe), ptr(cs), ptr(attn),
                                      ptr(cost), ptr(pred), ptr(h), LAM, None))
    ar.check_guards()
    assert all_written(Xe) and all_written(cs) and all_written(h)
    Xe_h, run = host(Xe), np.zeros((S, F), bool)
    for s in range(S):
        run[s, :n_frames[s]] = True
    # Xe is X outside rows 0..D-1 of the frames that ran
    assert np.array_equal(Xe_h[~run], X[~run]) and np.array_equal(Xe_h[:, :, D:], X[:, :, D:])
    for t in (attn, cost, pred):
        keep_t = host(untouched(t)).reshape(S, F, -1)
        assert keep_t[~run].all() and not keep_t[run].any()
    hh = h0.astype(np.float64)
    for s in range(S):
        n = n_active[s]
        for f in range(n_frames[s]):
            x0 = ref.gridlstm_cell(X[s, f, :D], hh, cW, cb, tuple(cP) if peep else None,
                                   feature_size=fs_, num_units=u)[0]
            assert close(Xe_h[s, f, :D], x0) <= TOL
            o = ref.mcr_forward(*map(f64, (np.concatenate((x0, X[s, f, D:])), Rel[s], G[s], w["Wv"],
                                           w["bv"], w["Wr"], w["Wc"], w["Wo"][:, :n])), LAM)
            A = host(attn[s, f])
            assert np.abs(A - o["attn"]).max() <= TOL * max(1.0, np.abs(o["attn"]).max())
            assert close(host(cost[s, f]), o["cost"]) <= TOL
            p = host(pred[s, f])
            assert close(p[:, :n], o["pred_path_band"].reshape(24, n)) <= TOL
            assert np.all(p[:, n:] == 0)
            hh = ref.recurrence_step(o["attn"], hh)
    assert close_h(host(h), hh)


# ---------------------------------------------------------------------------
# the fused step's and the train step's write footprints
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused_case():
    """Inputs and the oracle's outputs, computed once for the eight cases."""
    rng = np.random.default_rng(9400)
    S, F, H, Nmax, D = 4, 5, 64, 30, 16
    n_active, n_frames = [1, 16, 17, 30], [5, 0, 3, 5]
    w = weights(rng, D, Nmax)
    W = F - 1 + 8
    pos, vis = f32(rng, S, W, Nmax, 2), f32(rng, S, 2, Nmax)
    tgt = f32(rng, S, F, Nmax, 12, 2, scale=0.3)
    for s, n in enumerate(n_active):                      # the real-data path zero-fills
        pos[s, :, n:] = 0
        vis[s, :, n:] = 0
        tgt[s, :, n:] = 0
    G, h0 = f32(rng, S, D, 8), f32(rng, S, D, H)
    want = [ref.scene_step(pos[s], vis[s], G[s], w, tgt[s], n_active[s], h0[s], n_frames=n_frames[s],
                           stride=1, keep=True) for s in range(S)]
    return dict(S=S, F=F, H=H, Nmax=Nmax, W=W, n_active=n_active, n_frames=n_frames, w=w, pos=pos,
                vis=vis, tgt=tgt, G=G, h0=h0, want=want)


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("layout", ["band", "ped"])
@pytest.mark.parametrize("entry", ["step", "train"])
def test_fused_step_write_footprint(lib, fused_case, entry, layout, split):
    c = fused_case
    S, F, H, Nmax, D = c["S"], c["F"], c["H"], c["Nmax"], 16
    flags = (_lib.STEP_PRED_PED_MAJOR if layout == "ped" else 0) | (split << _lib.STEP_SPLIT_SHIFT)
    d = dims(S=S, F=F, H=H, Nmax=Nmax, W=c["W"], stride=1, flags=flags)
    ar = Arena("cuda")
    pred = ar.alloc((S, F, 24, Nmax) if layout == "band" else (S, F, Nmax, 12, 2), name="pred")
    h_out, metrics = ar.alloc((S, D, H), name="h_out"), ar.alloc((S, 8), name="metrics")
    ws, keep = abi_weights(c["w"])
    ins = [dev(c["pos"]), dev(c["vis"]), dev(c["G"]), dev(c["tgt"]), dev(c["n_active"], np.int32),
           dev(c["n_frames"], np.int32), None, dev(c["h0"])]
    if entry == "step":
        A, cost = ar.alloc((S, F, D, D), name="A_out"), ar.alloc((S, F, 8, 8), name="cost_out")
        nws = int(lib.g2k_step_workspace_bytes(ctypes.byref(d)))
        assert (nws == 0) == (split == 1)
        wsp = ar.alloc((max(nws, 4),), U8, name="workspace")
        ok(lib, lib.g2k_step_fused_f32(ctypes.byref(d), ctypes.byref(ws), *[ptr(t) for t in ins],
                                       ptr(h_out), ptr(pred), ptr(metrics), ptr(A), ptr(cost), 5e-4,
                                       ptr(wsp), nws, None))
    else:
        P = int(lib.g2k_grad_size(ctypes.byref(d)))
        assert P == 24 * Nmax + 496
        grad = ar.alloc((P + 2,), name="grad")
        nws = int(lib.g2k_train_workspace_bytes(ctypes.byref(d)))
        wsp = ar.alloc((nws,), U8, name="workspace")
        ok(lib, lib.g2k_train_step_f32(ctypes.byref(d), ctypes.byref(ws), *[ptr(t) for t in ins],
                                       ptr(h_out), ptr(pred), ptr(metrics), 5e-4, ptr(grad), ptr(wsp),
                                       nws, None, None, 5e-3, 0.95, 10.0, None))
    ar.check_guards()
    assert all_written(metrics) and all_written(h_out)
    if entry == "train":
        assert all_written(grad) and np.isfinite(host(grad)).all()
    keep_p, got_p = host(untouched(pred)), host(pred)
    hh, met = host(h_out), host(metrics)
    for s in range(S):
        n, nf = c["n_active"][s], c["n_frames"][s]
        pr, h, m, ex = c["want"][s]
        assert keep_p[s, nf:].all(), s
        if layout == "band":
            lim = min(Nmax, 16 * ((n + 15) // 16))
            assert not keep_p[s, :nf, :, :lim].any() and keep_p[s, :nf, :, lim:].all(), s
            assert np.all(got_p[s, :nf, :, n:lim].view(np.int32) == 0), s
            band = got_p[s, :nf, :, :n]
        else:
            assert not keep_p[s, :nf, :n].any() and keep_p[s, :nf, n:].all(), s
            band = np.transpose(got_p[s, :nf, :n], (0, 3, 2, 1)).reshape(nf, 24, n)
        assert np.isfinite(band).all()
        if nf:
            assert close(band.reshape(nf, 2, 12, n), pr) <= TOL, s
        else:
            assert np.array_equal(hh[s].view(np.int32), c["h0"][s].view(np.int32))   # h_out == h_in
        assert close_h(hh[s], h), s
        assert close(met[s, :6], m[:6]) <= TOL, s
        assert np.all(met[s, 6:] == 0)
        if entry == "step":
            for t, want, k in ((A, ex["A"], "A"), (cost, ex["cost"], "cost")):
                keep_t = host(untouched(t))[s]
                assert keep_t[nf:].all() and not keep_t[:nf].any(), (s, k)
                if nf:
                    r = np.stack(want)
                    assert np.abs(host(t)[s, :nf] - r).max() <= TOL * max(1.0, np.abs(r).max()), (s, k)
