"""GPU: the full-covariance trajectory head (csrc/g2k_fullcov.hip;
fullcov.FullCovHead; evaluate.py --fullcov_head) against the float64 checker
tests/fullcov_ref.py.  PARITY UNPINNED: the reference has no probabilistic
head.  Tolerance: the project's rule close(got, ref) <= 1e-4 unless stated.

Best-of-K and sampler: the six shapes of tests/test_best_of_k_gpu.py (the
draws of a pair on 1, 2, 4 and 16 lanes, K not a multiple of the lanes, one
and several frame chunks per scene, more pairs than threads, shared targets,
NULL mask / n_frames, a seed that wraps) with a dense random factor whose
upper triangle holds NaN.

Stats and fit: the stats kernel deals the S F Nmax slots to workgroups of at
least 512 slots (fullcov_geom), so "one" (240 slots), "n256" (512) and
"shared" (495) are one workgroup that writes the outputs itself, and "rows"
(1240 slots: three workgroups, 414 slots each, a range that ends inside a
scene-frame) goes through the rows kernel; "rank" has 11 pairs (a
rank-deficient M), "none" has no pair.  The kernel works in double on exact
f32 differences, so only the summation order (and L^-1 r by a product with
the inverse, not a solve) differs from the checker: moments and stats within
1e-12 max(1, |ref|), the counts equal (no q of these inputs lies within 1e-9
of a radius, asserted).  Every non-pair of pred and targets holds NaN: finite
outputs prove they were never read.  Measured on an MI355X: best-of-K per_ped
within 1.5e-6 and sums within 3.7e-7 of the checker, the sampler within
3.6e-6, every index attains the checker's minimum exactly; moments within
6.6e-15 and stats within 7.7e-16 of max(1, |ref|), every count equal; the fit
within 5.5e-8 of the checker's factor, |fit fit^T - C| <= 8.2e-8 max|C|, and
sum q / 24 n at the device-written fit 1 - 5e-6 (the ridge and the f32
factor)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib
from tests import fullcov_ref as fr
from tests.abi_arena import Arena, all_written
from tests.bestk_ref import MASK64, pair_mask
from tests.conftest import close

pytestmark = pytest.mark.gpu
TOL = 1e-4
SEED = (7 << 32) + 99
LEVELS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99)
NL = len(LEVELS)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _head(fc_chol, dev):
    from multimodaltraj_2_amd.fullcov import FullCovHead
    fc = FullCovHead(device=dev)
    fc.chol = fc_chol if isinstance(fc_chol, torch.Tensor) else _t(fc_chol, dev)
    return fc


# ---------------------------------------------------------------------------
# best-of-K and the sampler
# ---------------------------------------------------------------------------
#           S  F   Nmax K   sigma n_active              n_frames          mask   shared seed
BK_CASES = [(5, 3, 20, 20, 0.05, [0, 1, 13, 20, 7], [3, 0, 2, 3, 1], True, False, SEED),
            (2, 2, 256, 3, 1.0, [256, 37], None, False, False, SEED),
            (3, 4, 17, 1, 0.3, [17, 1, 0], [4, 2, 4], True, False, SEED),
            (2, 40, 32, 7, 0.3, [32, 21], [40, 33], True, False, SEED),
            (3, 4, 20, 20, 0.05, [20, 0, 13], [4, 4, 0], True, True, SEED),
            (2, 2, 9, 5, 0.3, [9, 4], [2, 1], True, False, (1 << 64) - 2)]
BK_IDS = ["s5f3n20k20", "n256", "k1", "f40k7", "shared", "wrap"]


def _dense_factor(rng, sigma):
    """Diagonal in [0.5, 1.5] sigma, off-diagonals of the same scale, NaN above."""
    Lm = sigma * rng.uniform(-1.0, 1.0, (24, 24))
    Lm[np.arange(24), np.arange(24)] = sigma * rng.uniform(0.5, 1.5, 24)
    Lm[np.triu_indices(24, 1)] = np.nan
    return Lm.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _bk_inputs(i):
    S, F, N, K, sigma, nact, nfr, masked, shared, seed = BK_CASES[i]
    rng = np.random.default_rng(500 + i)
    pred = rng.standard_normal((S, F, 24, N)).astype(np.float32)
    Ft = 1 if shared else F
    base = pred[:, :Ft].reshape(S, Ft, 2, 12, N).transpose(0, 1, 4, 3, 2)
    tg = (base + 3 * sigma * rng.standard_normal((S, Ft, N, 12, 2))).astype(np.float32)
    pm = (rng.random((S, N)) > 0.2).astype(np.uint8) if masked else None
    return dict(pred=pred, targets=np.ascontiguousarray(tg), chol=_dense_factor(rng, sigma),
                n_active=np.array(nact, np.int32),
                n_frames=None if nfr is None else np.array(nfr, np.int32), ped_mask=pm,
                K=K, seed=seed, shared=shared)


@functools.lru_cache(maxsize=None)
def _bk_reference(i):
    c = _bk_inputs(i)
    return fr.best_of_k_ref(c["pred"], c["targets"], c["n_active"], c["chol"], c["seed"], c["K"],
                            c["n_frames"], c["ped_mask"])


def _bk_run(i, dev):
    c = _bk_inputs(i)
    fc = _head(c["chol"], dev)
    pred = _t(c["pred"], dev)
    r = fc.best_of_k(pred, _t(c["targets"], dev), _t(c["n_active"], dev), c["K"], seed=c["seed"],
                     n_frames=_t(c["n_frames"], dev), ped_mask=_t(c["ped_mask"], dev),
                     targets_shared=c["shared"], want_best=True)
    torch.cuda.synchronize()
    return fc, pred, r


_BK = {}


def _bk_result(i, dev):
    if i not in _BK:
        _BK[i] = _bk_run(i, dev)
    return _BK[i]


@pytest.mark.parametrize("i", range(len(BK_CASES)), ids=BK_IDS)
def test_best_of_k_values_match_checker(gpu, i):
    _, pred, r = _bk_result(i, gpu)
    R = _bk_reference(i)
    per, out = r.per_ped.cpu().numpy(), r.sums.cpu().numpy()
    m = R["pairs"]
    print(f"case {BK_IDS[i]}: pairs {int(m.sum())}, per_ped err {close(per[..., :2], R['per_ped'][..., :2]):.3g}, "
          f"sums err {close(out[:, :5], R['out'][:, :5]):.3g}")
    assert np.all(np.isfinite(per)) and np.all(np.isfinite(out))       # NaN above the diagonal: not read
    assert close(per[..., :2], R["per_ped"][..., :2]) <= TOL
    assert close(out[:, :5], R["out"][:, :5]) <= TOL
    np.testing.assert_array_equal(out[:, 2], R["out"][:, 2])
    np.testing.assert_array_equal(out[:, 5], R["out"][:, 5])
    assert np.all(out[:, 6:] == 0)
    assert np.all(per[~m] == 0)                           # non-pairs: exactly zero, all four
    off = ~torch.from_numpy(m).to(gpu)[:, :, None, :].expand_as(pred)
    assert torch.equal(r.best[off], pred[off])            # ... and pred in best


@pytest.mark.parametrize("i", range(len(BK_CASES)), ids=BK_IDS)
def test_best_of_k_indices_attain_the_minimum(gpu, i):
    _, _, r = _bk_result(i, gpu)
    R = _bk_reference(i)
    K = BK_CASES[i][3]
    per = r.per_ped.cpu().numpy().astype(np.float64)
    m = R["pairs"]
    for col, errs in ((2, R["ade_k"]), (3, R["fde_k"])):
        k = per[..., col][m]
        assert np.all(k == np.round(k)) and np.all((k >= 0) & (k < K))
        at = np.take_along_axis(errs, per[..., col].astype(np.int64)[None], axis=0)[0][m]
        best = errs.min(axis=0)[m]
        worst = float((np.abs(at - best) / np.maximum(1.0, np.abs(best))).max()) if at.size else 0.0
        print(f"case {BK_IDS[i]} col {col}: {at.size} pairs, checker error at the kernel's index vs "
              f"checker minimum: {worst:.3g}")
        assert worst <= TOL


@pytest.mark.parametrize("i", range(len(BK_CASES)), ids=BK_IDS)
def test_best_is_the_unfused_draw_exactly(gpu, i):
    """best == FullCovHead.sample(pred, seed + kA) gathered per pedestrian, bit
    for bit (fullcov_advance is shared), and the sampler matches the checker."""
    fc, pred, r = _bk_result(i, gpu)
    c = _bk_inputs(i)
    pairs = torch.from_numpy(_bk_reference(i)["pairs"]).to(gpu)
    kA = r.per_ped[..., 2]
    want = pred.clone()
    checked = False
    for k in range(c["K"]):
        sel = pairs & (kA == k)
        if bool(sel.any()):
            xk = fc.sample(pred, seed=(c["seed"] + k) & MASK64)
            if not checked:                               # one draw per case against the checker
                ref = fr.sample(c["pred"], c["chol"], (c["seed"] + k) & MASK64)
                err = close(xk.cpu().numpy(), ref)
                print(f"case {BK_IDS[i]}: sample(seed + {k}) err {err:.3g}")
                assert err <= TOL
                checked = True
            want = torch.where(sel[:, :, None, :], xk, want)
    assert torch.equal(r.best, want)
    if bool(pairs.any()):
        assert not torch.equal(r.best, pred)


@pytest.mark.parametrize("i", [0, 3], ids=[BK_IDS[0], BK_IDS[3]])
def test_best_of_k_repeated_calls_are_bit_identical(gpu, i):
    a, b = _bk_result(i, gpu)[2], _bk_run(i, gpu)[2]
    assert torch.equal(a.sums, b.sums) and torch.equal(a.per_ped, b.per_ped)
    assert torch.equal(a.best, b.best)


@pytest.mark.parametrize("i", [0, 3], ids=[BK_IDS[0], BK_IDS[3]])
def test_reduces_to_the_per_step_head(gpu, i):
    """With the per-step head's block factor the draws are GaussianHead's
    (values within the project tolerance; the fmaf grouping differs) and so
    are minADE / minFDE."""
    from multimodaltraj_2_amd.fullcov import FullCovHead
    from multimodaltraj_2_amd.nll import GaussianHead
    c = _bk_inputs(i)
    sigma = BK_CASES[i][4]
    rng = np.random.default_rng(40 + i)
    head = np.stack([np.log(sigma) + 0.2 * rng.standard_normal(12),
                     np.log(sigma) + 0.2 * rng.standard_normal(12),
                     0.5 * rng.standard_normal(12)]).astype(np.float32)
    gh = GaussianHead(device=gpu)
    gh.head = _t(head, gpu)
    fc = FullCovHead.from_gaussian_head(gh.head)
    assert fc.chol.device == gh.head.device
    pred = _t(c["pred"], gpu)
    a, b = fc.sample(pred, seed=c["seed"]), gh.sample(pred, seed=c["seed"])
    err = close(a.cpu().numpy(), b.cpu().numpy())
    print(f"case {BK_IDS[i]}: sample vs GaussianHead.sample {err:.3g}")
    assert err <= TOL
    kw = dict(seed=c["seed"], n_frames=_t(c["n_frames"], gpu), ped_mask=_t(c["ped_mask"], gpu),
              targets_shared=c["shared"])
    args = (pred, _t(c["targets"], gpu), _t(c["n_active"], gpu), c["K"])
    ra, rb = fc.best_of_k(*args, **kw), gh.best_of_k(*args, **kw)
    e1 = close(ra.per_ped[..., :2].cpu().numpy(), rb.per_ped[..., :2].cpu().numpy())
    e2 = close(ra.sums.cpu().numpy(), rb.sums.cpu().numpy())
    print(f"case {BK_IDS[i]}: best_of_k vs g2k_best_of_k_f32: per_ped {e1:.3g}, sums {e2:.3g}")
    assert e1 <= TOL and e2 <= TOL
    assert ra.pairs == rb.pairs > 0


def _msd2(x, pred):
    """Mean squared second difference over the steps of draw - pred [S, F, 24, N]."""
    d = (x - pred).reshape(x.shape[0], x.shape[1], 2, 12, x.shape[3])
    dd = d[:, :, :, 2:] - 2 * d[:, :, :, 1:-1] + d[:, :, :, :-2]
    return float((dd ** 2).mean())


def test_random_walk_factor_draws_smooth_trajectories(gpu):
    """L[2t+c][2u+c] = sigma for u <= t: a draw is a random walk.  Its mean
    squared second difference is below that of the per-step head with the same
    marginals (sigma_t = sigma sqrt(t + 1)) by the factor the checker computes
    for the same draws (both are sums over the same normals: deterministic)."""
    from multimodaltraj_2_amd.fullcov import FullCovHead
    from multimodaltraj_2_amd.nll import GaussianHead
    from oracle import g2k_ref as ref
    sigma, seed = 0.05, 1234
    rng = np.random.default_rng(9)
    pred = rng.standard_normal((2, 2, 24, 32)).astype(np.float32)
    Lm = np.zeros((24, 24), np.float32)
    for t in range(12):
        for u in range(t + 1):
            Lm[2 * t, 2 * u] = Lm[2 * t + 1, 2 * u + 1] = sigma
    head = np.zeros((3, 12), np.float32)
    head[:2] = np.log(sigma * np.sqrt(np.arange(12) + 1.0))
    p = _t(pred, gpu)
    gh = GaussianHead(device=gpu)
    gh.head = _t(head, gpu)
    walk = _msd2(_head(Lm, gpu).sample(p, seed=seed).double().cpu().numpy(), pred.astype(np.float64))
    indep = _msd2(gh.sample(p, seed=seed).double().cpu().numpy(), pred.astype(np.float64))
    rwalk = _msd2(fr.sample(pred, Lm, seed), pred.astype(np.float64))
    rindep = _msd2(ref.gauss_sample(pred, head, seed), pred.astype(np.float64))
    print(f"mean squared second difference: walk {walk:.6g} (checker {rwalk:.6g}), independent steps "
          f"{indep:.6g} (checker {rindep:.6g}); ratio {indep / walk:.4g} (checker {rindep / rwalk:.4g})")
    # expected: walk 2 sigma^2 (the difference of two steps' normals) against
    # (6 t + 6) sigma^2 averaged over t = 1..10, 39 sigma^2: a factor near 20
    assert rindep / rwalk > 10 and walk < indep
    assert close(walk, rwalk) <= TOL and close(indep, rindep) <= TOL
    assert close(indep / walk, rindep / rwalk) <= TOL


# ---------------------------------------------------------------------------
# stats and fit
# ---------------------------------------------------------------------------
#           S   F  Nmax n_active            n_frames   mask    shared
ST_CASES = [(3, 2, 40, [40, 38, 40], [2, 2, 2], "one", False),
            (20, 2, 31, "rand", "rand", "rand", False),
            (2, 1, 256, [256, 130], None, None, False),
            (5, 3, 33, [33, 0, 17, 33, 1], [3, 3, 2, 0, 3], "rand", True),
            (2, 1, 9, [9, 4], [1, 1], "one", False),
            (2, 2, 9, [0, 0], [2, 2], "one", False)]
ST_IDS = ["one", "rows", "n256", "shared", "rank", "none"]
WELL = [0, 1, 2]                                          # >= 200 pairs, cond(C) <= 1e3


def _known_factor(rng):
    Lm = np.zeros((24, 24))
    for i in range(24):
        for j in range(i + 1):
            Lm[i, j] = 0.05 * (1.0 if i == j else 0.6 ** ((i - j + 1) // 2)) * (0.5 + rng.random())
    return Lm


@functools.lru_cache(maxsize=None)
def _st_inputs(i):
    S, F, N, nact, nfr, masked, shared = ST_CASES[i]
    rng = np.random.default_rng(700 + i)
    if isinstance(nact, str):
        nact = rng.integers(N // 2, N + 1, S)
        nact[3] = 0
    if isinstance(nfr, str):
        nfr = rng.integers(1, F + 1, S)
        nfr[5] = 0
    nact = np.asarray(nact, np.int32)
    nfr = None if nfr is None else np.asarray(nfr, np.int32)
    pm = None
    if masked == "one":
        pm = np.ones((S, N), np.uint8)
        pm[:, 2] = 0
    elif masked == "rand":
        pm = (rng.random((S, N)) > 0.2).astype(np.uint8)
    Lk = _known_factor(rng)
    pred = rng.standard_normal((S, F, 24, N)).astype(np.float32)
    Ft = 1 if shared else F
    r = rng.standard_normal((S, Ft, N, 24)) @ Lk.T
    tg = np.empty((S, Ft, N, 12, 2))
    tg[..., 0] = np.transpose(pred[:, :Ft, :12], (0, 1, 3, 2)) + r[..., 0::2]
    tg[..., 1] = np.transpose(pred[:, :Ft, 12:], (0, 1, 3, 2)) + r[..., 1::2]
    tg = np.ascontiguousarray(tg.astype(np.float32))
    chol = np.tril(Lk * rng.uniform(0.8, 1.25, (24, 24))).astype(np.float32)
    chol[np.triu_indices(24, 1)] = np.nan
    m = pair_mask(S, F, N, nact, nfr, pm)
    np.transpose(pred, (0, 1, 3, 2))[~m] = np.nan         # a view: pred itself
    if shared:
        tg[:, 0][~m.any(axis=1)] = np.nan
    else:
        tg[~m] = np.nan
    return dict(pred=pred, targets=tg, chol=chol, n_active=nact, n_frames=nfr, ped_mask=pm,
                shared=shared, pairs=int(m.sum()))


@functools.lru_cache(maxsize=None)
def _st_reference(i, chol="case"):
    c = _st_inputs(i)
    return fr.stats_ref(c["pred"], c["targets"], c["n_active"], chol=c["chol"] if chol == "case" else None,
                        r2=fr.levels_r2(LEVELS) if chol == "case" else None, n_frames=c["n_frames"],
                        ped_mask=c["ped_mask"])


def _st_run(i, dev, chol="case", levels=LEVELS):
    c = _st_inputs(i)
    if chol is None:
        fc = _head(np.eye(24, dtype=np.float32), dev)
    else:
        fc = _head(c["chol"] if isinstance(chol, str) else chol, dev)
    r = fc.stats(_t(c["pred"], dev), _t(c["targets"], dev), _t(c["n_active"], dev), levels,
                 n_frames=_t(c["n_frames"], dev), ped_mask=_t(c["ped_mask"], dev),
                 targets_shared=c["shared"], use_head=chol is not None)
    torch.cuda.synchronize()
    return r


_ST = {}


def _st_result(i, dev):
    if i not in _ST:
        _ST[i] = _st_run(i, dev)
    return _ST[i]


def _ws_bytes(i, nl=NL):
    S, F, N = ST_CASES[i][:3]
    d = _lib.G2KDims(S, F, 8, 12, 16, 64, N, 8, 0)
    return int(_lib.load().g2k_fullcov_stats_workspace_bytes(ctypes.byref(d), nl))


def test_stats_cases_cover_both_reductions_and_ranks():
    """By the kernel's own geometry: "rows" is three workgroups (the rows
    kernel) whose ranges end inside a scene-frame, the others are one."""
    row = (460 + 13 * NL) * 8
    assert [_ws_bytes(i) for i in (0, 2, 3, 4, 5)] == [0] * 5
    assert _ws_bytes(1) == 3 * row
    S, F, N = ST_CASES[1][:3]
    assert -(-S * F * N // 3) % N != 0
    pairs = [_st_inputs(i)["pairs"] for i in range(len(ST_CASES))]
    assert all(pairs[i] >= 200 for i in WELL), pairs
    assert 24 <= pairs[3] < 200 and 1 <= pairs[4] < 24 and pairs[5] == 0, pairs
    for i in WELL:
        assert np.linalg.cond(_st_reference(i)["C"]) <= 1e3


@pytest.mark.parametrize("i", range(len(ST_CASES)), ids=ST_IDS)
def test_stats_values_match_checker(gpu, i):
    r = _st_result(i, gpu)
    R = _st_reference(i)
    n = _st_inputs(i)["pairs"]
    mo, st = r.moments.cpu().numpy(), r.stats.cpu().numpy()
    assert mo.dtype == st.dtype == np.float64 and np.all(np.isfinite(mo)) and np.all(np.isfinite(st))
    assert r.pairs == R["pairs"] == n
    np.testing.assert_array_equal(st[:, 0], np.full(12, n, np.float64))
    assert np.all(st[:, 3] == 0)
    np.testing.assert_array_equal(mo[:24], mo[:24].T)     # both triangles, equal
    em = np.max(np.abs(mo - R["moments"]) / np.maximum(1.0, np.abs(R["moments"])))
    es = np.max(np.abs(st - R["stats"]) / np.maximum(1.0, np.abs(R["stats"])))
    print(f"case {ST_IDS[i]}: {n} pairs, moments err {em:.3g}, stats err {es:.3g}")
    assert em <= 1e-12 and es <= 1e-12
    ins = r.inside.cpu().numpy()
    assert ins.dtype == np.int64 and ins.shape == (13, NL)
    if n:
        r2 = fr.levels_r2(LEVELS)
        qs = np.concatenate([R["q_t"], R["q"][:, None]], axis=1)         # [P, 13]
        rad = np.concatenate([np.repeat(r2[:1], 12, axis=0), r2[1:]], axis=0)   # [13, NL]
        lo = (qs[:, :, None] <= (rad * (1 - 1e-9))[None]).sum(axis=0)
        hi = (qs[:, :, None] <= (rad * (1 + 1e-9))[None]).sum(axis=0)
        assert np.array_equal(lo, hi), "no q may lie within 1e-9 of a level's radius"
    np.testing.assert_array_equal(ins, R["inside"])
    if n == 0:
        assert np.all(mo == 0) and np.all(st == 0) and np.all(ins == 0)


@pytest.mark.parametrize("i", range(len(ST_CASES)), ids=ST_IDS)
def test_fit_matches_checker(gpu, i):
    r = _st_result(i, gpu)
    R = _st_reference(i)
    n = _st_inputs(i)["pairs"]
    fit = r.fit.cpu().numpy()
    assert fit.dtype == np.float32 and fit.shape == (24, 24)
    assert np.all(fit[np.triu_indices(24, 1)] == 0) and np.all(np.diag(fit) > 0)
    if n == 0:
        np.testing.assert_array_equal(fit, np.eye(24, dtype=np.float32))
        return
    f64 = fit.astype(np.float64)
    eb = np.abs(f64 @ f64.T - R["C"]).max() / np.abs(R["C"]).max()
    print(f"case {ST_IDS[i]}: {n} pairs, |fit fit^T - C| / max|C| {eb:.3g}, factor err {close(fit, R['fit']):.3g}")
    assert eb <= 1e-4                                     # backward-stable in L L^T, whatever the rank
    if i in WELL:
        assert close(fit, R["fit"]) <= TOL
        at = _st_run(i, gpu, chol=r.fit)
        print(f"case {ST_IDS[i]}: q_ratio at the device-written fit 1 + {at.q_ratio - 1:.3g}")
        assert abs(at.q_ratio - 1.0) <= 1e-4


@pytest.mark.parametrize("i", [0, 1], ids=[ST_IDS[0], ST_IDS[1]])
def test_stats_properties_are_the_definitions(gpu, i):
    r = _st_result(i, gpu)
    R = _st_reference(i)
    n = R["pairs"]
    assert abs(r.nll - R["stats"][:, 1].sum() / n) <= 1e-12 * max(1.0, abs(r.nll))
    np.testing.assert_allclose(r.nll_per_step, R["stats"][:, 1] / n, rtol=1e-12)
    assert abs(r.q_ratio - R["stats"][:, 2].sum() / (24 * n)) <= 1e-12
    np.testing.assert_array_equal(r.coverage, R["inside"][:12] / n)
    np.testing.assert_array_equal(r.coverage_joint, R["inside"][12] / n)
    assert r.ece_joint == float(np.abs(r.coverage_joint - np.asarray(LEVELS)).mean())
    np.testing.assert_allclose(r.cov, R["moments"][:24] / n, rtol=0, atol=1e-12)
    c = R["moments"][:24] / n
    cx = c[0::2, 0::2]
    want = cx / np.sqrt(np.outer(np.diag(cx), np.diag(cx)))
    np.testing.assert_allclose(r.step_corr, want, rtol=0, atol=1e-12)
    assert abs(r.lag1_corr - np.diag(want, 1).mean()) <= 1e-12
    # the wrapper's radii (bisection) against the checker's (Newton): two
    # float64 root finders, a few ulp apart at most
    np.testing.assert_allclose(r.r2.cpu().numpy(), fr.levels_r2(LEVELS), rtol=1e-14, atol=0)


@pytest.mark.parametrize("i", [0, 1], ids=[ST_IDS[0], ST_IDS[1]])
def test_stats_reduce_to_the_per_step_head(gpu, i):
    """With the per-step head's block factor: sum nll_t and sum q_t are
    g2k_head_stats_f32's columns 6, 7 (1e-6 relative: the f32 rounding of the
    block entries), and the steps' counts are the checker's on that factor."""
    from multimodaltraj_2_amd.fullcov import FullCovHead
    from multimodaltraj_2_amd.nll import GaussianHead
    c = _st_inputs(i)
    rng = np.random.default_rng(60 + i)
    head = np.stack([np.log(0.12) + 0.2 * rng.standard_normal(12),
                     np.log(0.12) + 0.2 * rng.standard_normal(12),
                     0.5 * rng.standard_normal(12)]).astype(np.float32)
    gh = GaussianHead(device=gpu)
    gh.head = _t(head, gpu)
    fc = FullCovHead.from_gaussian_head(gh.head)
    args = (_t(c["pred"], gpu), _t(c["targets"], gpu), _t(c["n_active"], gpu), LEVELS)
    kw = dict(n_frames=_t(c["n_frames"], gpu), ped_mask=_t(c["ped_mask"], gpu), targets_shared=c["shared"])
    a, b = fc.stats(*args, **kw), gh.stats(*args, **kw)
    sa, sb = a.stats.cpu().numpy(), b.stats.cpu().numpy()
    err = np.abs(sa[:, 1:3] - sb[:, 6:8]) / np.abs(sb[:, 6:8])
    print(f"case {ST_IDS[i]}: sum nll_t / sum q_t vs g2k_head_stats_f32: max rel err {err.max():.3g}")
    assert np.all(err <= 1e-6) and a.pairs == b.pairs
    R = fr.stats_ref(c["pred"], c["targets"], c["n_active"], chol=fc.chol.cpu().numpy(),
                     r2=fr.levels_r2(LEVELS), n_frames=c["n_frames"], ped_mask=c["ped_mask"])
    r2 = fr.levels_r2(LEVELS)[0]
    lo = (R["q_t"][:, :, None] <= (r2 * (1 - 1e-9))[None, None]).sum(axis=0)
    hi = (R["q_t"][:, :, None] <= (r2 * (1 + 1e-9))[None, None]).sum(axis=0)
    assert np.array_equal(lo, hi), "no q_t may lie within 1e-9 of a level's radius"
    np.testing.assert_array_equal(a.inside[:12].cpu().numpy(), R["inside"][:12])


def _raw(dev, c, S, F, N, chol, nl, ar):
    """The raw ABI call into guarded, poisoned outputs: float64 / int64 are
    float32 / int32 payloads of twice the length, viewed."""
    lib = _lib.load()
    d = _lib.G2KDims(S, F, 8, 12, 16, 64, N, 8, _lib.STEP_TARGETS_SHARED if c["shared"] else 0)
    mom32 = ar.alloc(2 * 25 * 24, torch.float32, "moments")
    stats32 = ar.alloc(2 * 12 * 4, torch.float32, "stats")
    inside32 = ar.alloc(2 * 13 * nl, torch.int32, "inside") if nl else None
    fit = ar.alloc((24, 24), torch.float32, "fit")
    need = int(lib.g2k_fullcov_stats_workspace_bytes(ctypes.byref(d), nl))
    ws = ar.alloc(max(need, 8), torch.uint8, "workspace")
    keep = [_t(c[k], dev) for k in ("pred", "targets", "n_active", "n_frames", "ped_mask")]
    r2 = _t(fr.levels_r2(LEVELS[:nl]), dev) if nl else None
    p = lambda t: None if t is None else t.data_ptr()
    rc = lib.g2k_fullcov_stats_f32(ctypes.byref(d), *(p(t) for t in keep), p(chol), p(r2), nl, p(mom32),
                                   p(stats32), p(inside32), p(fit), p(ws), need, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.g2k_last_error()
    ar.check_guards()
    return mom32, stats32, inside32, fit


@pytest.mark.parametrize("i", [0, 1, 5], ids=[ST_IDS[0], ST_IDS[1], ST_IDS[5]])
def test_stats_write_footprint(gpu, i):
    c = _st_inputs(i)
    S, F, N = ST_CASES[i][:3]
    mom32, stats32, inside32, fit = _raw(gpu, c, S, F, N, _t(c["chol"], gpu), NL, Arena(gpu))
    for t in (mom32, stats32, inside32, fit):
        assert all_written(t)
    r = _st_result(i, gpu)
    assert torch.equal(mom32.view(torch.float64).view(25, 24), r.moments)
    assert torch.equal(stats32.view(torch.float64).view(12, 4), r.stats)
    assert torch.equal(inside32.view(torch.int64).view(13, NL), r.inside)
    assert torch.equal(fit, r.fit)
    # fewer levels, no factor: the moments' and the fit's bits do not change
    mom3, _, ins3, fit3 = _raw(gpu, c, S, F, N, _t(c["chol"], gpu), 3, Arena(gpu))
    assert torch.equal(mom3, mom32) and torch.equal(fit3, fit)
    assert torch.equal(ins3.view(torch.int64).view(13, 3)[:, 0], r.inside[:, 0])
    mom0, stats0, _, fit0 = _raw(gpu, c, S, F, N, None, 0, Arena(gpu))
    assert all_written(mom0) and all_written(stats0) and all_written(fit0)
    st0 = stats0.view(torch.float64).view(12, 4)
    assert torch.equal(mom0, mom32) and torch.equal(fit0, fit)
    assert bool((st0[:, 1:] == 0).all()) and torch.equal(st0[:, 0], r.stats[:, 0])
    if c["pairs"] == 0:
        assert bool((mom32.view(torch.int32) == 0).all()) and bool((stats32.view(torch.int32) == 0).all())
        assert bool((inside32 == 0).all()) and torch.equal(fit, torch.eye(24, device=gpu))


@pytest.mark.parametrize("i", [1, 3], ids=[ST_IDS[1], ST_IDS[3]])
def test_stats_repeated_calls_are_bit_identical(gpu, i):
    a, b = _st_result(i, gpu), _st_run(i, gpu)
    assert torch.equal(a.moments.view(torch.int64), b.moments.view(torch.int64))
    assert torch.equal(a.stats.view(torch.int64), b.stats.view(torch.int64))
    assert torch.equal(a.inside, b.inside) and torch.equal(a.fit, b.fit)


def test_fit_sets_the_factor(gpu):
    c = _st_inputs(0)
    fc = _head(np.eye(24, dtype=np.float32), gpu)
    args = (_t(c["pred"], gpu), _t(c["targets"], gpu))
    kw = dict(n_frames=_t(c["n_frames"], gpu), ped_mask=_t(c["ped_mask"], gpu))
    st = fc.fit(*args, _t(c["n_active"], gpu), **kw)
    assert fc.chol is st.fit and torch.equal(st.fit, _st_result(0, gpu).fit)
    assert st.nll is None and st.coverage is None and st.q_ratio is None and st.inside is None
    assert bool((st.stats[:, 1:] == 0).all())
    with pytest.raises(ValueError, match="no .* pair"):
        fc.fit(*args, torch.zeros(3, dtype=torch.int32, device=gpu), **kw)


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def test_evaluation_end_to_end(gpu, tmp_path, data_root):
    """The recipe of tests/test_head_stats_gpu.py::test_evaluation_end_to_end.
    --fullcov_head train adds exactly FULLCOV_FIGURES, each finite and equal
    to a direct FullCovHead call on ``keep``'s tensors; the other keys do not
    move.  --fullcov_head eval (in-sample): the full-covariance family
    contains the block-diagonal one, so its joint NLL is not above the
    --fit_head eval run's NLL (+ 1e-3: the ridge's <= 1.2e-5 per pair and the
    f32 factor)."""
    from multimodaltraj_2_amd import checkpoint, evaluate
    from multimodaltraj_2_amd import train as tr
    from multimodaltraj_2_amd.argParser import ArgsParser
    from multimodaltraj_2_amd.fullcov import FullCovHead
    argv = ["--data_root", data_root, "--leaveDataset", "2", "--n_max", "32", "--train_scenes", "64",
            "--train_batch", "32", "--num_epochs", "2", "--loss", "l2", "--num_samples", "4",
            "--mode", "train", "--save_dir", str(tmp_path), "--log_dir", str(tmp_path),
            "--device", "cuda:0"]
    args = ArgsParser().parser.parse_args(argv)
    tr.run_train_mode(args, gpu, log=lambda s: None)
    prm = checkpoint.load_params(checkpoint.read_state(str(tmp_path)), device=gpu)
    logs0, keep0 = [], {}
    res0 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs0.append, keep=keep0)
    assert "fullcov" not in keep0 and not any("full-covariance" in s for s in logs0)

    args.fullcov_head = "train"
    logs, keep = [], {}
    res = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs.append, keep=keep)
    assert list(res) == list(res0) + list(evaluate.FULLCOV_FIGURES)
    assert {k: res[k] for k in res0} == res0
    assert sorted(set(keep) - set(keep0)) == ["fullcov", "fullcov_chol"]
    assert logs[:len(logs0)] == logs0
    assert len(logs) == len(logs0) + 1 and logs[-1].startswith("full-covariance head on dataset 2")
    # the factor is FullCovHead.fit on the fold's plan; the figures a direct call's
    fplan = evaluate.fold_plan(args, prm.nmax)
    ft, fout, fone = evaluate._fused_step(args, prm, fplan, gpu)
    fc = FullCovHead(device=gpu)
    fitted = fc.fit(fout.pred, ft["targets"], ft["n_active"], n_frames=fone, ped_mask=ft["ped_mask"])
    assert fitted.pairs > 0 and torch.equal(keep["fullcov_chol"], fc.chol)
    t = keep["plan"].to_device(gpu, F=1)
    one = torch.ones(keep["plan"].S, dtype=torch.int32, device=gpu)
    st = fc.stats(keep["pred"], t["targets"], t["n_active"], evaluate.CALIB_LEVELS, n_frames=one,
                  ped_mask=t["ped_mask"])
    bk = fc.best_of_k(keep["pred"], t["targets"], t["n_active"], 4, seed=args.sample_seed, n_frames=one,
                      ped_mask=t["ped_mask"], want_per_ped=False)
    direct = evaluate.fullcov_figures(bk, st)
    assert tuple(direct) == evaluate.FULLCOV_FIGURES
    for k in evaluate.FULLCOV_FIGURES:
        print(f"evaluation {k}: {res[k]:.8g}")
        assert np.isfinite(res[k]) and res[k] == direct[k], k
    assert bk.pairs == res["pairs"]
    cli = evaluate.main(argv + ["--fullcov_head", "train"], log=lambda s: None)
    assert [cli[k] for k in evaluate.FULLCOV_FIGURES] == [res[k] for k in evaluate.FULLCOV_FIGURES]

    # in-sample: the full-covariance optimum is not above the per-step one
    args.fullcov_head, args.fit_head = "eval", "eval"
    logs2 = []
    res2 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs2.append)
    print(f"in-sample joint NLL per pair ({res2['pairs']} pairs): full covariance "
          f"{res2['fullcov_nll']:.8g}, per-step head {res2['nll']:.8g}; lag-1 correlation "
          f"{res2['fullcov_lag1_corr']:.4f}")
    assert any(s.startswith("full-covariance head") and "in-sample" in s for s in logs2)
    assert res2["fullcov_nll"] <= res2["nll"] + 1e-3
    # in-sample sum q / 24 n is rank(M) / 24 up to the ridge: 1 only from 24 pairs on
    print(f"in-sample q_ratio {res2['fullcov_q_ratio']:.6g} on {res2['pairs']} pairs")
    assert 0.0 < res2["fullcov_q_ratio"] <= 1.0
