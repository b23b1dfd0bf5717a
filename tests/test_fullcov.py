"""The full-covariance trajectory head, the parts that need no GPU: the three
entry points (g2k_fullcov_stats_f32, g2k_fullcov_sample_f32,
g2k_fullcov_best_of_k_f32; added after ABI 11) reject bad arguments before
touching a device, the flag defaults to off, chi2_even_quantile reproduces
known quantiles, from_gaussian_head builds the per-step head's blocks, and the
float64 checker (tests/fullcov_ref.py) obeys the definition's own invariant:
at its own fit, sum q / (24 n) is 1 up to the ridge."""
import ctypes
import math

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib
from tests import fullcov_ref as fr

P = ctypes.c_void_p(16)


def _dims(**kw):
    d = dict(S=2, F=20, T=8, L=12, D=16, H=128, Nmax=32, W=8, stride=0)
    d.update(kw)
    return _lib.G2KDims(**d)


def _stats(lib, d, n_levels=3, ws_bytes=1 << 30, **over):
    a = dict(pred=P, targets=P, n_active=P, chol=P, r2=P, moments=P, stats=P, inside=P, fit=P, ws=P)
    a.update(over)
    return lib.g2k_fullcov_stats_f32(ctypes.byref(d), a["pred"], a["targets"], a["n_active"], None, None,
                                     a["chol"], a["r2"], n_levels, a["moments"], a["stats"],
                                     a["inside"], a["fit"], a["ws"], ws_bytes, None)


def _bestk(lib, d, K=20, ws_bytes=1 << 30, **over):
    a = dict(pred=P, targets=P, n_active=P, chol=P, per_ped=P, best=P, out=P, ws=P)
    a.update(over)
    return lib.g2k_fullcov_best_of_k_f32(ctypes.byref(d), a["pred"], a["targets"], a["n_active"], None,
                                         None, a["chol"], ctypes.c_uint64(7), K, a["per_ped"],
                                         a["best"], a["out"], a["ws"], ws_bytes, None)


def _sample(lib, d, **over):
    a = dict(pred=P, chol=P, out=P)
    a.update(over)
    return lib.g2k_fullcov_sample_f32(ctypes.byref(d), a["pred"], a["chol"], ctypes.c_uint64(7),
                                      a["out"], None)


@pytest.mark.parametrize("name", ["pred", "targets", "n_active", "moments", "stats", "r2", "ws"])
def test_stats_rejects_null(name):
    lib = _lib.load()
    assert _stats(lib, _dims(), **{name: None}) == -1
    assert lib.g2k_last_error()


@pytest.mark.parametrize("name", ["pred", "targets", "n_active", "chol", "out", "ws"])
def test_best_of_k_rejects_null(name):
    lib = _lib.load()
    assert _bestk(lib, _dims(), **{name: None}) == -1
    assert lib.g2k_last_error()


@pytest.mark.parametrize("name", ["pred", "chol", "out"])
def test_sample_rejects_null(name):
    lib = _lib.load()
    assert _sample(lib, _dims(), **{name: None}) == -1
    assert lib.g2k_last_error()


@pytest.mark.parametrize("K", [0, 4097])
def test_best_of_k_rejects_k(K):
    lib = _lib.load()
    assert _bestk(lib, _dims(), K=K) == -1 and b"K=" in lib.g2k_last_error()


@pytest.mark.parametrize("Nmax", [0, 257])
def test_rejects_nmax(Nmax):
    lib = _lib.load()
    d = _dims(Nmax=Nmax)
    assert _stats(lib, d) == -1
    assert _bestk(lib, d) == -1
    assert _sample(lib, d) == -1
    assert lib.g2k_fullcov_stats_workspace_bytes(ctypes.byref(d), 3) == -1


def test_stats_rejects_levels():
    lib = _lib.load()
    assert _stats(lib, _dims(), n_levels=33) == -1
    assert lib.g2k_fullcov_stats_workspace_bytes(ctypes.byref(_dims()), 33) == -1
    assert _stats(lib, _dims(), n_levels=-1) == -1
    # no factor: no levels, no counts
    assert _stats(lib, _dims(), chol=None, n_levels=3) == -1 and b"chol" in lib.g2k_last_error()
    assert _stats(lib, _dims(), chol=None, n_levels=0, r2=None) == -1          # inside still given
    assert _stats(lib, _dims(S=0), chol=None, n_levels=0, r2=None, inside=None) == 0
    # scene-frames are indexed in 32 bits
    assert _stats(lib, _dims(S=1 << 20, F=1 << 12)) == -1


def test_workspaces_and_zero_scenes():
    lib = _lib.load()
    d = _dims()                                           # 1280 slots: three workgroups' rows
    need = lib.g2k_fullcov_stats_workspace_bytes(ctypes.byref(d), 3)
    assert need == 3 * (460 + 13 * 3) * 8
    assert _stats(lib, d, ws_bytes=need - 4) == -1 and b"workspace" in lib.g2k_last_error()
    assert lib.g2k_fullcov_stats_workspace_bytes(ctypes.byref(_dims(S=1, F=1)), 3) == 0   # one workgroup
    assert _stats(lib, _dims(S=0), ws_bytes=0) == 0       # nothing to run
    assert lib.g2k_fullcov_stats_workspace_bytes(ctypes.byref(_dims(S=-1)), 3) == -1
    bneed = lib.g2k_fullcov_best_of_k_workspace_bytes(ctypes.byref(d))
    assert bneed == lib.g2k_best_of_k_workspace_bytes(ctypes.byref(d)) == 2 * 20 * 8 * 4
    assert _bestk(lib, d, ws_bytes=bneed - 4) == -1 and b"workspace" in lib.g2k_last_error()
    assert _bestk(lib, _dims(S=0), ws_bytes=0, ws=None) == 0
    assert _sample(lib, _dims(S=0)) == 0
    assert lib.g2k_abi_version() == 11 and _lib.ABI_VERSION == 11   # added after ABI 11: by symbol


def test_flag_defaults_off():
    from multimodaltraj_2_amd.argParser import ArgsParser
    assert ArgsParser().parser.parse_args([]).fullcov_head == "off"
    for mode in ("off", "train", "eval"):
        assert ArgsParser().parser.parse_args(["--fullcov_head", mode]).fullcov_head == mode
    with pytest.raises(SystemExit):
        ArgsParser().parser.parse_args(["--fullcov_head", "both"])
    from multimodaltraj_2_amd import evaluate
    assert evaluate.FULLCOV_FIGURES == ("fullcov_min_ade", "fullcov_min_fde", "fullcov_nll",
                                        "fullcov_coverage_90", "fullcov_q_ratio", "fullcov_lag1_corr")


def test_chi2_even_quantile():
    from multimodaltraj_2_amd.fullcov import chi2_even_quantile
    for p, want in ((0.5, 23.3367), (0.9, 33.1962), (0.95, 36.4150)):
        got = chi2_even_quantile(p, 24)
        assert abs(got - want) <= 5e-5, (p, got)
        assert abs(got - fr.chi2_even_quantile(p, 24)) <= 1e-12 * got      # bisection vs Newton
    for p in (1e-6, 0.1, 0.5, 0.9, 0.99, 1 - 1e-9):
        assert chi2_even_quantile(p, 2) == -2.0 * math.log1p(-p)
        # NumPy's log1p may round the last bit differently from libm's
        assert abs(chi2_even_quantile(p, 2) + 2.0 * np.log1p(-p)) <= 4.5e-16 * chi2_even_quantile(p, 2)
    # the CDF at the quantile is p (dof 4: 1 - exp(-x/2) (1 + x/2))
    x = chi2_even_quantile(0.3, 4)
    assert abs(1 - np.exp(-x / 2) * (1 + x / 2) - 0.3) <= 1e-14
    for bad in ((0.5, 3), (0.5, 0), (0.0, 24), (1.0, 24)):
        with pytest.raises(ValueError):
            chi2_even_quantile(*bad)


@pytest.mark.parametrize("levels", [(0.0,), (1.0,), (0.5, -0.1), tuple([0.5] * 33)])
def test_wrapper_rejects_levels(levels):
    from multimodaltraj_2_amd.fullcov import FullCovHead
    fc = FullCovHead(device="cpu")
    z = torch.zeros(1)
    with pytest.raises(ValueError, match="level"):
        fc.stats(z, z, z, levels)


def test_from_gaussian_head():
    from multimodaltraj_2_amd.fullcov import FullCovHead
    fc = FullCovHead(device="cpu")
    assert fc.chol.dtype == torch.float32 and torch.equal(fc.chol, torch.eye(24))
    rng = np.random.default_rng(3)
    head = np.stack([np.log(0.3) + 0.2 * rng.standard_normal(12), np.log(0.2) + 0.2 * rng.standard_normal(12),
                     0.5 * rng.standard_normal(12)]).astype(np.float32)
    got = FullCovHead.from_gaussian_head(torch.from_numpy(head)).chol
    assert got.dtype == torch.float32 and tuple(got.shape) == (24, 24) and got.device.type == "cpu"
    want = np.zeros((24, 24))
    for t in range(12):
        sx, sy, rho = np.exp(float(head[0, t])), np.exp(float(head[1, t])), np.tanh(float(head[2, t]))
        want[2 * t:2 * t + 2, 2 * t:2 * t + 2] = [[sx, 0.0], [sy * rho, sy * np.sqrt(1 - rho * rho)]]
    np.testing.assert_array_equal(got.numpy(), want.astype(np.float32))
    np.testing.assert_array_equal(got.numpy(), fr.block_factor(head).astype(np.float32))
    with pytest.raises(ValueError):
        FullCovHead.from_gaussian_head(torch.zeros(2, 12))


def _known_factor(rng, cond_target=300.0):
    """A random-walk-like factor: dense lower triangle, decaying with the lag."""
    Lm = np.zeros((24, 24))
    for i in range(24):
        for j in range(i + 1):
            Lm[i, j] = 0.05 * (1.0 if i == j else 0.6 ** ((i - j + 1) // 2)) * (0.5 + rng.random())
    return Lm


@pytest.mark.parametrize("seed,S,N", [(0, 4, 30), (1, 5, 40)])
def test_checker_fit_whitens_its_own_residuals(seed, S, N):
    """Residuals drawn from a known factor (>= 200 pairs): at the checker's own
    f32-rounded fit sum q / (24 n) is 1 within 1e-4 (the ridge's 1e-6 and the
    rounding of the factor), the moments are the residuals', and the fit
    reproduces the ridged covariance."""
    rng = np.random.default_rng(seed)
    Lm = _known_factor(rng)
    F = 2
    pred = rng.standard_normal((S, F, 24, N)).astype(np.float32)
    r = rng.standard_normal((S, F, N, 24)) @ Lm.T
    tg = np.empty((S, F, N, 12, 2))
    tg[..., 0] = np.transpose(pred[:, :, :12], (0, 1, 3, 2)) + r[..., 0::2]
    tg[..., 1] = np.transpose(pred[:, :, 12:], (0, 1, 3, 2)) + r[..., 1::2]
    tg = tg.astype(np.float32)
    nact = np.full(S, N, np.int32)
    A = fr.stats_ref(pred, tg, nact)
    assert A["pairs"] == S * F * N >= 200 and np.all(A["stats"][:, 1:] == 0)
    fit32 = A["fit"].astype(np.float32)
    cond = np.linalg.cond(A["C"])
    B = fr.stats_ref(pred, tg, nact, chol=fit32, r2=fr.levels_r2((0.5, 0.9)))
    ratio = B["stats"][:, 2].sum() / (24 * B["pairs"])
    print(f"pairs {A['pairs']}, cond(C) {cond:.3g}, sum q / 24 n at the f32 fit: 1 + {ratio - 1:.3g}")
    assert abs(ratio - 1.0) <= 1e-4
    np.testing.assert_allclose(A["fit"] @ A["fit"].T, A["C"], rtol=0, atol=1e-12 * np.abs(A["C"]).max())
    assert np.all(np.triu(A["fit"], 1) == 0) and np.all(np.diag(A["fit"]) > 0)
    np.testing.assert_array_equal(B["moments"], A["moments"])
    # the counts are monotone in the level and bounded by the pairs
    assert np.all(B["inside"][:, 0] <= B["inside"][:, 1]) and np.all(B["inside"] <= B["pairs"])
    # joint coverage is near its level on Gaussian residuals
    assert abs(B["inside"][12, 1] / B["pairs"] - 0.9) < 0.1


def test_checker_sample_reduces_to_the_per_step_head():
    """x = mu + L z with the per-step head's blocks is oracle gauss_sample."""
    from oracle import g2k_ref as ref
    rng = np.random.default_rng(5)
    pred = rng.standard_normal((2, 3, 24, 7))
    head = np.stack([np.log(0.3) + 0.2 * rng.standard_normal(12), np.log(0.2) + 0.2 * rng.standard_normal(12),
                     0.5 * rng.standard_normal(12)])
    got = fr.sample(pred, fr.block_factor(head), 12345)
    np.testing.assert_allclose(got, ref.gauss_sample(pred, head, 12345), rtol=0, atol=1e-13)
    # entries above the diagonal are not read
    Ln = fr.block_factor(head)
    Ln[np.triu_indices(24, 1)] = np.nan
    np.testing.assert_array_equal(fr.sample(pred, Ln, 12345), got)


def test_checker_no_pair():
    pred = np.zeros((1, 1, 24, 3), np.float32)
    tg = np.zeros((1, 1, 3, 12, 2), np.float32)
    Z = fr.stats_ref(pred, tg, np.zeros(1, np.int32), chol=np.eye(24), r2=fr.levels_r2((0.5,)))
    assert Z["pairs"] == 0 and np.all(Z["moments"] == 0) and np.all(Z["stats"] == 0)
    assert np.all(Z["inside"] == 0) and np.array_equal(Z["fit"], np.eye(24))
