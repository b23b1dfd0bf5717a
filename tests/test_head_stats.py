"""Head calibration, the parts that need no GPU: the C ABI rejects bad
arguments before touching a device (g2k_head_stats_f32, added after ABI 11),
the two new flags default to off, the wrapper validates its levels, and the
float64 checker (tests/calib_ref.py) obeys the definition's own invariants:
the closed-form fit zeroes the NLL's head gradient (oracle.g2k_ref
.bivariate_nll) and makes mean(q) / 2 exactly 1."""
import ctypes

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib
from oracle import g2k_ref as ref
from tests.calib_ref import RHO_MAX, VAR_FLOOR, head_stats_ref, levels_r2

P = ctypes.c_void_p(16)
LEVELS = (0.1, 0.5, 0.9, 0.95, 0.99)


def _dims(**kw):
    d = dict(S=2, F=20, T=8, L=12, D=16, H=128, Nmax=32, W=27, stride=1)
    d.update(kw)
    return _lib.G2KDims(**d)


def _call(lib, d, n_levels=3, ws_bytes=1 << 30, **over):
    a = dict(pred=P, targets=P, n_active=P, head=P, r2=P, stats=P, inside=P, fit=P, ws=P)
    a.update(over)
    return lib.g2k_head_stats_f32(ctypes.byref(d), a["pred"], a["targets"], a["n_active"], None, None,
                                  a["head"], a["r2"], n_levels, a["stats"], a["inside"], a["fit"],
                                  a["ws"], ws_bytes, None)


@pytest.mark.parametrize("name", ["pred", "targets", "n_active", "stats", "r2", "ws"])
def test_abi_rejects_null(name):
    lib = _lib.load()
    assert _call(lib, _dims(), **{name: None}) == -1
    assert lib.g2k_last_error()


@pytest.mark.parametrize("Nmax", [0, 257])
def test_abi_rejects_nmax(Nmax):
    lib = _lib.load()
    assert _call(lib, _dims(Nmax=Nmax)) == -1
    assert lib.g2k_head_stats_workspace_bytes(ctypes.byref(_dims(Nmax=Nmax)), 3) == -1


@pytest.mark.parametrize("n_levels", [-1, 33])
def test_abi_rejects_levels(n_levels):
    lib = _lib.load()
    assert _call(lib, _dims(), n_levels=n_levels) == -1
    assert lib.g2k_head_stats_workspace_bytes(ctypes.byref(_dims()), n_levels) == -1


def test_abi_no_head_takes_no_levels():
    lib = _lib.load()
    assert _call(lib, _dims(), head=None, n_levels=3) == -1 and b"head" in lib.g2k_last_error()
    assert _call(lib, _dims(), head=None, n_levels=0, r2=None) == -1      # inside still given
    assert _call(lib, _dims(S=0), head=None, n_levels=0, r2=None, inside=None) == 0


def test_abi_workspace_and_zero_scenes():
    lib = _lib.load()
    d = _dims()                                           # 1280 slots: three workgroups' rows
    need = lib.g2k_head_stats_workspace_bytes(ctypes.byref(d), 3)
    assert need == 3 * (96 + 12 * 3) * 8
    assert _call(lib, d, ws_bytes=need - 4) == -1 and b"workspace" in lib.g2k_last_error()
    assert lib.g2k_head_stats_workspace_bytes(ctypes.byref(_dims(S=1, F=1)), 3) == 0   # one workgroup
    assert _call(lib, _dims(S=0), ws_bytes=0) == 0        # nothing to run
    assert lib.g2k_head_stats_workspace_bytes(ctypes.byref(_dims(S=-1)), 3) == -1
    assert lib.g2k_abi_version() == 11 and _lib.ABI_VERSION == 11


def test_flags_default_off():
    from multimodaltraj_2_amd.argParser import ArgsParser
    a = ArgsParser().parser.parse_args([])
    assert (a.fit_head, a.calibration) == ("off", 0)
    a = ArgsParser().parser.parse_args(["--num_samples", "20", "--fit_head", "train", "--calibration", "1"])
    assert (a.fit_head, a.calibration) == ("train", 1)
    assert ArgsParser().parser.parse_args(["--fit_head", "eval"]).fit_head == "eval"
    with pytest.raises(SystemExit):
        ArgsParser().parser.parse_args(["--fit_head", "both"])


@pytest.mark.parametrize("levels", [(0.0,), (1.0,), (0.5, -0.1), (0.5, 1.5), tuple([0.5] * 33)])
def test_wrapper_rejects_levels(levels):
    from multimodaltraj_2_amd.nll import GaussianHead
    gh = GaussianHead(device="cpu")
    z = torch.zeros(1)
    with pytest.raises(ValueError, match="level"):
        gh.stats(z, z, z, levels)


def _case(seed=0, S=3, F=2, N=9):
    """tests/test_best_of_k.py::_case's shapes with an anisotropic, correlated
    residual that grows with the step."""
    rng = np.random.default_rng(seed)
    pred = rng.standard_normal((S, F, 24, N)).astype(np.float32)
    e = rng.standard_normal((S, F, N, 12, 2))
    grow = (0.2 + 0.05 * np.arange(12))[None, None, None, :]
    rx = grow * e[..., 0]
    ry = 0.5 * grow * (0.6 * e[..., 0] + 0.8 * e[..., 1])
    tg = (pred.reshape(S, F, 2, 12, N).transpose(0, 1, 4, 3, 2) + np.stack([rx, ry], -1)).astype(np.float32)
    return pred, tg, np.array([0, 5, N], np.int32)[:S]


def _oracle_nll(pred, tg, head, nact):
    nll, pairs, dhead = 0.0, 0, np.zeros((3, 12))
    for s in range(pred.shape[0]):
        a, p, dh, _ = ref.bivariate_nll(pred[s], tg[s], head, int(nact[s]), pred.shape[1])
        nll, pairs, dhead = nll + a, pairs + p, dhead + dh
    return nll, pairs, dhead


def test_checker_fit_zeroes_the_gradient():
    pred, tg, nact = _case()
    R = head_stats_ref(pred, tg, nact)
    assert R["pairs"] == 2 * (5 + 9) and np.all(R["stats"][:, 0] == R["pairs"])
    assert np.all(R["stats"][:, 6:] == 0)                     # no head: no nll, no q
    _, pairs, dhead = _oracle_nll(pred, tg, R["fit"], nact)
    assert pairs == R["pairs"]
    print(f"max |dhead| at the fit: {np.abs(dhead).max():.3g} ({pairs} pairs)")
    assert np.abs(dhead).max() <= 1e-9 * pairs
    # at the fit mean(q) / 2 is 1, step by step, and the NLL is the oracle's
    A = head_stats_ref(pred, tg, nact, head=R["fit"], r2=levels_r2(LEVELS))
    np.testing.assert_allclose(A["stats"][:, 7] / (2 * pairs), 1.0, rtol=0, atol=1e-12)
    nll, _, _ = _oracle_nll(pred, tg, R["fit"], nact)
    assert abs(A["stats"][:, 6].sum() - nll) <= 1e-9 * abs(nll)
    # off the fit the gradient is far from zero (row 0 raised by 0.1)
    off = R["fit"].copy()
    off[0] += 0.1
    _, _, dh = _oracle_nll(pred, tg, off, nact)
    assert np.all(np.abs(dh[0]) >= 0.05 * pairs)


def test_checker_inside_is_monotone():
    pred, tg, nact = _case(seed=4)
    head = head_stats_ref(pred, tg, nact)["fit"]
    levels = (0.01, 0.1, 0.5, 0.9, 0.99, 0.999999)
    A = head_stats_ref(pred, tg, nact, head=head, r2=levels_r2(levels))
    assert np.all(np.diff(A["inside"], axis=1) >= 0)
    assert np.all(A["inside"] <= A["pairs"]) and np.all(A["inside"] >= 0)
    assert A["inside"][:, -1].sum() > A["inside"][:, 0].sum()


def test_checker_clamps():
    pred, tg, nact = _case(seed=5)
    base = pred.reshape(3, 2, 2, 12, 9).transpose(0, 1, 4, 3, 2)      # [S, F, N, 12, 2]
    tg = tg.copy()
    tg[:, :, :, 3] = base[:, :, :, 3]                         # step 3: target == pred
    pred = pred.copy()
    pv = pred.reshape(3, 2, 2, 12, 9)
    pv[:, :, :, 7] = 0.0                                      # step 7: dy = 2 dx exactly
    small = np.round(8 * np.random.default_rng(6).standard_normal((3, 2, 9))) / 8 + 0.0625
    tg[:, :, :, 7, 0] = small
    tg[:, :, :, 7, 1] = 2 * small
    fit = head_stats_ref(pred, tg, nact)["fit"]
    assert fit[0, 3] == fit[1, 3] == 0.5 * np.log(VAR_FLOOR) and fit[2, 3] == 0.0
    assert fit[2, 7] == np.arctanh(RHO_MAX) and fit[2, 7] == np.arctanh(1 - 1e-6)
    # a launch without any pair: zeros
    Z = head_stats_ref(pred, tg, np.zeros(3, np.int32))
    assert Z["pairs"] == 0 and np.all(Z["fit"] == 0) and np.all(Z["stats"] == 0)
