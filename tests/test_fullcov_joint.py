"""Joint best-of-K evaluation of the full-covariance head, the parts that need
no GPU: the entry point (g2k_fullcov_joint_eval_f32, added after ABI 11) is
declared, bound and exported and rejects bad arguments before touching a
device; its workspace is g2k_joint_eval_f32's (the row format is shared); the
float64 checker (tests/fullcov_joint_ref.py) reproduces tests/joint_ref.py for
the per-step head's block factor; the figures' tuple and the wrapper's
argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib
from tests import fullcov_ref as fr
from tests import fullcov_joint_ref as fj
from tests.joint_ref import joint_eval_ref

P = ctypes.c_void_p(16)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("g2k_fullcov_joint_eval_workspace_bytes", "g2k_fullcov_joint_eval_f32")


def _dims(**kw):
    d = dict(S=2, F=20, T=8, L=12, D=16, H=128, Nmax=32, W=27, stride=1)
    d.update(kw)
    return _lib.G2KDims(**d)


def _call(lib, d, K=20, radius=0.2, ws_bytes=1 << 30, fn="g2k_fullcov_joint_eval_f32", **null):
    a = dict(pred=P, targets=P, n_active=P, chol=P, sums_f=P, sums_i=P, ws=P)
    a.update(null)
    return getattr(lib, fn)(ctypes.byref(d), a["pred"], a["targets"], a["n_active"], None, None,
                            a["chol"], ctypes.c_uint64(5), K, ctypes.c_float(radius), None, None,
                            a["sums_f"], a["sums_i"], a["ws"], ws_bytes, None)


def test_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "g2k_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SYMBOLS, name
        assert hasattr(lib, name), name
    assert _lib.SYMBOLS[NAMES[1]] == _lib.SYMBOLS["g2k_joint_eval_f32"]      # the same signature
    assert lib.g2k_abi_version() == 11 and _lib.ABI_VERSION == 11            # added after ABI 11: by symbol


@pytest.mark.parametrize("name", ["pred", "targets", "n_active", "chol", "sums_f", "sums_i"])
def test_rejects_null(name):
    lib = _lib.load()
    assert _call(lib, _dims(), **{name: None}) == -1
    assert b"NULL" in lib.g2k_last_error()


@pytest.mark.parametrize("K", [0, 4097])
def test_rejects_k(K):
    lib = _lib.load()
    assert _call(lib, _dims(), K=K) == -1 and b"K=" in lib.g2k_last_error()


@pytest.mark.parametrize("radius", [-0.5, float("nan"), float("inf")])
def test_rejects_radius(radius):
    lib = _lib.load()
    assert _call(lib, _dims(), radius=radius) == -1 and b"radius" in lib.g2k_last_error()


@pytest.mark.parametrize("Nmax", [0, 300])
def test_rejects_nmax(Nmax):
    lib = _lib.load()
    assert _call(lib, _dims(Nmax=Nmax)) == -1 and b"Nmax" in lib.g2k_last_error()


def test_flags_as_the_per_step_entry_point():
    """G2K_STEP_TARGETS_SHARED is honoured (it passes validation); the layout
    flag neither entry point can honour is rejected with the same code."""
    lib = _lib.load()
    d = _dims(flags=_lib.STEP_PRED_PED_MAJOR)
    rc = _call(lib, d)
    assert rc != 0 and b"fullcov_joint_eval" in lib.g2k_last_error()
    assert rc == _call(lib, d, fn="g2k_joint_eval_f32")
    # shared targets: validation reaches the workspace check, the last before a launch
    d = _dims(flags=_lib.STEP_TARGETS_SHARED)
    assert _call(lib, d, ws_bytes=0) == -1 and b"workspace" in lib.g2k_last_error()


def test_workspace_and_zero_scenes():
    lib = _lib.load()
    for d in (_dims(), _dims(S=256), _dims(S=3, F=1, Nmax=256), _dims(S=1, F=0), _dims(S=0)):
        need = lib.g2k_fullcov_joint_eval_workspace_bytes(ctypes.byref(d))
        assert need == lib.g2k_joint_eval_workspace_bytes(ctypes.byref(d))   # the shared row format
    d = _dims()
    need = lib.g2k_fullcov_joint_eval_workspace_bytes(ctypes.byref(d))
    assert need == 2 * 20 * 8 * 10 * 4                  # a row [10] per (scene, frame, slice of draws)
    assert _call(lib, d, ws_bytes=need - 1) == -1 and b"workspace" in lib.g2k_last_error()
    assert _call(lib, d, ws=None) == -1 and b"workspace" in lib.g2k_last_error()
    assert _call(lib, _dims(S=0), ws_bytes=0) == 0      # nothing to run
    assert _call(lib, _dims(S=0), ws=None, ws_bytes=0) == 0
    assert lib.g2k_fullcov_joint_eval_workspace_bytes(ctypes.byref(_dims(S=-1))) == -1


def _case(seed=0, S=3, F=2, N=20, sigma=0.3):
    rng = np.random.default_rng(seed)
    pred = rng.standard_normal((S, F, 24, N)).astype(np.float32)
    base = pred.reshape(S, F, 2, 12, N).transpose(0, 1, 4, 3, 2)
    tg = (base + sigma * rng.standard_normal((S, F, N, 12, 2))).astype(np.float32)
    head = np.stack([np.log(sigma) + 0.2 * rng.standard_normal(12),
                     np.log(sigma) + 0.2 * rng.standard_normal(12),
                     0.5 * rng.standard_normal(12)]).astype(np.float32)
    pm = (rng.random((S, N)) > 0.2).astype(np.uint8)
    return pred, tg, head, np.array([N, 7, 0], np.int32), np.array([2, 1, 2], np.int32), pm


def test_checker_reduces_to_the_per_step_head():
    """With the per-step head's block factor the checker is tests/joint_ref.py:
    floats to 1e-12, every integer column exactly."""
    pred, tg, head, nact, nfr, pm = _case()
    K, radius = 4, 0.3
    A = joint_eval_ref(pred, tg, nact, head, 77, K, radius, nfr, pm)
    B = fj.joint_eval_ref(pred, tg, nact, fr.block_factor(head), 77, K, radius, nfr, pm)
    assert sorted(A) == sorted(B)
    assert A["per_frame_i"][..., 0].sum() > 20 and A["col_k"].sum() > 0
    for key in A:
        if A[key].dtype.kind == "f":
            np.testing.assert_allclose(B[key], A[key], rtol=0, atol=1e-12, err_msg=key)
        else:
            np.testing.assert_array_equal(B[key], A[key], err_msg=key)
    # entries above the diagonal are not read
    C = fj.joint_eval_ref(pred, tg, nact, fj.nan_above(fr.block_factor(head)), 77, K, radius, nfr, pm)
    np.testing.assert_allclose(C["per_frame_f"], B["per_frame_f"], rtol=0, atol=1e-6)
    assert np.isfinite(C["jade_k"]).all()


def test_walk_factor():
    sigma = 0.3
    Lm = fj.walk_factor(sigma, np.random.default_rng(1)).astype(np.float64)
    assert Lm.shape == (24, 24) and np.all(np.triu(Lm, 1) == 0)
    assert np.all(np.diag(Lm) >= 0.02 * sigma) and np.all(Lm[np.tril_indices(24)] != 0)
    base = fj.walk_factor(sigma, np.random.default_rng(1)) - np.tril(
        0.05 * sigma * np.random.default_rng(1).standard_normal((24, 24)))
    # the walk's part: the last step's standard deviation is sigma
    i, j = np.indices((24, 24))
    walk = np.where((j <= i) & ((i - j) % 2 == 0), sigma / np.sqrt(12.0), 0.0)
    assert abs(np.sqrt((walk[22] ** 2).sum()) - sigma) <= 1e-12
    assert abs(np.sqrt((walk[23] ** 2).sum()) - sigma) <= 1e-12
    off = ~np.eye(24, dtype=bool)
    np.testing.assert_allclose(base[off], walk[off], rtol=0, atol=1e-7)
    assert np.isnan(fj.nan_above(Lm)[np.triu_indices(24, 1)]).all()
    np.testing.assert_array_equal(fj.nan_above(Lm)[np.tril_indices(24)],
                                  Lm.astype(np.float32)[np.tril_indices(24)])


def test_figures_tuple():
    from multimodaltraj_2_amd import evaluate
    assert evaluate.FULLCOV_JOINT_FIGURES == ("fullcov_jade", "fullcov_jfde", "fullcov_collision_rate",
                                              "fullcov_collision_rate_best")
    assert evaluate.FULLCOV_FIGURES == ("fullcov_min_ade", "fullcov_min_fde", "fullcov_nll",
                                        "fullcov_coverage_90", "fullcov_q_ratio", "fullcov_lag1_corr")
    assert not set(evaluate.FULLCOV_JOINT_FIGURES) & set(evaluate.JOINT_FIGURES + evaluate.FULLCOV_FIGURES)


def test_wrapper_checks_arguments():
    from multimodaltraj_2_amd.fullcov import FullCovHead
    fc = FullCovHead(device="cpu")
    pred = torch.zeros((1, 1, 24, 4))
    tg = torch.zeros((1, 1, 4, 12, 2))
    na = torch.ones(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):                    # CPU tensors: no launch
        fc.joint_eval(pred, tg, na, 2, 0.1)
    for k in (0, 4097):
        with pytest.raises(ValueError, match="k = "):
            fc.joint_eval(pred, tg, na, k, 0.1)
    for r in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError, match="radius"):
            fc.joint_eval(pred, tg, na, 2, r)
    with pytest.raises(ValueError, match="pred must be"):
        fc.joint_eval(torch.zeros((1, 1, 23, 4)), tg, na, 2, 0.1)
    with pytest.raises(ValueError, match="targets must be"):
        fc.joint_eval(pred, torch.zeros((1, 1, 5, 12, 2)), na, 2, 0.1)
    with pytest.raises(ValueError, match="targets must be"):       # shared targets: one frame
        fc.joint_eval(torch.zeros((1, 2, 24, 4)), torch.zeros((1, 2, 4, 12, 2)), na, 2, 0.1,
                      targets_shared=True)
    with pytest.raises(ValueError, match="n_active"):
        fc.joint_eval(pred, tg, torch.ones(2, dtype=torch.int32), 2, 0.1)
    with pytest.raises(ValueError, match="ped_mask"):
        fc.joint_eval(pred, tg, na, 2, 0.1, ped_mask=torch.ones((1, 5), dtype=torch.uint8))
    with pytest.raises(ValueError, match="n_frames"):
        fc.joint_eval(pred, tg, na, 2, 0.1, n_frames=torch.ones(2, dtype=torch.int32))
    with pytest.raises(TypeError, match="n_active"):
        fc.joint_eval(pred, tg, torch.ones(1, dtype=torch.int64), 2, 0.1)
    fc.chol = torch.eye(23)
    with pytest.raises(ValueError, match="chol"):
        fc.joint_eval(pred, tg, na, 2, 0.1)
