"""Joint best-of-K evaluation, the parts that need no GPU: the C ABI rejects
bad arguments before touching a device (g2k_joint_eval_f32, ABI 11), the new
flag defaults to off, and the float64 checker (tests/joint_ref.py) obeys the
definition's own invariants and a structured case counted by hand."""
import ctypes

import numpy as np
import pytest

from multimodaltraj_2_amd import _lib
from tests.bestk_ref import best_of_k_ref
from tests.joint_ref import couples_case, joint_eval_ref

P = ctypes.c_void_p(16)


def _dims(**kw):
    d = dict(S=2, F=20, T=8, L=12, D=16, H=128, Nmax=32, W=27, stride=1)
    d.update(kw)
    return _lib.G2KDims(**d)


def _call(lib, d, K=20, radius=0.2, ws_bytes=1 << 30, **null):
    a = dict(pred=P, targets=P, n_active=P, head=P, sums_f=P, sums_i=P, ws=P)
    a.update(null)
    return lib.g2k_joint_eval_f32(ctypes.byref(d), a["pred"], a["targets"], a["n_active"], None, None,
                                  a["head"], ctypes.c_uint64(5), K, ctypes.c_float(radius), None, None,
                                  a["sums_f"], a["sums_i"], a["ws"], ws_bytes, None)


def test_abi_version_is_11():
    assert _lib.ABI_VERSION == 11 and _lib.load().g2k_abi_version() == 11


@pytest.mark.parametrize("name", ["pred", "targets", "n_active", "head", "sums_f", "sums_i"])
def test_abi_rejects_null(name):
    lib = _lib.load()
    assert _call(lib, _dims(), **{name: None}) == -1
    assert lib.g2k_last_error()


@pytest.mark.parametrize("K", [0, -3, 4097])
def test_abi_rejects_k(K):
    assert _call(_lib.load(), _dims(), K=K) == -1


@pytest.mark.parametrize("Nmax", [0, 257])
def test_abi_rejects_nmax(Nmax):
    assert _call(_lib.load(), _dims(Nmax=Nmax)) == -1


@pytest.mark.parametrize("radius", [float("nan"), float("inf"), -float("inf"), -0.5])
def test_abi_rejects_radius(radius):
    lib = _lib.load()
    assert _call(lib, _dims(), radius=radius) == -1
    assert b"radius" in lib.g2k_last_error()


def test_abi_workspace_and_zero_scenes():
    lib = _lib.load()
    d = _dims()
    need = lib.g2k_joint_eval_workspace_bytes(ctypes.byref(d))
    assert need == 2 * 20 * 8 * 10 * 4                  # a row [10] per (scene, frame, slice of draws)
    assert _call(lib, d, ws_bytes=need - 4) == -1 and b"workspace" in lib.g2k_last_error()
    assert _call(lib, d, ws=None) == -1 and b"workspace" in lib.g2k_last_error()
    assert _call(lib, _dims(S=0), ws_bytes=0) == 0      # nothing to run
    assert _call(lib, _dims(S=0), ws=None, ws_bytes=0) == 0
    assert lib.g2k_joint_eval_workspace_bytes(ctypes.byref(_dims(S=-1))) == -1
    # many scene-frames: one unit each
    assert lib.g2k_joint_eval_workspace_bytes(ctypes.byref(_dims(S=256))) == 256 * 20 * 10 * 4


def test_flag_defaults_off():
    from multimodaltraj_2_amd.argParser import ArgsParser
    a = ArgsParser().parser.parse_args([])
    assert a.collision_radius == 0.0 and isinstance(a.collision_radius, float)
    a = ArgsParser().parser.parse_args(["--num_samples", "20", "--collision_radius", "0.25"])
    assert a.collision_radius == 0.25 and a.num_samples == 20


def test_python_binding_rejects_radius():
    import torch
    from multimodaltraj_2_amd.nll import GaussianHead
    gh = GaussianHead(device="cpu")
    z = torch.zeros((1, 1, 24, 4))
    for r in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError, match="radius"):
            gh.joint_eval(z, torch.zeros((1, 1, 4, 12, 2)), torch.ones(1, dtype=torch.int32), 2, r)


def _case(seed=0, S=3, F=2, N=9, sigma=0.3):
    rng = np.random.default_rng(seed)
    pred = rng.standard_normal((S, F, 24, N)).astype(np.float32)
    tg = (pred.reshape(S, F, 2, 12, N).transpose(0, 1, 4, 3, 2)
          + sigma * rng.standard_normal((S, F, N, 12, 2))).astype(np.float32)
    head = np.stack([np.log(sigma) + 0.2 * rng.standard_normal(12),
                     np.log(sigma) + 0.2 * rng.standard_normal(12),
                     0.5 * rng.standard_normal(12)]).astype(np.float32)
    pm = (rng.random((S, N)) > 0.2).astype(np.uint8)
    return pred, tg, head, np.array([0, 5, N], np.int32)[:S], np.array([F, 1, F], np.int32)[:S], pm


SEED = (7 << 32) + 99


def test_checker_one_draw_is_the_marginal_sum():
    """K = 1: P * minJADE == the sum of the pairs' minADE of best_of_k_ref."""
    pred, tg, head, nact, nfr, pm = _case()
    J = joint_eval_ref(pred, tg, nact, head, SEED, 1, 0.3, nfr, pm)
    M = best_of_k_ref(pred, tg, nact, head, SEED, 1, nfr, pm)
    Pn = J["per_frame_i"][..., 0]
    np.testing.assert_array_equal(Pn, M["pairs"].sum(axis=2))
    np.testing.assert_allclose(Pn * J["per_frame_f"][..., 0], M["per_ped"][..., 0].sum(axis=2),
                               rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(Pn * J["per_frame_f"][..., 1], M["per_ped"][..., 1].sum(axis=2),
                               rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(J["sums_f"][:, 0], M["out"][:, 0], rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(J["sums_i"][:, 0], M["out"][:, 2])
    assert np.all(J["per_frame_f"][..., 2:] == 0) and np.all(J["sums_f"][:, 2] == 1)
    np.testing.assert_array_equal(J["per_frame_i"][..., 4], J["per_frame_i"][..., 5])   # the one draw


def test_checker_joint_is_not_below_marginal():
    pred, tg, head, nact, nfr, pm = _case(seed=1)
    J = joint_eval_ref(pred, tg, nact, head, SEED, 20, 0.3, nfr, pm)
    M = best_of_k_ref(pred, tg, nact, head, SEED, 20, nfr, pm)
    Pn = J["per_frame_i"][..., 0]
    for c in (0, 1):
        marg = M["per_ped"][..., c].sum(axis=2)
        assert np.all(Pn * J["per_frame_f"][..., c] >= marg - 1e-12)
        assert np.any(Pn * J["per_frame_f"][..., c] > marg + 1e-6)        # and really differs
    assert Pn[0].sum() == 0 and np.all(J["per_frame_f"][0] == 0) and np.all(J["per_frame_i"][0] == 0)
    assert np.all(J["per_frame_i"][1, 1] == 0)                            # f >= n_frames
    np.testing.assert_array_equal(J["per_frame_i"][..., 1], Pn * (Pn - 1) // 2)
    assert np.all(J["col_lo"] <= J["col_k"]) and np.all(J["col_k"] <= J["col_hi"])
    assert J["col_k"].sum() > 0


def test_checker_nested_draws():
    pred, tg, head, nact, nfr, pm = _case(seed=2)
    a = joint_eval_ref(pred, tg, nact, head, SEED, 10, 0.3, nfr, pm)
    b = joint_eval_ref(pred, tg, nact, head, SEED, 20, 0.3, nfr, pm)
    np.testing.assert_array_equal(b["jade_k"][:10], a["jade_k"])
    np.testing.assert_array_equal(b["col_k"][:10], a["col_k"])
    assert np.all(b["per_frame_f"][..., :2] <= a["per_frame_f"][..., :2])
    assert np.all(b["per_frame_i"][..., 4] >= a["per_frame_i"][..., 4])
    for k in (2, 3):                                    # mean / targets columns do not depend on K
        np.testing.assert_array_equal(b["per_frame_i"][..., k], a["per_frame_i"][..., k])
    # the seed wraps: draw 2 of seed 2^64 - 2 is draw 0 of seed 0
    w = joint_eval_ref(pred, tg, nact, head, (1 << 64) - 2, 3, 0.3, nfr, pm)
    z = joint_eval_ref(pred, tg, nact, head, 0, 1, 0.3, nfr, pm)
    np.testing.assert_array_equal(w["jade_k"][2], z["jade_k"][0])


def test_checker_radius_zero_counts_nothing():
    pred, tg, head, nact, nfr, pm = _case(seed=2)
    J = joint_eval_ref(pred, tg, nact, head, SEED, 3, 0.0, nfr, pm)
    assert np.all(J["per_frame_i"][..., 2:] == 0) and np.all(J["col_lo"] == 0)


def test_checker_structured_couples():
    """Couples 0.05 apart, >= 1.0 from each other, sigma 1e-3, radius 0.1:
    every draw, the mean and the targets collide in exactly the intact
    couples, and nothing is within eps of the threshold."""
    c, intact = couples_case()
    assert intact.tolist() == [[8, 8], [6, 6], [5, 0]]                  # counted by hand
    K = 6
    J = joint_eval_ref(c["pred"], c["targets"], c["n_active"], c["head"], SEED, K, c["radius"],
                       c["n_frames"], c["ped_mask"])
    for k in range(K):
        np.testing.assert_array_equal(J["col_k"][k], intact)
    np.testing.assert_array_equal(J["col_lo"], J["col_hi"])
    np.testing.assert_array_equal(J["pred_lo"], J["pred_hi"])
    np.testing.assert_array_equal(J["gt_lo"], J["gt_hi"])
    assert J["amb_k"].sum() == 0 and J["amb_pred"].sum() == 0 and J["amb_gt"].sum() == 0
    pi = J["per_frame_i"]
    np.testing.assert_array_equal(pi[..., 2], intact)
    np.testing.assert_array_equal(pi[..., 3], intact)
    np.testing.assert_array_equal(pi[..., 4], K * intact)
    np.testing.assert_array_equal(pi[..., 5], intact)
    np.testing.assert_array_equal(J["sums_i"][:, 4], K * intact.sum(axis=1))
