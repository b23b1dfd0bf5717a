"""Best-of-K sampling evaluation, the parts that need no GPU: the C ABI
rejects bad arguments before touching a device (g2k_best_of_k_f32, ABI 10),
the three new flags default to off, and the float64 checker
(tests/bestk_ref.py) obeys the definition's own invariants."""
import ctypes

import numpy as np
import pytest

from multimodaltraj_2_amd import _lib
from oracle import g2k_ref as ref
from tests.bestk_ref import best_of_k_ref, draw_errors

P = ctypes.c_void_p(16)


def _dims(**kw):
    d = dict(S=2, F=20, T=8, L=12, D=16, H=128, Nmax=32, W=27, stride=1)
    d.update(kw)
    return _lib.G2KDims(**d)


def _call(lib, d, K=20, ws_bytes=1 << 30, **null):
    a = dict(pred=P, targets=P, n_active=P, head=P, out=P, ws=P)
    a.update(null)
    return lib.g2k_best_of_k_f32(ctypes.byref(d), a["pred"], a["targets"], a["n_active"], None, None,
                                 a["head"], ctypes.c_uint64(5), K, None, None, a["out"], a["ws"],
                                 ws_bytes, None)


@pytest.mark.parametrize("name", ["pred", "targets", "n_active", "head", "out"])
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


def test_abi_workspace_and_zero_scenes():
    lib = _lib.load()
    d = _dims()
    need = lib.g2k_best_of_k_workspace_bytes(ctypes.byref(d))
    assert need == 2 * 20 * 8 * 4                       # one row [8] per (scene, frame) at most
    assert _call(lib, d, ws_bytes=need - 4) == -1 and b"workspace" in lib.g2k_last_error()
    assert _call(lib, d, ws=None) == -1
    assert _call(lib, _dims(S=0), ws_bytes=0) == 0      # nothing to run
    assert lib.g2k_best_of_k_workspace_bytes(ctypes.byref(_dims(S=-1))) == -1


def test_flags_default_off():
    from multimodaltraj_2_amd.argParser import ArgsParser
    a = ArgsParser().parser.parse_args([])
    assert (a.num_samples, a.sample_seed, a.head_log_sigma) == (0, 0, 0.0)
    a = ArgsParser().parser.parse_args(["--num_samples", "20", "--sample_seed", "7",
                                        "--head_log_sigma", "-1.5"])
    assert (a.num_samples, a.sample_seed, a.head_log_sigma) == (20, 7, -1.5)


def _case(seed=0, S=3, F=2, N=9, sigma=0.3):
    rng = np.random.default_rng(seed)
    pred = rng.standard_normal((S, F, 24, N)).astype(np.float32)
    tg = (pred.reshape(S, F, 2, 12, N).transpose(0, 1, 4, 3, 2)
          + sigma * rng.standard_normal((S, F, N, 12, 2))).astype(np.float32)
    head = np.stack([np.log(sigma) + 0.2 * rng.standard_normal(12),
                     np.log(sigma) + 0.2 * rng.standard_normal(12),
                     0.5 * rng.standard_normal(12)]).astype(np.float32)
    return pred, tg, head, np.array([0, 5, N], np.int32)[:S]


def test_checker_nested_draws():
    """The first 10 draws of K = 20 are the draws of K = 10 (same seed)."""
    pred, tg, head, nact = _case()
    seed = (7 << 32) + 99
    r10 = best_of_k_ref(pred, tg, nact, head, seed, 10)
    r20 = best_of_k_ref(pred, tg, nact, head, seed, 20)
    assert r20["pairs"].sum() == 2 * (5 + 9)
    assert np.all(r20["per_ped"][..., 0] <= r10["per_ped"][..., 0])
    assert np.all(r20["per_ped"][..., 1] <= r10["per_ped"][..., 1])
    assert np.all(r20["per_ped"][~r20["pairs"]] == 0)
    assert np.all(r20["out"][:, 5] == 20) and r20["out"][0, :5].tolist() == [0] * 5


def test_checker_one_draw_is_the_sampler():
    pred, tg, head, nact = _case(seed=3)
    seed = (1 << 64) - 2
    r = best_of_k_ref(pred, tg, nact, head, seed, 1)
    ade, fde = draw_errors(ref.gauss_sample(pred, head, seed), tg)
    m = r["pairs"]
    np.testing.assert_array_equal(r["per_ped"][..., 0][m], ade[m])
    np.testing.assert_array_equal(r["per_ped"][..., 1][m], fde[m])
    assert np.all(r["per_ped"][..., 2:] == 0)
    # the seed wraps: draw 2 of seed 2^64 - 2 is draw 0 of seed 0
    r3 = best_of_k_ref(pred, tg, nact, head, seed, 3)
    a0, _ = draw_errors(ref.gauss_sample(pred, head, 0), tg)
    np.testing.assert_array_equal(r3["ade_k"][2], a0)
