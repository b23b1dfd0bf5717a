"""CPU: the Gaussian-mixture trajectory head (include/g2k_mix.h,
multimodaltraj_2_amd/mixture.py) — the header, the module's binding table and
the library's exports agree; every validator rejects bad arguments before
touching the GPU; and the float64 checker tests/mixture_ref.py alone: it
reduces to tests/fullcov_ref.py with one slot, never draws from a dead slot,
its EM never loses more than 1e-4 nat per pair in a step and recovers two
modes, and ``MixtureHead.init_from`` is the definition's deterministic start.

EM data: 2400 residuals from two equal full-rank components N(+-4 L e, L L^T)
(e a unit vector: the means are 4 sigma apart from the centre in the whitened
direction e).  One Gaussian pays 1/2 ln det(I + 16 e e^T) = 1/2 ln 17 = 1.42
nat per pair for that direction, the mixture ln 2 = 0.69 (the label's entropy:
the modes do not overlap), so the fitted M = 2 NLL is below the M = 1 one by
0.72, asserted at 0.5.  The ridge C_ii (1 + 1e-6) makes an M-step inexact by
O(24e-6) per pair; the project's 1e-4 bounds a step's loss."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib, mixture
from tests import fullcov_ref as fr
from tests import mixture_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2k_mix.h")
_P = 16                        # a non-NULL pointer, 16-byte aligned (never dereferenced)
_EINVAL, _EUNSUPPORTED = -1, -4


def _declarations():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(g2k_[a-z0-9_]+)\s*\(([^)]*)\)", src)}


def _dims(**kw):
    d = dict(S=2, F=20, T=8, L=12, D=16, H=128, Nmax=32, W=27, stride=1)
    d.update(kw)
    return _lib.G2KDims(**d)


# ---------------------------------------------------------------------------
# the header, the binding and the exports
# ---------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    decl = _declarations()
    assert sorted(decl) == sorted(mixture.SYMBOLS)
    for name, args in decl.items():
        assert len(args.split(",")) == len(mixture.SYMBOLS[name][1]), name
    # by symbol, after ABI 11: not part of the versioned header or its table
    hip = open(os.path.join(ROOT, "include", "g2k_hip.h")).read()
    assert not set(decl) & set(_lib.SYMBOLS) and "g2k_mix_" not in hip
    lib = mixture.load()
    for name, (res, args) in mixture.SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.g2k_abi_version() == _lib.ABI_VERSION == 11
    assert mixture.load() is lib
    src = open(HEADER).read()
    assert int(re.search(r"G2K_MIX_SLOTS (\d+)", src).group(1)) == mixture.SLOTS == mr.SLOTS
    assert int(re.search(r"G2K_MIX_PITCH (\d+)", src).group(1)) == mixture.PITCH == mr.PITCH
    assert "Alignment (bytes) of g2k_mix_em_f32: targets 8, moments 8, resp 8, total 8," in src
    assert "Alignment (bytes) of g2k_mix_best_of_k_f32: targets 8, per_ped 16," in src


class _Call:
    def __init__(self, lib, fn, order, **defaults):
        self.lib, self.fn, self.order, self.defaults = lib, getattr(lib, fn), order, defaults

    def rc(self, d, **kw):
        a = dict(self.defaults)
        assert set(kw) <= set(a), kw
        a.update(kw)
        return self.fn(ctypes.byref(d) if d is not None else None, *[a[n] for n in self.order])

    def rejects(self, code, word, d, **kw):
        rc = self.rc(d, **kw)
        msg = self.lib.g2k_last_error() or b""
        assert rc == code and word in msg, (kw, rc, msg)


_EM = ("pred", "targets", "n_active", "n_frames", "ped_mask", "mix_in", "moments", "resp", "total",
       "mix_out", "ws", "ws_bytes", "stream")


def _em_ws(S, F, N):
    """The documented workspace: gamma [8][slots] f64, then per workgroup a
    row [10] and 8 rows [448]; W = ceil(slots / 512) in 1..256."""
    slots = S * F * N
    W = min(256, max(1, -(-slots // 512)))
    return 8 * (8 * slots + W * (10 + 8 * 448)), W


def test_em_entry_point_validates():
    lib = mixture.load()
    size = lib.g2k_mix_em_workspace_bytes
    d = _dims()
    need = size(ctypes.byref(d))
    assert need == _em_ws(2, 20, 32)[0] and _em_ws(2, 20, 32)[1] == 3
    assert size(ctypes.byref(_dims(S=1, F=1))) == _em_ws(1, 1, 32)[0] and _em_ws(1, 1, 32)[1] == 1
    far = 1 << 20
    c = _Call(lib, "g2k_mix_em_f32", _EM, pred=_P, targets=_P, n_active=_P, n_frames=None,
              ped_mask=None, mix_in=_P, moments=_P, resp=_P, total=_P, mix_out=far, ws=_P,
              ws_bytes=need, stream=None)
    c.rejects(_EINVAL, b"dims is NULL", None)
    c.rejects(_EUNSUPPORTED, b"mix_em reads pred_path_band", _dims(flags=_lib.STEP_PRED_PED_MAJOR))
    for bad in (dict(Nmax=0), dict(Nmax=257), dict(S=-1), dict(F=-1), dict(S=1 << 16, F=1 << 15),
                dict(S=1 << 13, F=1 << 13, Nmax=32)):
        c.rejects(_EINVAL, b"S F Nmax < 2^31", _dims(**bad))
        assert size(ctypes.byref(_dims(**bad))) == -1
    assert size(None) == -1
    for name in ("pred", "targets", "n_active", "mix_in", "moments", "resp", "total"):
        c.rejects(_EINVAL, name.encode() + b" is NULL", d, **{name: None})
    c.rejects(_EINVAL, b"pred is NULL", d, pred=None, targets=20)          # NULLs before alignment
    c.rejects(_EINVAL, b"targets must be 8-byte aligned", d, targets=20)
    for name in ("moments", "resp", "total"):
        c.rejects(_EINVAL, b"moments, resp and total must be 8-byte aligned", d, **{name: 20})
    c.rejects(_EINVAL, b"4-byte aligned", d, mix_in=18)
    c.rejects(_EINVAL, b"4-byte aligned", d, mix_out=far + 2)
    # mix_out must not overlap mix_in: equal, and either end inside the other
    block = 8 * 608 * 4
    for out in (far, far + 4, far + block - 4, far - block + 4):
        c.rejects(_EINVAL, b"mix_out must not overlap mix_in", d, mix_in=far, mix_out=out)
    assert c.rc(_dims(S=0), mix_in=far, mix_out=far + block) == 0          # adjacent: fine
    assert c.rc(_dims(S=0), mix_in=far, mix_out=far - block) == 0
    c.rejects(_EINVAL, b"workspace must be 8-byte aligned", d, ws=20)
    c.rejects(_EINVAL, b"workspace of %d bytes needed (got %d), 8-byte aligned" % (need, need), d,
              ws=None)
    c.rejects(_EINVAL, b"workspace of %d bytes needed (got %d), 8-byte aligned" % (need, need - 8), d,
              ws_bytes=need - 8)
    c.rejects(_EINVAL, b"overlap", d, mix_in=far, ws=None)                 # before the workspace
    # no scene: nothing to do (validated all the same), with or without mix_out
    assert c.rc(_dims(S=0), ws=None, ws_bytes=0) == 0
    assert c.rc(_dims(S=0, T=9, L=10, D=3, H=5), ws=None, ws_bytes=0, mix_out=None) == 0
    c.rejects(_EINVAL, b"resp is NULL", _dims(S=0), resp=None)


def test_sampler_entry_point_validates():
    lib = mixture.load()
    c = _Call(lib, "g2k_mix_sample_f32", ("pred", "mix", "seed", "out", "comp", "stream"), pred=_P,
              mix=_P, seed=3, out=_P, comp=None, stream=None)
    c.rejects(_EINVAL, b"dims is NULL", None)
    c.rejects(_EUNSUPPORTED, b"flags must be 0", _dims(flags=_lib.STEP_PRED_PED_MAJOR))
    c.rejects(_EUNSUPPORTED, b"flags must be 0", _dims(flags=_lib.STEP_TARGETS_SHARED))
    c.rejects(_EUNSUPPORTED, b"T=9 L=12", _dims(T=9))
    c.rejects(_EINVAL, b"Nmax=0", _dims(Nmax=0))
    c.rejects(_EINVAL, b"Nmax=257", _dims(Nmax=257))
    c.rejects(_EINVAL, b"S=-1", _dims(S=-1))
    c.rejects(_EINVAL, b"required buffer pointer is NULL", _dims(), pred=None)
    c.rejects(_EINVAL, b"required buffer pointer is NULL", _dims(), mix=None)
    c.rejects(_EINVAL, b"out is NULL", _dims(), out=None)
    c.rejects(_EINVAL, b"out is NULL", _dims(S=0), out=None)
    assert c.rc(_dims(S=0)) == 0 and c.rc(_dims(F=0)) == 0 and c.rc(_dims(S=0), comp=_P) == 0


def test_best_of_k_entry_point_validates():
    lib = mixture.load()
    d = _dims()
    need = lib.g2k_mix_best_of_k_workspace_bytes(ctypes.byref(d))
    assert need == lib.g2k_fullcov_best_of_k_workspace_bytes(ctypes.byref(d)) == 2 * 20 * 32
    order = ("pred", "targets", "n_active", "n_frames", "ped_mask", "head", "seed", "K", "per_ped",
             "best", "out", "ws", "ws_bytes", "stream")
    c = _Call(lib, "g2k_mix_best_of_k_f32", order, pred=_P, targets=_P, n_active=_P, n_frames=None,
              ped_mask=None, head=_P, seed=7, K=20, per_ped=_P, best=None, out=_P, ws=_P,
              ws_bytes=need, stream=None)
    c.rejects(_EINVAL, b"dims is NULL", None)
    c.rejects(_EUNSUPPORTED, b"mix_best_of_k reads pred_path_band", _dims(flags=_lib.STEP_PRED_PED_MAJOR))
    c.rejects(_EINVAL, b"Nmax=257", _dims(Nmax=257))
    c.rejects(_EINVAL, b"S=-1", _dims(S=-1))
    c.rejects(_EINVAL, b"K=0 ", d, K=0)
    c.rejects(_EINVAL, b"K=4097 ", d, K=4097)
    for name in ("pred", "targets", "n_active", "head", "out"):
        c.rejects(_EINVAL, b"required buffer pointer is NULL", d, **{name: None})
    c.rejects(_EINVAL, b"targets must be 8-byte aligned", d, targets=20)
    c.rejects(_EINVAL, b"per_ped must be 16-byte aligned", d, per_ped=24)
    c.rejects(_EINVAL, b"workspace of %d bytes needed (got %d)" % (need, need), d, ws=None)
    c.rejects(_EINVAL, b"workspace of %d bytes needed (got %d)" % (need, need - 4), d,
              ws_bytes=need - 4)
    assert c.rc(_dims(S=0), ws=None, ws_bytes=0) == 0
    assert lib.g2k_mix_best_of_k_workspace_bytes(None) == -1


def test_module_rejects_bad_arguments_on_the_host():
    with pytest.raises(ValueError, match="components = 0"):
        mixture.MixtureHead(components=0, device="cpu")
    with pytest.raises(ValueError, match="components = 9"):
        mixture.MixtureHead(components=9, device="cpu")
    h = mixture.MixtureHead(components=3, device="cpu")
    assert tuple(h.params.shape) == (8, 608) and h.components == 3
    assert h.weights.tolist() == [np.float32(1 / 3)] * 3 + [0.0] * 5
    assert tuple(h.means.shape) == (8, 24) and tuple(h.chols.shape) == (8, 24, 24)
    assert torch.equal(h.chols[2], torch.eye(24)) and not bool(h.chols[3].any())
    with pytest.raises(ValueError, match=r"params must be \[8, 608\]"):
        mixture.MixtureHead.from_block(np.zeros((8, 600)), device="cpu")


# ---------------------------------------------------------------------------
# the checker alone
# ---------------------------------------------------------------------------
def _factor(rng, scale=0.05):
    Lm = np.zeros((24, 24))
    for i in range(24):
        for j in range(i + 1):
            Lm[i, j] = scale * (1.0 if i == j else 0.6 ** ((i - j + 1) // 2)) * (0.5 + rng.random())
    return Lm


def test_one_slot_mixture_is_the_full_covariance_head():
    rng = np.random.default_rng(11)
    Lm = _factor(rng).astype(np.float32)
    up = Lm.copy()
    up[np.triu_indices(24, 1)] = np.nan
    for slot in (0, 5):                                    # the live slot need not be the first
        mix = np.full((8, 608), np.nan, np.float32)        # dead slots hold NaN: never read
        mix[:, 0] = 0
        mix[slot, 0] = 0.7                                 # any weight: w / sum w = 1
        mix[slot, 8:32] = 0
        mix[slot, 32:] = up.reshape(-1)
        S, F, N = 2, 3, 7
        pred = rng.standard_normal((S, F, 24, N)).astype(np.float32)
        tg = rng.standard_normal((S, F, N, 12, 2)).astype(np.float32)
        nact = np.array([7, 4], np.int32)
        r = fr.residuals(pred, tg, nact)
        e = mr.em_step(r, mix)
        R = fr.stats_ref(pred, tg, nact, chol=up)
        assert e["total"][0] == R["pairs"] == 33
        assert abs(-e["total"][1] - R["stats"][:, 1].sum()) <= 1e-9 * abs(R["stats"][:, 1].sum())
        assert np.all(e["gamma"][:, slot] == 1.0) and np.all(e["hard"] == slot)
        np.testing.assert_allclose(e["moments"][slot], R["moments"], rtol=1e-13, atol=1e-13)
        assert e["resp"][slot].tolist() == [33.0, 33.0]
        for seed in (0, (1 << 64) - 1):
            x, comp = mr.sample(pred, mix, seed)
            assert np.all(comp == slot)
            np.testing.assert_array_equal(x, fr.sample(pred, up, seed))


def test_dead_slots_are_never_drawn_and_weights_are_met():
    """Weights (0.5, 0, 0.3, 0, 0, 0.2, 0, 0): the cumulative weights are
    forced to 1 at the last live slot, dead slots never appear, and the counts
    of 4096 trajectories are within 5 sigma of the binomial means."""
    mix = mr.block([0.5, 0, 0.3, 0, 0, 0.2, 0, 0])
    cw = mr.cum_weights(mix)
    assert cw.dtype == np.float32 and cw[5] == 1.0 and cw[0] == 0.5 and cw[1] == 0.5
    assert cw[2] == cw[3] == cw[4] == np.float32(0.8)
    shape = (4, 8, 24, 128)
    n = 4 * 8 * 128
    seen = np.zeros(8)
    for seed in (0, 1, (3 << 32) + 5):
        comp = mr.components(shape, mix, seed)
        assert set(np.unique(comp)) <= {0, 2, 5}
        cnt = np.bincount(comp.reshape(-1), minlength=8)
        for m, w in ((0, 0.5), (2, 0.3), (5, 0.2)):
            assert abs(cnt[m] - n * w) <= 5 * np.sqrt(n * w * (1 - w)), (seed, m, cnt)
        seen += cnt
    u = mr.selector_u(shape, 0)
    assert u.dtype == np.float32 and 0 < u.min() and u.max() <= 1.0
    # another seed, another assignment; the same seed, the same
    assert not np.array_equal(mr.components(shape, mix, 0), mr.components(shape, mix, 1))
    np.testing.assert_array_equal(mr.components(shape, mix, 7), mr.components(shape, mix, 7))


@functools.lru_cache(maxsize=None)
def _two_modes():
    rng = np.random.default_rng(2024)
    Lk = _factor(rng)
    e = rng.standard_normal(24)
    e /= np.linalg.norm(e)
    n = 2400
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    r = rng.standard_normal((n, 24)) @ Lk.T + 4.0 * sign[:, None] * (Lk @ e)[None]
    M = r.T @ r
    fit = fr.fit_from_moments(M, n).astype(np.float32)
    return r, M / n, fit


@functools.lru_cache(maxsize=None)
def _em_trace(M, iters=30):
    r, C, fit = _two_modes()
    mix = mr.init_from(C, fit, M)
    trace = []
    for _ in range(iters):
        e = mr.em_step(r, mix)
        trace.append(e["total"][1] / e["total"][0])
        mix = e["mix_out"]
    last = mr.em_step(r, mix)
    trace.append(last["total"][1] / last["total"][0])
    return np.array(trace), mix, last


def test_em_never_loses_more_than_the_ridge_allows():
    trace, mix, last = _em_trace(2)
    steps = np.diff(trace)
    print(f"log-likelihood per pair: {trace[0]:.6f} -> {trace[-1]:.6f}; smallest step {steps.min():.3g}")
    assert np.all(np.isfinite(trace)) and steps.min() >= -1e-4
    assert trace[-1] > trace[0]
    assert mr.live(mix).tolist() == [True, True] + [False] * 6


def test_em_recovers_the_two_modes():
    t1, _, _ = _em_trace(1)
    t2, mix, last = _em_trace(2)
    print(f"NLL per pair: M = 1 {-t1[-1]:.6f}, M = 2 {-t2[-1]:.6f}, gain {t2[-1] - t1[-1]:.6f} "
          f"(1/2 ln 17 - ln 2 = {0.5 * np.log(17) - np.log(2):.4f})")
    assert -t2[-1] <= -t1[-1] - 0.5
    w = mix[:2, 0]
    assert np.all(np.abs(w - 0.5) < 0.05), w
    assert np.all(np.abs(last["resp"][:2, 1] - 1200) <= 60)


def test_init_from_is_deterministic_and_the_definition():
    from multimodaltraj_2_amd.fullcov import FullCovStats
    r, C, fit = _two_modes()
    n = r.shape[0]
    mom = np.zeros((25, 24))
    mom[:24] = C * n
    mom[24] = r.sum(axis=0)
    stats = np.zeros((12, 4))
    stats[:, 0] = n
    st = FullCovStats(moments=torch.from_numpy(mom), stats=torch.from_numpy(stats), inside=None,
                      fit_chol=torch.from_numpy(fit), has_head=False)
    for M in (1, 2, 3, 8):
        a = mixture.MixtureHead.init_from(st, M, device="cpu")
        b = mixture.MixtureHead.init_from(st, M, device="cpu")
        assert torch.equal(a.params, b.params) and a.components == M
        want = mr.init_from(C, fit, M)
        got = a.params.numpy()
        np.testing.assert_array_equal(got[:, 0], want[:, 0])
        np.testing.assert_array_equal(got[:, 32:], want[:, 32:])
        np.testing.assert_array_equal(got[:, 1:8], 0)
        # the two quantile routines agree to a few ulp of float64: 1e-6 after the f32 rounding
        np.testing.assert_allclose(got[:, 8:32], want[:, 8:32], rtol=1e-6, atol=1e-9)
        np.testing.assert_array_equal(got[M:], 0)
    # the definition, spelled out for M = 3
    lam, vec = np.linalg.eigh(C)
    v = vec[:, -1] * np.sign(vec[np.argmax(np.abs(vec[:, -1])), -1])
    got = mixture.MixtureHead.init_from(st, 3, device="cpu").params.numpy()
    z = 0.96742156610170103955                             # the normal quantile of 5/6
    np.testing.assert_allclose(got[2, 8:32], z * np.sqrt(lam[-1]) * v, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(got[0, 8:32], -got[2, 8:32], rtol=1e-6, atol=1e-9)
    assert np.all(got[1, 8:32] == 0) and v[np.argmax(np.abs(v))] > 0
    assert np.all(got[:3, 0] == np.float32(1 / 3))
    with pytest.raises(ValueError, match="components = 9"):
        mixture.MixtureHead.init_from(st, 9, device="cpu")


def test_gpu_em_cases_reach_their_branches():
    """The inputs of tests/test_mixture_gpu.py's EM cases "outliers", "starved"
    and "cap" meet the conditions under which they reach the branches they are
    for (the max-shifted logsumexp, the "too little mass" finish, the
    256-workgroup cap), and the selector blocks their edges: conditions on the
    checker alone, held here so that the CPU suite sees a case drift away."""
    from tests import test_mixture_gpu as tg
    tg.em_branch_preconditions(log=lambda s: None)
    tg.selector_edge_preconditions()
