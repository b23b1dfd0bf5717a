"""CPU: the KDE-NLL's definition and plumbing (g2k_kde_nll_f32 /
g2k_fullcov_kde_nll_f32, csrc/g2k_kde.hip; tests/kde_ref.py is the float64
checker).  PARITY UNPINNED against the reference (it has no probabilistic
head); the definition is pinned against scipy.stats.gaussian_kde, which is what
Trajectron++ calls.  The GPU gate (kde_ref.GATE) is measured here, from the
checker's restated-precision mode over the GPU cases' exact inputs with the
oracle's draws — never from the kernel's output."""
import ctypes

import numpy as np
import pytest

from multimodaltraj_2_amd import _lib
from tests import kde_cases as kc
from tests import kde_ref as kr

_P = 16                        # a non-NULL pointer, 16-byte aligned (never dereferenced)
_EINVAL, _EUNSUPPORTED = -1, -4
ENTRY = [("g2k_kde_nll_f32", b"kde_nll"), ("g2k_fullcov_kde_nll_f32", b"fullcov_kde_nll")]


@pytest.mark.parametrize("K", [4, 5, 20, 64, 200])
def test_checker_is_scipys_gaussian_kde(K):
    """Pins the divisor K - 1, Scott's exponent and the normaliser."""
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(K)
    worst = 0.0
    for trial in range(8):
        A = rng.standard_normal((2, 2)) * rng.uniform(0.1, 1.5)
        x = rng.standard_normal((K, 2)) @ A.T + rng.standard_normal(2)
        y = x.mean(axis=0) + (rng.standard_normal((5, 2)) * (1 + trial)) @ A.T
        want = stats.gaussian_kde(x.T).logpdf(y.T)
        got, ok = kr.kde_logp(x[:, None, :], y)
        assert ok.all()
        worst = max(worst, float(np.max(np.abs(got - want) / np.abs(want))))
    print(f"K {K}: checker vs scipy.stats.gaussian_kde, worst relative difference {worst:.3g}")
    assert worst <= 1e-9


@pytest.mark.parametrize("restated", [False, True])
def test_clip_and_singular_rule(restated):
    """All points equal and points on a line: det H is not positive, every
    step sits on the floor and counts as clipped; a far target clips, a near
    one does not, and the floor is the term."""
    K, S, F, N = 6, 1, 1, 3
    rng = np.random.default_rng(3)
    draws = np.zeros((K, S, F, 24, N), np.float32)
    draws[..., 0] = 1.5                                                   # n 0: all points equal
    tline = np.arange(K, dtype=np.float32)[:, None, None, None] * 0.25     # n 1: y = 2 x - 0.5, exactly
    draws[:, :, :, :12, 1] = tline
    draws[:, :, :, 12:, 1] = 2 * tline - 0.5
    draws[..., 2] = rng.standard_normal((K, S, F, 24)).astype(np.float32)  # n 2: a proper cloud
    pred = np.zeros((S, F, 24, N), np.float32)
    targets = np.zeros((S, F, N, 12, 2), np.float32)
    targets[0, 0, 2, 6:] = 40.0                                           # n 2: steps 6.. far away
    pairs = np.ones((S, F, N), bool)
    R = kr.kde_nll_ref(draws, targets, pairs, -20.0, pred=pred, restated=restated)
    per = R["per_ped"][0, 0]
    for n in (0, 1):
        assert np.all(R["logp"][0, 0, n] == -np.inf) and np.all(R["clip"][0, 0, n])
        assert per[n].tolist() == [20.0, 20.0, 12.0, 0.0]
    assert not R["clip"][0, 0, 2, :6].any() and R["clip"][0, 0, 2, 6:].all()
    assert np.all(R["term"][0, 0, 2, 6:] == -20.0) and np.all(R["term"][0, 0, 2, :6] > -20.0)
    assert per[2, 1] == 20.0 and per[2, 2] == 6.0
    np.testing.assert_allclose(per[2, 0], -R["term"][0, 0, 2].mean(), rtol=1e-15)
    assert R["out"][0].tolist()[2:] == [3.0, 30.0, 6.0, -20.0, 0.0, 0.0]
    # a floor below every density: nothing clips but the singular steps
    R2 = kr.kde_nll_ref(draws, targets, pairs, -1e30, pred=pred, restated=restated)
    assert R2["per_ped"][0, 0, 2, 2] == 0 and R2["per_ped"][0, 0, 0, 2] == 12
    with pytest.raises(ValueError):
        kr.kde_nll_ref(draws[:3], targets, pairs)


def _dims(**kw):
    d = dict(S=2, F=20, T=8, L=12, D=16, H=128, Nmax=32, W=27, stride=1)
    d.update(kw)
    return _lib.G2KDims(**d)


def _call(lib, fn, d, **kw):
    a = dict(pred=_P, targets=_P, n_active=_P, n_frames=None, ped_mask=None, head=_P, seed=7, K=20,
             log_floor=-20.0, per_ped=_P, out=_P, ws=_P, ws_bytes=2 * 20 * 32, stream=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    rc = getattr(lib, fn)(ctypes.byref(d) if d is not None else None, a["pred"], a["targets"],
                          a["n_active"], a["n_frames"], a["ped_mask"], a["head"], a["seed"], a["K"],
                          a["log_floor"], a["per_ped"], a["out"], a["ws"], a["ws_bytes"], a["stream"])
    return rc, (lib.g2k_last_error() or b"")


@pytest.mark.parametrize("fn,short", ENTRY)
def test_entry_points_validate(fn, short):
    """Without a GPU: every rejection happens before any launch, in the
    best-of-K entry points' order (dims, flags, sizes, K, the scalar, NULLs,
    alignment, workspace); S = 0 and F = 0 return 0 and launch nothing."""
    lib = _lib.load()
    d = _dims()

    def rejects(code, word, dims, **kw):
        rc, msg = _call(lib, fn, dims, **kw)
        assert rc == code and word in msg, (fn, kw, rc, msg)

    rejects(_EINVAL, b"dims is NULL", None)
    rejects(_EUNSUPPORTED, short + b" reads pred_path_band", _dims(flags=_lib.STEP_PRED_PED_MAJOR))
    for bad, word in ((dict(Nmax=0), b"Nmax=0"), (dict(Nmax=257), b"Nmax=257"), (dict(S=-1), b"S=-1"),
                      (dict(F=-1), b"F=-1")):
        rejects(_EINVAL, word, _dims(**bad))
    for K in (3, 0, -1, 4097):
        rejects(_EINVAL, b"K=%d (4..4096)" % K, d, K=K)
    for v in (float("nan"), float("inf"), float("-inf")):
        rejects(_EINVAL, b"log_floor=", d, log_floor=v)
    rejects(_EINVAL, b"K=3 ", d, K=3, log_floor=float("nan"))            # K before the floor
    rejects(_EINVAL, b"log_floor=", d, log_floor=float("nan"), pred=None)  # the floor before the pointers
    for name in ("pred", "targets", "n_active", "head", "out"):
        rejects(_EINVAL, b"required buffer pointer is NULL", d, **{name: None})
    rejects(_EINVAL, b"required buffer", d, pred=None, targets=20)         # NULLs before alignment
    rejects(_EINVAL, b"targets must be 8-byte aligned", d, targets=20)
    rejects(_EINVAL, b"per_ped must be 16-byte aligned", d, per_ped=24)
    rejects(_EINVAL, b"per_ped", d, per_ped=24, ws=None)                   # alignment before the workspace
    need = 2 * 20 * 32
    rejects(_EINVAL, b"workspace of %d bytes needed (got %d)" % (need, need), d, ws=None)
    rejects(_EINVAL, b"workspace of %d bytes needed (got %d)" % (need, need - 4), d, ws_bytes=need - 4)
    # nothing to do: no launch, no workspace needed when S = 0; still validated
    assert _call(lib, fn, _dims(S=0), ws=None, ws_bytes=0)[0] == 0
    assert _call(lib, fn, _dims(F=0), ws_bytes=2 * 32)[0] == 0
    assert _call(lib, fn, _dims(S=0, F=0), ws=None, ws_bytes=0, per_ped=None)[0] == 0
    rejects(_EINVAL, b"K=3 ", _dims(S=0), K=3)
    rejects(_EINVAL, b"required buffer", _dims(F=0), head=None)
    rejects(_EINVAL, b"workspace of 64 bytes", _dims(F=0), ws_bytes=60)


def test_workspace_sizes():
    """S max(F, 1) 32 bytes: one row [8] per (scene, chunk), at most F chunks."""
    lib = _lib.load()
    for fn in ("g2k_kde_nll_workspace_bytes", "g2k_fullcov_kde_nll_workspace_bytes"):
        size = getattr(lib, fn)
        for S, F in [(2, 20), (1, 1), (3, 0), (0, 20), (256, 20), (7, 37)]:
            assert size(ctypes.byref(_dims(S=S, F=F))) == S * max(F, 1) * 32
        assert size(None) == -1
        assert size(ctypes.byref(_dims(S=-1))) == -1 and size(ctypes.byref(_dims(F=-1))) == -1


def test_flags_and_figures():
    from multimodaltraj_2_amd import evaluate
    from multimodaltraj_2_amd.argParser import ArgsParser
    args = ArgsParser().parser.parse_args([])
    assert args.kde_nll == 0 and args.kde_floor == -20.0
    args = ArgsParser().parser.parse_args(["--kde_nll", "1", "--kde_floor", "-12.5"])
    assert args.kde_nll == 1 and args.kde_floor == -12.5
    assert evaluate.KDE_FIGURES == ("kde_nll", "kde_nll_final", "kde_clipped")
    assert evaluate.FULLCOV_KDE_FIGURES == tuple("fullcov_" + k for k in evaluate.KDE_FIGURES)
    old = (evaluate.FIGURES + evaluate.JOINT_FIGURES + evaluate.CALIB_FIGURES + evaluate.FULLCOV_FIGURES
           + evaluate.FULLCOV_JOINT_FIGURES + ("scenes", "pairs", "K"))
    new = evaluate.KDE_FIGURES + evaluate.FULLCOV_KDE_FIGURES
    assert len(set(new)) == 6 and not set(new) & set(old)


def test_result_class():
    import torch
    from multimodaltraj_2_amd.nll import KdeNll
    out = torch.tensor([[6.0, 9.0, 3.0, 9.0, 20.0, -20.0, 0.0, 0.0],
                        [2.0, 1.0, 1.0, 3.0, 20.0, -20.0, 0.0, 0.0]])
    r = KdeNll(out=out, per_ped=None, k=20, log_floor=-20.0)
    assert r.pairs == 4 and r.kde_nll == 2.0 and r.kde_nll_final == 2.5
    assert r.clipped_share == 12.0 / (4 * 12)
    empty = KdeNll(out=torch.zeros((2, 8)), per_ped=None)
    assert empty.pairs == 0 and np.isnan(empty.kde_nll) and np.isnan(empty.clipped_share)


def test_gate_measurement():
    """The GPU gate: worst |restated precision - float64| of a clipped term and
    of a pair's kde_nll over the GPU cases' exact inputs with the oracle's
    draws, both heads; kde_ref.GATE is 8 x the recorded worst, and the record (to 10 %)
    is not below what is measured here."""
    worst_term = worst_pair = 0.0
    for i, name in enumerate(kc.IDS):
        c = kc.inputs(i)
        for which in kc.HEADS:
            draws = kc.oracle_draws(i, which)
            A = kr.kde_nll_ref(draws, c["targets"], c["pairs"], -20.0)
            B = kr.kde_nll_ref(draws, c["targets"], c["pairs"], -20.0, pred=c["pred"], restated=True)
            m = c["pairs"]
            dt = float(np.abs(A["term"][m] - B["term"][m]).max())
            dp = float(np.abs(A["per_ped"][..., :2] - B["per_ped"][..., :2]).max())
            assert np.isfinite(A["per_ped"]).all() and np.isfinite(B["per_ped"]).all()
            print(f"case {name} {which}: {int(m.sum())} pairs, worst |restated - float64| term "
                  f"{dt:.3g}, pair {dp:.3g}")
            worst_term, worst_pair = max(worst_term, dt), max(worst_pair, dp)
    print(f"worst term {worst_term:.3g}, worst pair {worst_pair:.3g}; recorded "
          f"{kr.MEASURED_WORST:.3g}, gate {kr.GATE:.3g}")
    assert kr.GATE == 8 * kr.MEASURED_WORST
    # 10 %: numpy's fp32 exp / log differ by an ulp between CPU dispatch paths
    assert max(worst_term, worst_pair) <= 1.1 * kr.MEASURED_WORST


def test_cases_stay_off_the_clip_boundary():
    """Steps whose float64 logp lies within the gate of the floor are left out
    of the GPU tests' exact clip counts: at most 1 % of a case's steps.  The
    "far" case clips a real share of its steps, the others next to none."""
    for i, name in enumerate(kc.IDS):
        c = kc.inputs(i)
        m = c["pairs"]
        for which in kc.HEADS:
            A = kr.kde_nll_ref(kc.oracle_draws(i, which), c["targets"], m, -20.0)
            near = np.abs(A["logp"][m] + 20.0) <= kr.GATE
            share = float(A["clip"][m].mean())
            print(f"case {name} {which}: {near.sum()} of {near.size} steps within the gate of the "
                  f"floor, clipped share {share:.4f}")
            assert near.mean() <= 0.01
            if name == "far":
                assert 0.05 <= share <= 0.95
