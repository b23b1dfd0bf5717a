"""CPU: the sample scores (include/g2k_scores.h, multimodaltraj_2_amd/scores.py,
csrc/g2k_scores.hip) — the header, the module's binding table and the
library's exports agree; every validator rejects bad arguments before touching
the GPU; the launch geometry is what tests/score_cases.py claims, every branch
of it reached; and the float64 checker tests/scores_ref.py alone: against plain
loops over the couples (and scipy.spatial.distance where it is importable), a
closed form at K = 2, a known answer on the oracle's draws, and the reason the
scores exist — the variogram score tells a full-covariance head from a
per-step head with the same marginals, the per-step energy score does not.

The known answer: for rho = 0 and sigma_x = sigma_y = sigma two independent
draws differ at a step by N(0, 2 sigma^2 I), whose length is Rayleigh with
scale sigma sqrt 2 and mean sigma sqrt pi: E[pF] = sigma_11 sqrt pi."""
import ctypes
import os
import re

import numpy as np

from multimodaltraj_2_amd import _lib, mixture, scores
from oracle import g2k_ref as ref
from tests import fullcov_ref
from tests import score_cases as sc
from tests import scores_ref as sr
from tests.bestk_ref import MASK64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2k_scores.h")
_P = 16                        # a non-NULL pointer, 16-byte aligned (never dereferenced)
_EINVAL, _EUNSUPPORTED = -1, -4
ENTRIES = ("g2k_sample_scores_f32", "g2k_fullcov_sample_scores_f32", "g2k_mix_sample_scores_f32")
L = 12


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
    assert sorted(decl) == sorted(scores.SYMBOLS)
    for name, args in decl.items():
        assert len(args.split(",")) == len(scores.SYMBOLS[name][1]), name
    # by symbol, after ABI 11: not part of the versioned header, the mixture's or their tables
    assert not set(decl) & set(_lib.SYMBOLS) and not set(decl) & set(mixture.SYMBOLS)
    for other in ("g2k_hip.h", "g2k_mix.h"):
        assert "sample_scores" not in open(os.path.join(ROOT, "include", other)).read()
    lib = scores.load()
    for name, (res, args) in scores.SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.g2k_abi_version() == _lib.ABI_VERSION == 11
    assert scores.load() is lib
    src = open(HEADER).read()
    assert int(re.search(r"G2K_SCORES_KMIN (\d+)", src).group(1)) == scores.KMIN == sr.K_MIN == 2
    assert int(re.search(r"G2K_SCORES_KMAX (\d+)", src).group(1)) == scores.KMAX == sr.K_MAX == 256
    assert int(re.search(r"G2K_SCORES_GEOM_FIELDS (\d+)", src).group(1)) == len(scores.GEOM_FIELDS)
    for i, f in enumerate(scores.GEOM_FIELDS):
        assert int(re.search(rf"G2K_SCORES_GEOM_{f.upper()} (\d+)", src).group(1)) == i
    assert ("Alignment (bytes) of g2k_sample_scores_f32, g2k_fullcov_sample_scores_f32\n"
            " * and g2k_mix_sample_scores_f32: targets 8, per_ped 16, workspace 4.") in src


# ---------------------------------------------------------------------------
# the validators: before any HIP call
# ---------------------------------------------------------------------------
_ORDER = ("pred", "targets", "n_active", "n_frames", "ped_mask", "head", "seed", "K", "per_ped", "out",
          "ws", "ws_bytes", "stream")


def _rc(lib, entry, d, **kw):
    a = dict(pred=_P, targets=_P, n_active=_P, n_frames=None, ped_mask=None, head=_P, seed=3, K=20,
             per_ped=None, out=_P, ws=_P, ws_bytes=1 << 30, stream=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    rc = getattr(lib, entry)(ctypes.byref(d) if d is not None else None, *[a[n] for n in _ORDER])
    return rc, lib.g2k_last_error() or b""


def _rejects(lib, entry, code, word, d, **kw):
    rc, msg = _rc(lib, entry, d, **kw)
    assert rc == code and word in msg, (entry, kw, rc, msg)


def test_entry_points_validate():
    lib = scores.load()
    size = lib.g2k_sample_scores_workspace_bytes
    d = _dims()
    need = size(ctypes.byref(d))
    assert need == 2 * 20 * 32                                 # one row [8] f32 per (scene, frame)
    assert size(ctypes.byref(_dims(F=0))) == 2 * 32 and size(ctypes.byref(_dims(S=0))) == 0
    assert size(None) == -1
    for bad in (dict(Nmax=0), dict(Nmax=257), dict(S=-1), dict(F=-1)):
        assert size(ctypes.byref(_dims(**bad))) == -1
    for e in ENTRIES:
        _rejects(lib, e, _EINVAL, b"dims is NULL", None)
        for flags in (_lib.STEP_PRED_PED_MAJOR, 4, 8, _lib.STEP_TARGETS_SHARED | 4, 1 << 8):
            _rejects(lib, e, _EUNSUPPORTED, b"0 or G2K_STEP_TARGETS_SHARED", _dims(flags=flags))
        for bad in (dict(Nmax=0), dict(Nmax=257), dict(S=-1), dict(F=-1)):
            _rejects(lib, e, _EINVAL, b"Nmax=", _dims(**bad))
        for k in (-1, 0, 1, 257, 4096):
            _rejects(lib, e, _EINVAL, b"K=%d (2..256)" % k, d, K=k)
        for name in ("pred", "targets", "n_active", "head", "out"):
            _rejects(lib, e, _EINVAL, b"a required buffer pointer is NULL", d, **{name: None})
        _rejects(lib, e, _EINVAL, b"targets must be 8-byte aligned", d, targets=20)
        _rejects(lib, e, _EINVAL, b"per_ped must be 16-byte aligned", d, per_ped=24)
        _rejects(lib, e, _EINVAL, b"workspace must be 4-byte aligned", d, ws=18)
        _rejects(lib, e, _EINVAL, b"workspace of %d bytes needed (got %d)" % (need, need - 4), d,
                 ws_bytes=need - 4)
        _rejects(lib, e, _EINVAL, b"workspace of %d bytes needed" % need, d, ws=None)
        # the weakest alignments the header states are accepted; no scene: nothing to do,
        # validated all the same
        none = _dims(S=0, flags=_lib.STEP_TARGETS_SHARED)
        assert _rc(lib, e, none, targets=24, per_ped=32, ws=20, ws_bytes=0, pred=20, head=20, out=20)[0] == 0
        assert _rc(lib, e, _dims(S=0), ws=None, ws_bytes=0, K=2)[0] == 0
        assert _rc(lib, e, _dims(S=0), ws=None, ws_bytes=0, K=256)[0] == 0
        _rejects(lib, e, _EINVAL, b"K=1 (2..256)", _dims(S=0), K=1)
        _rejects(lib, e, _EINVAL, b"NULL", _dims(S=0), out=None)
    out = (ctypes.c_int32 * 5)()
    geo = lib.g2k_sample_scores_geometry
    assert geo(None, 20, out) == _EINVAL and geo(ctypes.byref(d), 1, out) == _EINVAL
    assert geo(ctypes.byref(d), 257, out) == _EINVAL and geo(ctypes.byref(d), 20, None) == _EINVAL
    assert geo(ctypes.byref(_dims(Nmax=257)), 20, out) == _EINVAL
    assert geo(ctypes.byref(d), 20, out) == 0


# ---------------------------------------------------------------------------
# the geometry: what tests/score_cases.py claims, every branch reached
# ---------------------------------------------------------------------------
def test_geometry_claims_and_branches():
    reached = set()
    for i, case in enumerate(sc.CASES):
        name, S, F, N, K = case[:5]
        c = sc.inputs(i)
        g = scores.sample_scores_geometry(S, F, N, K)
        assert {k: g[k] for k in ("g", "fc", "c")} == c["geom"], (name, g)
        assert g["lanes"] == K and g["g"] * K <= 256
        assert sc.passes_of(i) == c["passes"], (name, sc.passes_of(i))
        # LDS: the draws [256][24], the lanes' sums [6][256], the items' rows [32][73], the
        # waves' rows [4][8]; with the mixture head's 19376 bytes below the 64 KB of a workgroup
        assert g["lds_bytes"] == 4 * (256 * 24 + 6 * 256 + 32 * 73 + 32) and g["lds_bytes"] + 19376 <= 65536
        reached.add("G capped" if 256 // K > 32 else "G = 256 // K")
        raw = 4 * g["g"] // N
        reached.add("FC cut by F" if raw > F else "FC raised to 1" if raw < 1 else "FC = 4 G // Nmax")
        reached.add("rows kernel" if g["c"] > 1 else "one workgroup per scene")
        reached.add("several passes" if c["passes"] > 1 else "one pass")
        if c["passes"] > 1 and (int(c["n_active"].max()) * g["fc"]) % g["g"]:
            reached.add("partial last group")
        if K % 2 == 0:
            reached.add("even K")
        else:
            reached.add("odd K")
        if K > 64:
            reached.add("pair past one wave")
        if 64 % K:
            reached.add("pair straddles waves")
        if g["fc"] > 1 and F % g["fc"]:
            reached.add("short last chunk")
        if any(int(n) == 0 for n in c["n_active"]):
            reached.add("empty scene")
    assert reached == {"G capped", "G = 256 // K", "FC cut by F", "FC raised to 1", "FC = 4 G // Nmax",
                       "rows kernel", "one workgroup per scene", "several passes", "one pass",
                       "partial last group", "even K", "odd K", "pair past one wave",
                       "pair straddles waves", "short last chunk", "empty scene"}, reached
    # the evaluation's two timing shapes (tools/time_sample_scores.py)
    assert scores.sample_scores_geometry(256, 20, 32, 20) == dict(
        g=12, lanes=20, fc=1, c=20, lds_bytes=40192)
    assert scores.sample_scores_geometry(128, 20, 256, 20)["c"] == 20
    # F = 0: one workgroup per scene, which writes the zeros
    assert scores.sample_scores_geometry(3, 0, 16, 20)["c"] == 1


# ---------------------------------------------------------------------------
# the checker against an independent restatement
# ---------------------------------------------------------------------------
def _loops(x, y):
    """x [K, L, 2], y [L, 2] -> the 7 columns by plain loops."""
    K = x.shape[0]
    a = lambda u, v: sum(float(np.hypot(*(u[t] - v[t]))) for t in range(L)) / L
    f = lambda u, v: float(np.hypot(*(u[L - 1] - v[L - 1])))
    r = lambda u, v: float(np.sqrt(sum(float(((u[t] - v[t]) ** 2).sum()) for t in range(L))))
    m = [sum(fn(x[k], y) for k in range(K)) / K for fn in (a, f, r)]
    nc = K * (K - 1) / 2
    p = [sum(fn(x[k], x[l]) for k in range(K) for l in range(k + 1, K)) / nc for fn in (a, f, r)]
    vs = 0.0
    for t in range(L):
        for u in range(t + 1, L):
            mean = sum(float(np.hypot(*(x[k, t] - x[k, u]))) ** 0.5 for k in range(K)) / K
            vs += (float(np.hypot(*(y[t] - y[u]))) ** 0.5 - mean) ** 2
    return m + p + [vs]


def test_checker_against_plain_loops():
    try:
        from scipy.spatial import distance
    except ImportError:
        distance = None
    worst = 0.0
    for name, which in (("k3", "per_step"), ("k20", "fullcov"), ("shared", "mix"), ("k2", "mix")):
        i = sc.IDS.index(name)
        c = sc.inputs(i)
        draws = sc.oracle_draws(i, which)
        R = sr.sample_scores_ref(draws, c["targets"], c["pairs"])
        x = sr.band_to_xy(draws).astype(np.float64)
        S, F, N = c["pairs"].shape
        y = np.broadcast_to(c["targets"].astype(np.float64), (S, F, N, L, 2))
        idx = np.argwhere(c["pairs"])
        for s, f, n in idx[:: max(1, len(idx) // 6)]:
            want = _loops(x[:, s, f, n], y[s, f, n])
            worst = max(worst, float(np.abs(R["per_ped"][s, f, n, :7] - want).max()))
            if distance is not None:
                flat = x[:, s, f, n].reshape(c["K"], 2 * L)
                pr = distance.pdist(flat).mean()
                mr_ = distance.cdist(flat, y[s, f, n].reshape(1, 2 * L)).mean()
                pf = distance.pdist(x[:, s, f, n, L - 1]).mean()
                worst = max(worst, abs(R["per_ped"][s, f, n, 5] - pr), abs(R["per_ped"][s, f, n, 2] - mr_),
                            abs(R["per_ped"][s, f, n, 4] - pf))
        assert np.all(R["per_ped"][~c["pairs"]] == 0) and np.all(R["per_ped"][..., 7] == 0)
        np.testing.assert_array_equal(R["out"][:, 7], c["pairs"].sum(axis=(1, 2)))
        np.testing.assert_allclose(R["out"][:, :7], R["per_ped"][..., :7].sum(axis=(1, 2)), atol=1e-12)
    print(f"checker vs plain loops{' and scipy' if distance is not None else ''}: worst {worst:.3g}")
    assert worst <= 1e-12


def test_closed_form_at_k2():
    i = sc.IDS.index("k2")
    c = sc.inputs(i)
    for which in sc.HEADS:
        draws = sc.oracle_draws(i, which)
        R = sr.sample_scores_ref(draws, c["targets"], c["pairs"])
        x = sr.band_to_xy(draws).astype(np.float64)
        y = c["targets"].astype(np.float64)
        m = c["pairs"]
        r0 = np.sqrt(((x[0] - y) ** 2).sum(axis=(-1, -2)))
        r1 = np.sqrt(((x[1] - y) ** 2).sum(axis=(-1, -2)))
        r01 = np.sqrt(((x[0] - x[1]) ** 2).sum(axis=(-1, -2)))
        es = sr.es_columns(R["per_ped"])[2]
        np.testing.assert_array_equal(es[m], (0.5 * (r0 + r1) - 0.5 * r01)[m])


def test_energy_scores_are_non_negative_on_every_case():
    for i in range(len(sc.CASES)):
        c = sc.inputs(i)
        for which in sc.HEADS:
            R = sr.sample_scores_ref(sc.oracle_draws(i, which), c["targets"], c["pairs"])
            assert np.isfinite(R["per_ped"]).all() and np.isfinite(R["out"]).all()
            for es in sr.es_columns(R["per_ped"]):
                assert es.min() >= 0.0, (sc.IDS[i], which, es.min())
            fig = sr.figures(R["out"])
            if c["pairs"].any():
                assert all(np.isfinite(v) for v in fig.values())


# ---------------------------------------------------------------------------
# a known answer, and what the scores are for
# ---------------------------------------------------------------------------
def test_known_answer_final_step_pairwise_distance():
    S, F, N, K, sigma = 4, 4, 32, 8, 0.6
    rng = np.random.default_rng(31)
    sig = rng.uniform(0.2, 1.2, L)
    sig[L - 1] = sigma
    head = np.stack([np.log(sig), np.log(sig), np.zeros(L)]).astype(np.float32)
    pred = rng.standard_normal((S, F, 2 * L, N)).astype(np.float32)
    draws = np.stack([ref.gauss_sample(pred, head, (77 + k) & MASK64) for k in range(K)]).astype(np.float32)
    tg = np.zeros((S, F, N, L, 2), np.float32)
    pairs = np.ones((S, F, N), bool)
    R = sr.sample_scores_ref(draws, tg, pairs)
    pf = R["per_ped"][..., 4].ravel()
    want = float(np.exp(head[0, L - 1])) * np.sqrt(np.pi)
    se = pf.std(ddof=1) / np.sqrt(pf.size)
    print(f"E[pF] = sigma sqrt(pi) = {want:.6f}; mean over {pf.size} pairs {pf.mean():.6f}, standard "
          f"error {se:.3g}: {abs(pf.mean() - want) / se:.2f} standard errors")
    assert abs(pf.mean() - want) <= 6 * se


PURPOSE_PAIRS = (8, 8, 32)      # S, F, N: 2048 pairs (see the test's docstring)


def test_variogram_score_sees_the_dependence_between_steps():
    """Targets from the AR(1) 0.7 full-covariance law around pred; the oracle's
    K = 20 draws of the per-step head with the same marginals and of the
    full-covariance head itself.  Per-pair differences (per-step minus
    full-covariance), mean / standard error over the 2048 pairs, measured on
    the CPU with the seeds below: vs +11.0 standard errors (asserted at 6),
    es_ade +0.09 (asserted: within 3, its noise), es_traj +5.3: the fair 24-D
    energy score does prefer the true joint law, but at this pair count not by
    the 6 standard errors asked for, so its sign is printed and not asserted
    (DESIGN.md §6j)."""
    S, F, N = PURPOSE_PAIRS
    K = 20
    rng = np.random.default_rng(2024)
    sx, sy = rng.uniform(0.1, 1.5, L), rng.uniform(0.1, 1.5, L)
    rho = rng.uniform(-0.9, 0.9, L)
    head = np.stack([np.log(sx), np.log(sy), np.arctanh(rho)]).astype(np.float32)
    B = fullcov_ref.block_factor(head)
    T = 0.7 ** np.abs(np.subtract.outer(np.arange(L), np.arange(L)))
    chol = np.linalg.cholesky(B @ np.kron(T, np.eye(2)) @ B.T).astype(np.float32)
    pred = rng.standard_normal((S, F, 2 * L, N)).astype(np.float32)
    mu = pred.reshape(S, F, 2, L, N).transpose(0, 1, 4, 3, 2)                  # [S, F, N, L, 2]
    z = rng.standard_normal((S, F, N, 2 * L))
    tg = (mu + (z @ chol.astype(np.float64).T).reshape(S, F, N, L, 2)).astype(np.float32)
    pairs = np.ones((S, F, N), bool)
    ps = np.stack([ref.gauss_sample(pred, head, (900 + k) & MASK64) for k in range(K)])
    fc = np.stack([fullcov_ref.sample(pred, chol, (900 + k) & MASK64) for k in range(K)])
    Rp = sr.sample_scores_ref(ps.astype(np.float32), tg, pairs)["per_ped"]
    Rf = sr.sample_scores_ref(fc.astype(np.float32), tg, pairs)["per_ped"]

    def margin(a, b):
        d = (a - b).ravel()
        return d.mean(), d.mean() / (d.std(ddof=1) / np.sqrt(d.size))
    ea_p, _, et_p = sr.es_columns(Rp)
    ea_f, _, et_f = sr.es_columns(Rf)
    vs = margin(Rp[..., 6], Rf[..., 6])
    ea = margin(ea_p, ea_f)
    et = margin(et_p, et_f)
    print(f"{pairs.sum()} pairs, K {K}; per-step minus full-covariance, mean (standard errors): "
          f"vs {vs[0]:.5g} ({vs[1]:.2f}), es_ade {ea[0]:.5g} ({ea[1]:.2f}), es_traj {et[0]:.5g} ({et[1]:.2f})")
    print(f"   vs {Rp[..., 6].mean():.5g} / {Rf[..., 6].mean():.5g}, es_ade {ea_p.mean():.5g} / "
          f"{ea_f.mean():.5g}, es_traj {et_p.mean():.5g} / {et_f.mean():.5g} (per-step / full-covariance)")
    assert vs[1] >= 6.0                       # the full-covariance head's vs is lower
    assert abs(ea[1]) < 3.0                   # the marginals are the same: es_ade cannot tell
    if et[1] >= 6.0:
        assert et[0] > 0
