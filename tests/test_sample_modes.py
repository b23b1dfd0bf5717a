"""CPU: the k-means reduction of the heads' samples (include/g2k_modes.h,
multimodaltraj_2_amd/modes.py, csrc/g2k_modes.hip) — the header, the module's
binding table and the library's exports agree; every validator rejects bad
arguments before touching the GPU; the launch geometry is what
tests/modes_cases.py claims, every branch of it reached; and the float64
checker tests/modes_ref.py alone: against plain loops, the closed forms of the
cases ``m1``, ``mk`` and ``collapsed``, tests/bestk_ref.py at iters = 0, the
descent of the inertia, the share of fragile pairs on the oracle's draws, and
the reason the reduction exists — the centres of 256 clustered draws are
closer to the target than the same number of raw draws."""
import ctypes
import os
import re

import numpy as np

from multimodaltraj_2_amd import _lib, mixture, modes, scores
from tests import bestk_ref
from tests import fullcov_ref
from tests import modes_cases as mc
from tests import modes_ref as mo
from tests.bestk_ref import MASK64, SEED_A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2k_modes.h")
_P = 16                        # a non-NULL pointer, 16-byte aligned (never dereferenced)
_EINVAL, _EUNSUPPORTED = -1, -4
ENTRIES = ("g2k_sample_modes_f32", "g2k_fullcov_sample_modes_f32", "g2k_mix_sample_modes_f32")
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
    assert sorted(decl) == sorted(modes.SYMBOLS)
    for name, args in decl.items():
        assert len(args.split(",")) == len(modes.SYMBOLS[name][1]), name
    # by symbol, after ABI 11: not part of the versioned header, the mixture's, the scores' or
    # their tables
    for other in (_lib.SYMBOLS, mixture.SYMBOLS, scores.SYMBOLS):
        assert not set(decl) & set(other)
    for other in ("g2k_hip.h", "g2k_mix.h", "g2k_scores.h"):
        assert "sample_modes" not in open(os.path.join(ROOT, "include", other)).read()
    lib = modes.load()
    for name, (res, args) in modes.SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.g2k_abi_version() == _lib.ABI_VERSION == 11
    assert modes.load() is lib
    src = open(HEADER).read()
    assert "PARITY\n * UNPINNED" in src or "PARITY UNPINNED" in src
    assert int(re.search(r"G2K_MODES_MMAX (\d+)", src).group(1)) == modes.MMAX == mo.M_MAX == 32
    assert int(re.search(r"G2K_MODES_KMAX (\d+)", src).group(1)) == modes.KMAX == mo.K_MAX == 256
    assert int(re.search(r"G2K_MODES_ITERS_MAX (\d+)", src).group(1)) == modes.ITERS_MAX == mo.ITERS_MAX == 64
    assert int(re.search(r"G2K_MODES_GEOM_FIELDS (\d+)", src).group(1)) == len(modes.GEOM_FIELDS)
    for i, f in enumerate(modes.GEOM_FIELDS):
        assert int(re.search(rf"G2K_MODES_GEOM_{f.upper()} (\d+)", src).group(1)) == i
    assert ("Alignment (bytes) of g2k_sample_modes_f32, g2k_fullcov_sample_modes_f32\n"
            " * and g2k_mix_sample_modes_f32: targets 8, per_ped 16, workspace 8.") in src


# ---------------------------------------------------------------------------
# the validators: before any HIP call
# ---------------------------------------------------------------------------
_ORDER = ("pred", "targets", "n_active", "n_frames", "ped_mask", "head", "seed", "K", "M", "iters",
          "radius", "per_ped", "centres", "weights", "out", "ws", "ws_bytes", "stream")


def _rc(lib, entry, d, **kw):
    a = dict(pred=_P, targets=_P, n_active=_P, n_frames=None, ped_mask=None, head=_P, seed=3, K=20, M=5,
             iters=10, radius=0.0, per_ped=None, centres=None, weights=None, out=_P, ws=_P,
             ws_bytes=1 << 30, stream=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    rc = getattr(lib, entry)(ctypes.byref(d) if d is not None else None, *[a[n] for n in _ORDER])
    return rc, lib.g2k_last_error() or b""


def _rejects(lib, entry, code, word, d, **kw):
    rc, msg = _rc(lib, entry, d, **kw)
    assert rc == code and word in msg, (entry, kw, rc, msg)


def test_entry_points_validate():
    lib = modes.load()
    size = lib.g2k_sample_modes_workspace_bytes
    d = _dims()
    need = size(ctypes.byref(d))
    assert need == 2 * 20 * 64                                 # one row [8] f64 per (scene, frame)
    assert size(ctypes.byref(_dims(F=0))) == 2 * 64 and size(ctypes.byref(_dims(S=0))) == 0
    assert size(None) == -1
    for bad in (dict(Nmax=0), dict(Nmax=257), dict(S=-1), dict(F=-1)):
        assert size(ctypes.byref(_dims(**bad))) == -1
    for e in ENTRIES:
        _rejects(lib, e, _EINVAL, b"dims is NULL", None)
        for flags in (_lib.STEP_PRED_PED_MAJOR, 4, 8, _lib.STEP_TARGETS_SHARED | 4, 1 << 8):
            _rejects(lib, e, _EUNSUPPORTED, b"0 or G2K_STEP_TARGETS_SHARED", _dims(flags=flags))
        for bad in (dict(Nmax=0), dict(Nmax=257), dict(S=-1), dict(F=-1)):
            _rejects(lib, e, _EINVAL, b"Nmax=", _dims(**bad))
        for m in (-1, 0, 33, 4096):
            _rejects(lib, e, _EINVAL, b"M=%d (1..32)" % m, d, M=m, K=64)
        for k, m in ((-1, 1), (0, 1), (4, 5), (19, 20), (257, 5), (4096, 32)):
            _rejects(lib, e, _EINVAL, b"K=%d (M=%d..256)" % (k, m), d, K=k, M=m)
        for it in (-1, 65, 1 << 20):
            _rejects(lib, e, _EINVAL, b"iters=%d (0..64)" % it, d, iters=it)
        for r in (-1e-30, -1.0, float("inf"), float("-inf"), float("nan")):
            _rejects(lib, e, _EINVAL, b"miss_radius=", d, radius=r)
        for name in ("pred", "targets", "n_active", "head", "out"):
            _rejects(lib, e, _EINVAL, b"a required buffer pointer is NULL", d, **{name: None})
        _rejects(lib, e, _EINVAL, b"targets must be 8-byte aligned", d, targets=20)
        _rejects(lib, e, _EINVAL, b"per_ped must be 16-byte aligned", d, per_ped=24)
        _rejects(lib, e, _EINVAL, b"workspace must be 8-byte aligned", d, ws=20)
        _rejects(lib, e, _EINVAL, b"workspace of %d bytes needed (got %d)" % (need, need - 8), d,
                 ws_bytes=need - 8)
        _rejects(lib, e, _EINVAL, b"workspace of %d bytes needed" % need, d, ws=None)
        # the weakest alignments the header states are accepted (every other pointer at its
        # element's own); no scene: nothing to do, validated all the same
        none = _dims(S=0, flags=_lib.STEP_TARGETS_SHARED)
        assert _rc(lib, e, none, targets=24, per_ped=32, ws=24, ws_bytes=0, pred=20, head=20, out=20,
                   centres=20, weights=20, n_active=20)[0] == 0
        for k, m, it in ((1, 1, 0), (256, 32, 64), (32, 32, 0), (256, 1, 64)):
            assert _rc(lib, e, _dims(S=0), ws=None, ws_bytes=0, K=k, M=m, iters=it, radius=3.5)[0] == 0
        _rejects(lib, e, _EINVAL, b"K=0 (M=1..256)", _dims(S=0), K=0, M=1)
        _rejects(lib, e, _EINVAL, b"NULL", _dims(S=0), out=None)
    out = (ctypes.c_int32 * 5)()
    geo = lib.g2k_sample_modes_geometry
    assert geo(None, 20, 5, out) == _EINVAL and geo(ctypes.byref(d), 4, 5, out) == _EINVAL
    assert geo(ctypes.byref(d), 257, 5, out) == _EINVAL and geo(ctypes.byref(d), 20, 5, None) == _EINVAL
    assert geo(ctypes.byref(d), 20, 0, out) == _EINVAL and geo(ctypes.byref(d), 64, 33, out) == _EINVAL
    assert geo(ctypes.byref(_dims(Nmax=257)), 20, 5, out) == _EINVAL
    assert geo(ctypes.byref(d), 20, 5, out) == 0


# ---------------------------------------------------------------------------
# the geometry: what tests/modes_cases.py claims, every branch reached
# ---------------------------------------------------------------------------
LDS_BYTES = 256 * 24 * 4 + 64 * 24 * 8 + 256 * 8 + 64 * 2 * 8 + 64 * 4 + 256 + 32 * 8 + 32 * 8 * 8


def test_geometry_claims_and_branches():
    reached = set()
    for i, case in enumerate(mc.CASES):
        name, S, F, N, K, M = case[:6]
        c = mc.inputs(i)
        g = modes.sample_modes_geometry(S, F, N, K, M)
        assert {k: g[k] for k in ("g", "fc", "c")} == c["geom"], (name, g)
        assert g["lanes"] == K and g["g"] * K <= 256 and g["g"] * M <= 64 and g["g"] <= 32
        assert mc.passes_of(i) == c["passes"], (name, mc.passes_of(i))
        # LDS: the draws [256][24] f32, the centres [64][24] f64, the lanes' d2 [256] f64, the
        # centres' {A, F} [64][2] f64 and counts [64], the assignment bytes [256], the pairs'
        # inertia [32] f64 and sums [32][8] f64; with the mixture head's 19376 bytes below the
        # 64 KB of a workgroup
        assert g["lds_bytes"] == LDS_BYTES == 42752 and g["lds_bytes"] + 19376 <= 65536
        lim = dict(lanes=256 // K, centres=64 // M, cap=32)
        reached.update(f"G bound by the {k}" for k, v in lim.items() if v == g["g"] == min(lim.values()))
        raw = 4 * g["g"] // N
        reached.add("FC cut by F" if raw > F else "FC raised to 1" if raw < 1 else "FC = 4 G // Nmax")
        reached.add("rows kernel" if g["c"] > 1 else "one workgroup per scene")
        reached.add("several passes" if c["passes"] > 1 else "one pass")
        if c["passes"] > 1 and (int(c["n_active"].max()) * g["fc"]) % g["g"]:
            reached.add("partial last group")
        reached.add("even K" if K % 2 == 0 else "odd K")
        if K > 64:
            reached.add("pair past one wave")
        if K == 64:
            reached.add("pair at one wave")
        if 64 % K:
            reached.add("pair straddles waves")
        if g["g"] * K < 256:
            reached.add("idle lanes")
        if g["fc"] > 1 and F % g["fc"]:
            reached.add("short last chunk")
        if any(int(n) == 0 for n in c["n_active"]):
            reached.add("empty scene")
        if c["iters"] == 0:
            reached.add("no iteration")
        if M == 1:
            reached.add("one centre")
        if M == K:
            reached.add("M = K")
        if M == 32:
            reached.add("the M cap")
        if K == 256:
            reached.add("the K cap")
        if c["shared"]:
            reached.add("shared targets")
    assert reached == {"G bound by the lanes", "G bound by the centres", "G bound by the cap",
                       "FC cut by F", "FC raised to 1", "FC = 4 G // Nmax", "rows kernel",
                       "one workgroup per scene", "several passes", "one pass", "partial last group",
                       "even K", "odd K", "pair past one wave", "pair at one wave",
                       "pair straddles waves", "idle lanes", "short last chunk", "empty scene",
                       "no iteration", "one centre", "M = K", "the M cap", "the K cap",
                       "shared targets"}, reached
    # the two timing shapes (tools/time_sample_modes.py)
    assert modes.sample_modes_geometry(256, 20, 32, 256, 20) == dict(
        g=1, lanes=256, fc=1, c=20, lds_bytes=LDS_BYTES)
    assert modes.sample_modes_geometry(128, 20, 256, 64, 5) == dict(
        g=4, lanes=64, fc=1, c=20, lds_bytes=LDS_BYTES)
    # F = 0: one workgroup per scene, which writes the zeros
    assert modes.sample_modes_geometry(3, 0, 16, 20, 5)["c"] == 1


# ---------------------------------------------------------------------------
# the checker against an independent restatement
# ---------------------------------------------------------------------------
def _loops(x, y, M, iters, radius):
    """x [K][24] (j = 2t + c), y [12][2] -> (the 8 columns, centres [M][24],
    weights [M]) by plain loops over Python floats."""
    K = len(x)
    x = [[float(v) for v in row] for row in x]
    c = [list(x[m]) for m in range(M)]

    def assign():
        a, d = [], []
        for k in range(K):
            best, bm = None, 0
            for m in range(M):
                d2 = 0.0
                for j in range(2 * L):
                    d2 += (x[k][j] - c[m][j]) ** 2
                if best is None or d2 < best:
                    best, bm = d2, m
            a.append(bm)
            d.append(best)
        return a, d
    for _ in range(iters):
        a, _d = assign()
        for m in range(M):
            members = [k for k in range(K) if a[k] == m]
            if members:
                for j in range(2 * L):
                    s = 0.0
                    for k in members:
                        s += x[k][j]
                    c[m][j] = s / len(members)
    a, d = assign()
    n = [sum(1 for k in range(K) if a[k] == m) for m in range(M)]
    A, Fm = [], []
    for m in range(M):
        dist = [float(np.hypot(c[m][2 * t] - float(y[t][0]), c[m][2 * t + 1] - float(y[t][1])))
                for t in range(L)]
        A.append(sum(dist) / 12.0)
        Fm.append(dist[L - 1])
    mA, mF = A.index(min(A)), Fm.index(min(Fm))
    cols = [A[mA], Fm[mF], mA, mF, n[mA] / K, n[mF] / K, sum(d) / K, sum(1 for v in n if v > 0)]
    return cols, c, [v / K for v in n]


def test_checker_against_plain_loops():
    worst = 0.0
    for name, which in (("m1", "per_step"), ("eval", "fullcov"), ("shared", "mix"), ("m32", "mix"),
                        ("tail", "per_step"), ("collapsed", "fullcov")):
        i = mc.IDS.index(name)
        c = mc.inputs(i)
        R = mc.oracle_modes(i, which)
        x = mo.band_to_flat(mc.oracle_draws(i, which)).astype(np.float64)      # [K, S, F, N, 24]
        S, F, N = c["pairs"].shape
        y = np.broadcast_to(c["targets"].astype(np.float64), (S, F, N, L, 2))
        idx = np.argwhere(c["pairs"])
        for s, f, n in idx[:: max(1, len(idx) // 5)]:
            cols, cen, wts = _loops(x[:, s, f, n], y[s, f, n], c["M"], c["iters"], mc.MISS_RADIUS)
            if R["margin"][s, f, n] >= mo.FRAGILE or name == "collapsed":
                worst = max(worst, float(np.abs(R["per_ped"][s, f, n] - cols).max()))
                band = mo.flat_to_band(np.asarray(cen)[None])[0]               # [1, M, 24] -> [24, M]
                worst = max(worst, float(np.abs(R["centres"][s, f, :, :, n] - band.T).max()))
                worst = max(worst, float(np.abs(R["weights"][s, f, :, n] - wts).max()))
        assert np.all(R["per_ped"][~c["pairs"]] == 0)
        assert np.all(np.moveaxis(R["centres"], 4, 2)[~c["pairs"]] == 0)
        assert np.all(np.moveaxis(R["weights"], 2, 3)[~c["pairs"]] == 0)
        np.testing.assert_array_equal(R["out"][:, 7], c["pairs"].sum(axis=(1, 2)))
        per = R["per_ped"]
        m = c["pairs"]
        want = np.stack([per[..., 0], per[..., 1], (1 - per[..., 4]) ** 2 * m, (1 - per[..., 5]) ** 2 * m,
                         (per[..., 1] > float(np.float32(mc.MISS_RADIUS))) * m, per[..., 6], per[..., 7]],
                        axis=-1).sum(axis=(1, 2))
        np.testing.assert_allclose(R["out"][:, :7], want, atol=1e-12)
        # the weights of a pair add to 1, the live count is the non-zero weights'
        np.testing.assert_allclose(R["weights"].sum(axis=2)[m], 1.0, atol=1e-12)
        np.testing.assert_array_equal((R["weights"] > 0).sum(axis=2)[m], per[..., 7][m])
    print(f"checker vs plain loops: worst {worst:.3g}")
    assert worst <= 1e-12


def test_band_and_flat_layouts_are_inverse():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 3, 24, 5))
    f = mo.band_to_flat(x)
    assert f.shape == (2, 3, 5, 24)
    np.testing.assert_array_equal(f[1, 2, 4, 2 * 7 + 1], x[1, 2, 12 + 7, 4])
    np.testing.assert_array_equal(f[0, 1, 3, 2 * 11], x[0, 1, 11, 3])
    np.testing.assert_array_equal(mo.flat_to_band(f), x)


def test_closed_forms():
    # m1: the centre is the mean of the draws, w = 1, the inertia their variance
    i = mc.IDS.index("m1")
    c = mc.inputs(i)
    for which in mc.HEADS:
        R = mc.oracle_modes(i, which)
        d = mc.oracle_draws(i, which).astype(np.float64)                      # [K, S, F, 24, N]
        m = c["pairs"]
        mean = d.mean(axis=0)                                                  # [S, F, 24, N]
        got = R["centres"][:, :, 0]
        np.testing.assert_allclose(np.moveaxis(got, 2, 3)[m], np.moveaxis(mean, 2, 3)[m], atol=1e-13)
        assert np.all(R["weights"][:, :, 0][m] == 1.0) and np.all(R["per_ped"][..., 4:6][m] == 1.0)
        assert np.all(R["per_ped"][..., 7][m] == 1) and np.all(R["per_ped"][..., 2:4] == 0)
        var = ((d - mean) ** 2).sum(axis=3).mean(axis=0)                      # [S, F, N]
        np.testing.assert_allclose(R["per_ped"][..., 6][m], var[m], rtol=1e-12)
        ade, fde = bestk_ref.draw_errors(mean, c["targets"])
        np.testing.assert_allclose(R["per_ped"][..., 0][m], ade[m], rtol=1e-12)
        np.testing.assert_allclose(R["per_ped"][..., 1][m], fde[m], rtol=1e-12)
        assert np.all(R["out"][:, 2:4] == 0)                                   # (1 - w)^2
    # mk: every draw its own cluster
    i = mc.IDS.index("mk")
    c = mc.inputs(i)
    for which in mc.HEADS:
        R = mc.oracle_modes(i, which)
        d = mc.oracle_draws(i, which).astype(np.float64)
        m = c["pairs"]
        for k in range(c["K"]):
            np.testing.assert_array_equal(np.moveaxis(R["centres"][:, :, k], 2, 3)[m],
                                          np.moveaxis(d[k], 2, 3)[m])
        assert np.all(np.moveaxis(R["weights"], 2, 3)[m] == 1.0 / 8) and np.all(R["per_ped"][..., 6] == 0)
        assert np.all(R["per_ped"][..., 7][m] == 8) and np.all(R["per_ped"][..., 4:6][m] == 0.125)
        np.testing.assert_allclose(R["out"][:, 2], m.sum(axis=(1, 2)) * (7 / 8) ** 2, rtol=1e-14)
    # collapsed: every draw is the mean; all go to centre 0, centres 1..3 are empty and stay
    i = mc.IDS.index("collapsed")
    c = mc.inputs(i)
    for which in mc.heads_of(i):
        d = mc.oracle_draws(i, which)
        m = c["pairs"]
        for k in range(c["K"]):
            np.testing.assert_array_equal(np.moveaxis(d[k], 2, 3)[m], np.moveaxis(c["pred"], 2, 3)[m])
        R = mc.oracle_modes(i, which)
        np.testing.assert_array_equal(np.moveaxis(R["weights"], 2, 3)[m],
                                      np.broadcast_to([1.0, 0, 0, 0], (int(m.sum()), 4)))
        assert np.all(R["per_ped"][..., 7][m] == 1) and np.all(R["per_ped"][..., 6] == 0)
        assert np.all(R["per_ped"][..., 2:4] == 0) and np.all(R["per_ped"][..., 4:6][m] == 1.0)
        ade, fde = bestk_ref.draw_errors(c["pred"].astype(np.float64), c["targets"])
        np.testing.assert_allclose(R["per_ped"][..., 0][m], ade[m], rtol=1e-13)
        np.testing.assert_allclose(R["per_ped"][..., 1][m], fde[m], rtol=1e-13)
        for k in range(c["M"]):                                               # the empty ones kept their place
            np.testing.assert_array_equal(np.moveaxis(R["centres"][:, :, k], 2, 3)[m],
                                          np.moveaxis(c["pred"].astype(np.float64), 2, 3)[m])
        assert np.all(R["margin"][m] == 0)                                     # exact ties by construction


def test_no_iteration_is_best_of_the_first_m_draws():
    i = mc.IDS.index("it0")
    c = mc.inputs(i)
    M = c["M"]
    for which in mc.HEADS:
        R = mc.oracle_modes(i, which)
        d = mc.oracle_draws(i, which).astype(np.float64)
        errs = [bestk_ref.draw_errors(d[k], c["targets"]) for k in range(M)]
        ade = np.stack([e[0] for e in errs])
        fde = np.stack([e[1] for e in errs])
        m = c["pairs"]
        np.testing.assert_allclose(R["per_ped"][..., 0][m], ade.min(axis=0)[m], rtol=1e-13)
        np.testing.assert_allclose(R["per_ped"][..., 1][m], fde.min(axis=0)[m], rtol=1e-13)
        np.testing.assert_array_equal(R["per_ped"][..., 2][m], ade.argmin(axis=0)[m])
        np.testing.assert_array_equal(R["per_ped"][..., 3][m], fde.argmin(axis=0)[m])
        for k in range(M):
            np.testing.assert_array_equal(np.moveaxis(R["centres"][:, :, k], 2, 3)[m],
                                          np.moveaxis(d[k], 2, 3)[m])


def test_inertia_never_increases():
    seen = 0
    for i, which in mc.ALL:
        R = mc.oracle_modes(i, which)
        tr = R["trace"][:, mc.inputs(i)["pairs"]]                             # [iters + 1, P]
        if tr.shape[0] > 1 and tr.shape[1]:
            assert np.all(np.diff(tr, axis=0) <= 1e-12 * np.maximum(1.0, tr[:-1])), (mc.IDS[i], which)
            seen += 1
        np.testing.assert_array_equal(tr[-1] if tr.shape[1] else [], R["per_ped"][..., 6][mc.inputs(i)["pairs"]])
    assert seen >= 25


def test_fragile_share_is_within_the_cap():
    """The cap is a condition on the inputs: at most 1 % of a case's pairs may
    have a margin below 1e-9 (expected: none), the collapsed case aside, whose
    ties are exact by construction."""
    for i, which in mc.ALL:
        if mc.IDS[i] == "collapsed":
            continue
        c = mc.inputs(i)
        R = mc.oracle_modes(i, which)
        n = int(c["pairs"].sum())
        frag = int((R["margin"][c["pairs"]] < mo.FRAGILE).sum())
        low = float(R["margin"][c["pairs"]].min()) if n else float("inf")
        print(f"case {mc.IDS[i]} {which}: {n} pairs, {frag} fragile, smallest margin {low:.3g}")
        assert frag <= mo.FRAGILE_SHARE * n, (mc.IDS[i], which, frag, n)
        assert np.isfinite(R["per_ped"]).all() and np.isfinite(R["out"]).all()
        assert np.isfinite(R["centres"]).all()


def test_boundary_seed_margins_and_the_carry():
    """Case mk (tests/modes_cases.BOUNDARY_ROW says why not m1) at seed A, whose
    low word carries at draw 1 (tests/test_sample_modes_gpu.py runs the kernel
    there): no fragile pair on the restated draws, and the checker's integer
    outputs (mA, mF) change when the draws are made with the carry dropped."""
    for which in mc.HEADS:
        i = mc.IDS.index(mc.BOUNDARY_ROW)
        c = mc.inputs(i)
        m = c["pairs"]
        R, D = (mo.sample_modes_ref(mc.oracle_draws(i, which, SEED_A, carry), c["targets"], m, c["M"], c["iters"],
                                    mc.MISS_RADIUS) for carry in (True, False))
        for v in (R, D):
            assert int((v["margin"][m] < mo.FRAGILE).sum()) == 0 and np.isfinite(v["per_ped"]).all()
        changed = int((R["per_ped"][m][:, [2, 3, 7]] != D["per_ped"][m][:, [2, 3, 7]]).sum())
        moved = np.abs(R["out"][:, :7] - D["out"][:, :7]).max()
        print(f"mk seed A {which}: carry dropped, {changed} of mA, mF, live change, the scene sums move by {moved:.3g}")
        assert changed > 0 and moved > 1e-2


def test_figures():
    out = np.array([[6.0, 9.0, 1.5, 0.75, 2.0, 12.0, 9.0, 3.0], [0.0] * 8])
    f = mo.figures(out)
    assert f == dict(min_ade=2.0, min_fde=3.0, brier_ade=2.5, brier_fde=3.25, miss_rate=2.0 / 3.0,
                     inertia=4.0, live=3.0)
    assert all(np.isnan(v) for v in mo.figures(np.zeros((2, 8))).values())
    assert tuple(f) == mo.FIGURES


# ---------------------------------------------------------------------------
# what the reduction is for
# ---------------------------------------------------------------------------
def test_clustered_centres_beat_the_first_raw_draws():
    """Targets from the AR(1) 0.7 full-covariance law around pred; the oracle's
    256 draws of that head.  20 centres after 10 iterations against the first
    20 raw draws (iters = 0): the mean cA over the pairs falls (DESIGN.md §6k:
    1.19 -> 1.01 over 400 pairs at these widths)."""
    S, F, N, K, M = 2, 2, 12, 256, 20
    rng = np.random.default_rng(2025)
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
    draws = np.stack([fullcov_ref.sample(pred, chol, (500 + k) & MASK64) for k in range(K)]).astype(np.float32)
    raw = mo.sample_modes_ref(draws, tg, pairs, M, 0)
    red = mo.sample_modes_ref(draws, tg, pairs, M, 10)
    a0, a1 = raw["per_ped"][..., 0], red["per_ped"][..., 0]
    d = (a0 - a1).ravel()
    se = d.std(ddof=1) / np.sqrt(d.size)
    print(f"{pairs.sum()} pairs, K {K}, M {M}: mean cA of the first {M} draws {a0.mean():.4f}, of the "
          f"{M} centres after 10 iterations {a1.mean():.4f}; difference {d.mean():.4f} = "
          f"{d.mean() / se:.1f} standard errors; live {red['per_ped'][..., 7].mean():.2f}")
    assert a1.mean() < a0.mean()
    assert red["per_ped"][..., 6].mean() < raw["per_ped"][..., 6].mean()       # and the inertia
