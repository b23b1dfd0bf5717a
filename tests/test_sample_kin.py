"""CPU: the kinematic scores (include/g2k_kin.h, multimodaltraj_2_amd/kin.py,
csrc/g2k_kin.hip) — the header, the module's binding table and the library's
exports agree; every validator rejects bad arguments before touching the GPU;
the launch geometry is what tests/kin_cases.py claims, every branch of it
reached; and the checker tests/kin_ref.py alone: against plain loops, closed
forms, and the reason the scores exist — a target drawn from the head's own law
has uniform PIT ranks, and the per-step head and the full-covariance head, which
share their marginals, are told apart by how their draws move."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib, kin, mixture, modes, ranks, scores
from multimodaltraj_2_amd import build as g2k_build
from tests import kin_cases as kc
from tests import kin_ref as kr
from tests.bestk_ref import SEED_A
from tests import ranks_cases as rc
from tests import ranks_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2k_kin.h")
P = 0x10000                    # a non-NULL pointer, 64-byte aligned (never dereferenced)
OK, EINVAL, EUNSUPPORTED = 0, -1, -4
ENTRIES = (("g2k_sample_kin_f32", "sample_kin"), ("g2k_fullcov_sample_kin_f32", "fullcov_sample_kin"),
           ("g2k_mix_sample_kin_f32", "mix_sample_kin"))
L = 12


def _declarations():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(g2k_[a-z0-9_]+)\s*\(([^)]*)\)", src)}


# ---------------------------------------------------------------------------
# the header, the binding and the exports
# ---------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    decl = _declarations()
    assert sorted(decl) == sorted(kin.SYMBOLS)
    for name, args in decl.items():
        assert len(args.split(",")) == len(kin.SYMBOLS[name][1]), name
    # by symbol, after ABI 11: in no other header or table
    for table in (_lib.SYMBOLS, mixture.SYMBOLS, scores.SYMBOLS, modes.SYMBOLS, ranks.SYMBOLS):
        assert not set(decl) & set(table)
    for other in ("g2k_hip.h", "g2k_mix.h", "g2k_scores.h", "g2k_modes.h", "g2k_ranks.h"):
        assert "sample_kin" not in open(os.path.join(ROOT, "include", other)).read()
    lib = kin.load()
    for name, (res, args) in kin.SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.g2k_abi_version() == _lib.ABI_VERSION == 11
    assert kin.load() is lib
    src = open(HEADER).read()
    for macro, value in (("KMIN", kin.KMIN), ("KMAX", kin.KMAX), ("BMAX", kin.BMAX), ("ROWS", kin.ROWS),
                         ("COLS", kin.COLS), ("GROUPS", len(kin.GROUPS))):
        assert int(re.search(rf"G2K_KIN_{macro} (\d+)", src).group(1)) == value
    assert (kin.KMIN, kin.KMAX, kin.BMAX, kin.ROWS) == (kr.K_MIN, kr.K_MAX, kr.B_MAX, kr.ROWS) == (2, 255, 64, 32)
    assert kin.GROUPS == kr.GROUPS and tuple(kin.GROUPS) == ("speed", "acc", "lacc", "straight")
    assert [s.stop - s.start for s in kin.GROUPS.values()] == [11, 10, 10, 1]
    assert int(re.search(r"G2K_KIN_GEOM_FIELDS (\d+)", src).group(1)) == len(kin.GEOM_FIELDS)
    for i, f in enumerate(kin.GEOM_FIELDS):
        assert int(re.search(rf"G2K_KIN_GEOM_{f.upper()} (\d+)", src).group(1)) == i
    assert kin.GEOM_FIELDS == scores.GEOM_FIELDS
    assert ("Alignment (bytes) of g2k_sample_kin_f32, g2k_fullcov_sample_kin_f32 and\n"
            " * g2k_mix_sample_kin_f32: targets 8, per_ped 16, sums 4, hist 4, tot 8,\n"
            " * workspace 8.") in src
    assert HEADER in [os.path.abspath(p) for p in g2k_build.HDR]    # hashed, and a change rebuilds


# ---------------------------------------------------------------------------
# the validators: before any HIP call
# ---------------------------------------------------------------------------
DIMS = dict(S=2, F=3, T=8, L=12, D=16, H=64, Nmax=5, W=8, stride=0, flags=0)
NEED = 2 * 3 * (8 * 8 + 16 * 4 + 32 * 7 * 4)    # S * F rows of {tot [8] int64, sums [16] f32, hist [32][B = 7] int32}
ARGS = dict(pred=P, targets=2 * P, n_active=3 * P, n_frames=None, ped_mask=None, head=6 * P, seed=7, K=20,
            B=7, per_ped=7 * P, sums=11 * P, hist=8 * P, tot=10 * P, ws=9 * P, ws_bytes=NEED, stream=None)
FLAGS = "{name}: flags %d (0 or G2K_STEP_TARGETS_SHARED)"
NULL = "a required buffer pointer is NULL"
# the checks in the order the library runs them; each fault alone, with its code and full message
CHECKS = [
    ("dims", [({"dims": None}, EINVAL, "dims is NULL")]),
    ("flags", [({"flags": f}, EUNSUPPORTED, FLAGS % f) for f in (1, 4, 6, 256)]),
    ("sizes", [({"Nmax": 0}, EINVAL, "S=2 F=3 Nmax=0"), ({"Nmax": 257}, EINVAL, "S=2 F=3 Nmax=257"),
               ({"S": -1}, EINVAL, "S=-1 F=3 Nmax=5"), ({"F": -1}, EINVAL, "S=2 F=-1 Nmax=5")]),
    ("K", [({"K": 1, "B": 1}, EINVAL, "K=1 (2..255)"), ({"K": 256, "B": 1}, EINVAL, "K=256 (2..255)"),
           ({"K": 0, "B": 1}, EINVAL, "K=0 (2..255)"), ({"K": -5, "B": 1}, EINVAL, "K=-5 (2..255)")]),
    ("B", [({"B": 0}, EINVAL, "B=0 (1..64, a divisor of K + 1 = 21)"),
           ({"B": 4}, EINVAL, "B=4 (1..64, a divisor of K + 1 = 21)"),
           ({"B": 20}, EINVAL, "B=20 (1..64, a divisor of K + 1 = 21)"),
           ({"B": 65, "K": 129}, EINVAL, "B=65 (1..64, a divisor of K + 1 = 130)"),
           ({"B": -1}, EINVAL, "B=-1 (1..64, a divisor of K + 1 = 21)")]),
    ("required", [({n: None}, EINVAL, NULL) for n in ("pred", "targets", "n_active", "head", "sums", "hist",
                                                      "tot")]),
    ("targets", [({"targets": 2 * P + 7}, EINVAL, "targets must be 8-byte aligned"),
                 ({"targets": 2 * P + 4}, EINVAL, "targets must be 8-byte aligned")]),
    ("per_ped", [({"per_ped": 7 * P + 15}, EINVAL, "per_ped must be 16-byte aligned"),
                 ({"per_ped": 7 * P + 8}, EINVAL, "per_ped must be 16-byte aligned")]),
    ("sums", [({"sums": 11 * P + 3}, EINVAL, "sums must be 4-byte aligned"),
              ({"sums": 11 * P + 2}, EINVAL, "sums must be 4-byte aligned")]),
    ("hist", [({"hist": 8 * P + 3}, EINVAL, "hist must be 4-byte aligned"),
              ({"hist": 8 * P + 2}, EINVAL, "hist must be 4-byte aligned")]),
    ("tot", [({"tot": 10 * P + 7}, EINVAL, "tot must be 8-byte aligned"),
             ({"tot": 10 * P + 4}, EINVAL, "tot must be 8-byte aligned")]),
    ("ws_align", [({"ws": 9 * P + 7}, EINVAL, "workspace must be 8-byte aligned"),
                  ({"ws": 9 * P + 4}, EINVAL, "workspace must be 8-byte aligned")]),
    ("ws_size", [({"ws_bytes": NEED - 1}, EINVAL, f"workspace of {NEED} bytes needed (got {NEED - 1})"),
                 ({"ws": None}, EINVAL, f"workspace of {NEED} bytes needed (got {NEED})"),
                 ({"ws_bytes": 0}, EINVAL, f"workspace of {NEED} bytes needed (got 0)")]),
]
# what returns G2K_OK without a launch, at the weakest alignments the header states
SUCCESSES = ({"S": 0}, {"S": 0, "ws": None, "ws_bytes": 0}, {"S": 0, "F": 0, "ws_bytes": 0},
             {"S": 0, "flags": 2}, {"S": 0, "per_ped": None, "K": 255, "B": 64}, {"S": 0, "K": 2, "B": 3},
             {"S": 0, "K": 3, "B": 1},
             {"S": 0, "targets": 2 * P + 8, "per_ped": 7 * P + 16, "sums": 11 * P + 4, "hist": 8 * P + 4,
              "tot": 10 * P + 8, "ws": 9 * P + 8, "pred": P + 4, "head": 6 * P + 4})
REFUSALS = (({"S": 0, "flags": 4}, EUNSUPPORTED, FLAGS % 4), ({"S": 0, "K": 1, "B": 1}, EINVAL, "K=1 (2..255)"),
            ({"S": 0, "B": 2}, EINVAL, "B=2 (1..64, a divisor of K + 1 = 21)"),
            ({"S": 0, "tot": None}, EINVAL, NULL), ({"S": 0, "sums": None}, EINVAL, NULL),
            ({"S": 0, "ws": 9 * P + 4}, EINVAL, "workspace must be 8-byte aligned"))


def _call(lib, symbol, faults):
    dims, args, null_dims = dict(DIMS), dict(ARGS), False
    for key, value in faults.items():
        if key == "dims":
            null_dims = True
        elif key in dims:
            dims[key] = value
        else:
            assert key in args, (symbol, key)
            args[key] = value
    d = None if null_dims else ctypes.byref(_lib.G2KDims(**dims))
    rc_ = getattr(lib, symbol)(d, *args.values())
    return rc_, (lib.g2k_last_error() or b"").decode()


@pytest.mark.parametrize("symbol,name", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_each_fault_alone_and_in_order(symbol, name):
    lib = kin.load()
    for label, ways in CHECKS:
        for faults, code, message in ways:
            assert _call(lib, symbol, faults) == (code, message.format(name=name)), (label, faults)
    # every adjacent pair of checks, both faults present: the earlier check's report
    for (label, first), (label2, second) in zip(CHECKS[1:], CHECKS[2:]):
        faults, code, message = first[0]
        both = dict(second[0][0], **faults)
        assert _call(lib, symbol, both) == (code, message.format(name=name)), (label, label2)


@pytest.mark.parametrize("symbol,name", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_successes_that_launch_nothing(symbol, name):
    lib = kin.load()
    for faults in SUCCESSES:
        rc_, msg = _call(lib, symbol, faults)
        assert rc_ == OK, (faults, msg)
    for faults, code, message in REFUSALS:
        assert _call(lib, symbol, faults) == (code, message.format(name=name)), faults


def test_workspace_bytes_and_geometry_queries():
    lib = kin.load()
    size = lib.g2k_sample_kin_workspace_bytes

    def d(**kw):
        return ctypes.byref(_lib.G2KDims(**dict(DIMS, **kw)))
    assert size(d(), 7) == NEED == 6144 and size(d(), 1) == 6 * (128 + 128) and size(d(), 64) == 6 * (128 + 128 * 64)
    assert size(d(F=0), 7) == 2 * (128 + 896) and size(d(S=0), 7) == 0
    assert size(None, 7) == -1
    for bad in (dict(Nmax=0), dict(Nmax=257), dict(S=-1), dict(F=-1)):
        assert size(d(**bad), 7) == -1
    assert size(d(), 0) == -1 and size(d(), 65) == -1 and size(d(), -3) == -1
    out = (ctypes.c_int32 * 5)()
    geo = lib.g2k_sample_kin_geometry
    for args, msg in (((None, 20, out), "dims is NULL"), ((d(Nmax=257), 20, out), "S=2 F=3 Nmax=257"),
                      ((d(), 1, out), "K=1 (2..255)"), ((d(), 256, out), "K=256 (2..255)"),
                      ((d(), 20, None), "out is NULL")):
        assert geo(*args) == EINVAL and lib.g2k_last_error().decode() == msg
    assert geo(d(), 20, out) == OK and geo(d(S=0), 2, out) == OK and geo(d(flags=1), 255, out) == OK


# ---------------------------------------------------------------------------
# the geometry: what tests/kin_cases.py claims, every branch reached
# ---------------------------------------------------------------------------
def test_geometry_claims_and_branches():
    reached = set()
    for i, case in enumerate(kc.CASES):
        name, S, F, N, K, B = case[:6]
        c = kc.inputs(i)
        g = kin.sample_kin_geometry(S, F, N, K)
        assert {k: g[k] for k in ("g", "fc", "c")} == c["geom"], (name, g)
        assert g["lanes"] == K and g["g"] * K <= 256
        assert kc.passes_of(i) == c["passes"], (name, kc.passes_of(i))
        assert (K + 1) % B == 0 and 1 <= B <= 64
        # LDS: the draws' features [256][24] (the scores kernel's xy footprint), the targets'
        # [32][24], the pairs' 16 sums [32][17], the histogram [32][64], the eight totals and the
        # waves' partial sums [4][16]; with the mixture head's 19376 bytes below 64 KB
        assert g["lds_bytes"] == 4 * (256 * 24 + 32 * 24 + 32 * 17 + 32 * 64 + 8 + 4 * 16) == 38304
        assert g["lds_bytes"] + 19376 <= 65536
        # the same shapes give the scores' kernel the same geometry
        assert {k: scores.sample_scores_geometry(S, F, N, K)[k] for k in ("g", "fc", "c")} == c["geom"]
        reached.add("G capped" if 256 // K > 32 else "G = 256 // K")
        raw = 4 * g["g"] // N
        reached.add("FC cut by F" if raw > F else "FC raised to 1" if raw < 1 else "FC = 4 G // Nmax")
        reached.add("rows kernel" if g["c"] > 1 else "one workgroup per scene")
        reached.add("several passes" if c["passes"] > 1 else "one pass")
        if c["passes"] > 1 and (int(c["n_active"].max()) * g["fc"]) % g["g"]:
            reached.add("partial last group")
        if K > 64:
            reached.add("pair past one wave")
        if K == 64:
            reached.add("pair = one wave")
        if 64 % K:
            reached.add("pair straddles waves")
        if g["fc"] > 1 and F % g["fc"]:
            reached.add("short last chunk")
        if any(int(n) == 0 for n in c["n_active"]):
            reached.add("empty scene")
        if c["shared"]:
            reached.add("shared targets")
        reached.add({2: "K minimum", 255: "K maximum"}.get(K, "K between"))
        reached.add("K even" if K % 2 == 0 else "K odd")
        reached.add("B = K + 1" if B == K + 1 else "B maximum" if B == 64 else "B minimum" if B == 1
                    else "several ranks per bin")
        if N == 256:
            reached.add("Nmax maximum")
    assert reached == {"G capped", "G = 256 // K", "FC cut by F", "FC raised to 1", "FC = 4 G // Nmax",
                       "rows kernel", "one workgroup per scene", "several passes", "one pass",
                       "partial last group", "pair past one wave", "pair = one wave", "pair straddles waves",
                       "short last chunk", "empty scene", "shared targets", "K minimum", "K maximum",
                       "K between", "K even", "K odd", "B = K + 1", "B maximum", "B minimum",
                       "several ranks per bin", "Nmax maximum"}, reached
    # the table is tests/ranks_cases.py's: shapes, masks and geometry, with K and B lowered in two cases
    for a, b in zip(kc.CASES, rc.CASES):
        assert a[1:4] + a[6:] == b[1:4] + b[6:]
        assert a == b or a[0] in ("k2", "shared")
    assert len(kc.CASES) == len(rc.CASES)
    assert {c[0]: c[4:6] for c in kc.CASES if c[0] in ("k2", "shared", "k255")} == {
        "k2": (2, 3), "shared": (3, 1), "k255": (255, 64)}
    k20 = kc.IDS.index("k20")
    for key in ("head", "chol", "mix"):
        np.testing.assert_array_equal(kc.inputs(k20)[key], rc.inputs(rc.IDS.index("k20"))[key])
    # the evaluation's two timing shapes (tools/time_sample_kin.py)
    assert kin.sample_kin_geometry(256, 20, 32, 20) == dict(g=12, lanes=20, fc=1, c=20, lds_bytes=38304)
    assert kin.sample_kin_geometry(128, 20, 256, 20)["c"] == 20
    # F = 0: one workgroup per scene, which writes the zeros
    assert kin.sample_kin_geometry(3, 0, 16, 20)["c"] == 1


# ---------------------------------------------------------------------------
# the checker against an independent restatement
# ---------------------------------------------------------------------------
def test_checker_against_plain_loops():
    checked = 0
    for name in ("k2", "shared", "k20"):
        i = kc.IDS.index(name)
        c = kc.inputs(i)
        S, F, N = c["pairs"].shape
        y = np.broadcast_to(c["targets"], (S, F, N, L, 2))
        for which in kc.HEADS:
            draws = kc.oracle_draws(i, which)
            R = kr.sample_kin_ref(draws, c["targets"], c["pairs"])
            x = kr.band_to_xy(draws)
            for s, f, n in np.argwhere(c["pairs"])[::5]:
                want = kr.pair_loops(x[:, s, f, n], y[s, f, n])
                got = R["per"][s, f, n]
                assert list(got[:32]) == want[:32], (name, which, s, f, n)
                np.testing.assert_allclose(got[32:], want[32:], rtol=1e-12, atol=1e-13)
                checked += 1
            per = R["per"]
            assert np.all(per[~c["pairs"]] == 0) and np.isfinite(per).all()
            assert per[..., :32].min() >= 0 and per[..., :32].max() <= c["K"]
            # the features: the vectorised restatement is the loops' bit for bit
            np.testing.assert_array_equal(R["fy"][0], np.array(kr.features_loops(y[c["pairs"]][0]), np.float32))
            assert R["fx"].dtype == np.float32 and R["fy"].dtype == np.float32
            # |x - y| >= 0 and the triangle inequality: p_g <= 2 m_g, so every crps >= 0
            m, p = per[c["pairs"]][:, 32:36], per[c["pairs"]][:, 36:40]
            assert np.all(m >= 0) and np.all(p >= 0) and np.all(p <= 2 * m + 1e-12)
            np.testing.assert_allclose(R["sums"], per[..., 32:].sum(axis=(1, 2)), rtol=0, atol=0)
    assert checked >= 30


@pytest.mark.parametrize("which", kc.HEADS)
def test_boundary_seed_ties_and_the_carry(which):
    """Case k2 at seed A, whose low word carries at draw 1
    (tests/test_sample_kin_gpu.py runs the kernel there): no fp32 tie between a
    draw's feature and the target's on the restated draws, and the checker's
    ranks and hist change when the draws are made with the carry dropped."""
    i = kc.IDS.index("k2")
    c = kc.inputs(i)
    R, D = (kr.sample_kin_ref(kc.oracle_draws(i, which, SEED_A, carry), c["targets"], c["pairs"])
            for carry in (True, False))
    for v in (R, D):
        assert int((v["fx"] == v["fy"][None]).sum()) == 0 and np.isfinite(v["per"]).all()
    changed = int((R["per"][..., :32] != D["per"][..., :32]).sum())
    hr, hd = (kr.hist_tot(v["per"], c["pairs"], c["K"], c["B"])[0] for v in (R, D))
    moved = np.abs(R["sums"] - D["sums"]).max()
    print(f"k2 seed A {which}: carry dropped, {changed} ranks change, sums move by {moved:.3g}")
    assert changed > 0 and not np.array_equal(hr, hd) and moved > 1e-2


def _band(xy):
    """[..., N, L, 2] -> [..., 2L, N]."""
    a = np.moveaxis(np.asarray(xy), -3, -1)                         # [..., L, 2, N]
    return np.concatenate([a[..., 0, :], a[..., 1, :]], axis=-2)


def _line(start, step):
    """A constant-velocity trajectory [L, 2] float32."""
    return (np.asarray(start, np.float32)[None] + np.arange(L, dtype=np.float32)[:, None]
            * np.asarray(step, np.float32)[None]).astype(np.float32)


def test_closed_forms():
    # a constant-velocity trajectory: s constant, a = l = 0, st = 1 (exact: small integers)
    f = kr.features(_line([1.0, -2.0], [3.0, 4.0]))
    assert np.all(f[:11] == 5.0) and np.all(f[11:31] == 0.0) and f[31] == 1.0
    assert kr.features_loops(_line([1.0, -2.0], [3.0, 4.0])) == list(f)
    # a stationary one: len = 0, st = 1 by definition
    f0 = kr.features(np.full((L, 2), 7.5, np.float32))
    assert np.all(f0[:31] == 0.0) and f0[31] == 1.0 and kr.features_loops(np.full((L, 2), 7.5, np.float32)) == list(f0)
    # there and back: six steps out, five back along the same line: st = 1/11
    z = np.zeros((L, 2), np.float32)
    z[:, 0] = [0, 1, 2, 3, 4, 5, 6, 5, 4, 3, 2, 1]
    fz = kr.features(z)
    assert np.all(fz[:11] == 1.0) and fz[31] == np.float32(1.0) / np.float32(11.0)
    assert list(fz[11:21]) == [0, 0, 0, 0, 0, 2, 0, 0, 0, 0] and np.all(fz[21:31] == 0.0)
    # a quarter turn at constant speed: a = sqrt(2) s, l = 0
    q = np.zeros((L, 2), np.float32)
    q[:, 0] = [0, 1, 2, 3, 4, 5, 5, 5, 5, 5, 5, 5]
    q[:, 1] = [0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6]
    fq = kr.features(q)
    assert fq[11 + 4] == np.sqrt(np.float32(2.0)) and np.all(fq[21:31] == 0.0)
    assert fq[31] == np.sqrt(np.float32(61.0)) / np.float32(11.0)
    # K = 2 by hand: X_0 walks (3, 4) a step (speed 5), X_1 stands still, Y walks (0, 2) a step (speed 2)
    x = np.stack([_line([0.0, 0.0], [3.0, 4.0]), np.full((L, 2), 1.0, np.float32)])   # [K, L, 2]
    y = _line([5.0, 5.0], [0.0, 2.0])
    pairs = np.ones((1, 1, 1), bool)
    R = kr.sample_kin_ref(_band(x[:, None, None, None]), y[None, None, None], pairs)
    per = R["per"][0, 0, 0]
    assert list(per[:11]) == [1.0] * 11 and not per[11:32].any()          # only X_1 is slower; ties rank 0
    assert list(per[32:36]) == [2.5, 0.0, 0.0, 0.0]                       # m: (|5 - 2| + |0 - 2|) / 2
    assert list(per[36:40]) == [5.0, 0.0, 0.0, 0.0]                       # p: |5 - 0|
    assert list(per[40:44]) == [2.5, 0.0, 0.0, 1.0]                       # d
    assert list(per[44:48]) == [2.0, 0.0, 0.0, 1.0]                       # y
    assert per[32] - 0.5 * per[36] == 0.0                                 # the fair CRPS of two draws around y
    assert kr.pair_loops(x, y) == list(per)
    hist, tot = kr.hist_tot(R["per"], pairs, 2, 3)
    assert hist.shape == (1, 32, 3) and np.all(hist[0, :11] == [0, 1, 0]) and np.all(hist[0, 11:] == [1, 0, 0])
    assert list(tot[0]) == [1, 11, 0, 0, 0, 0, 0, 0]
    # sigma = 0: every draw is the prediction: p = 0, d the prediction's feature, ranks in {0, K}
    K = 5
    z5 = np.broadcast_to(q[None], (K, L, 2))
    R = kr.sample_kin_ref(_band(z5[:, None, None, None]), y[None, None, None], pairs)
    per = R["per"][0, 0, 0]
    assert not per[36:40].any() and set(per[:32]) <= {0.0, float(K)}
    np.testing.assert_allclose(per[40:44], [fq[:11].mean(), fq[11:21].mean(), 0.0, fq[31]], rtol=1e-7)


@pytest.mark.parametrize("K,B", [(20, 21), (20, 7), (255, 32), (2, 3), (3, 1)])
def test_bin_edges_and_the_result_class(K, B):
    """Every rank 0..K once: (K + 1) / B in each bin, bin floor(r B / (K + 1));
    the result class's figures on hand-made counts."""
    w = (K + 1) // B
    per = np.zeros((1, 1, K + 1, 48))
    per[0, 0, :, :32] = np.arange(K + 1)[:, None]
    per[0, 0, :, 32:] = np.arange(16)[None] + 1.0
    pairs = np.ones((1, 1, K + 1), bool)
    hist, tot = kr.hist_tot(per, pairs, K, B)
    assert np.all(hist == w) and tot[0, 0] == K + 1
    assert list(tot[0, 1:]) == [11 * K * (K + 1) // 2, 10 * K * (K + 1) // 2, 10 * K * (K + 1) // 2,
                                K * (K + 1) // 2, 0, 0, 0]
    sums = per[..., 32:].sum(axis=(1, 2))
    sk = kin.SampleKin(sums=torch.from_numpy(sums.astype(np.float32)), hist=torch.from_numpy(hist.astype(np.int32)),
                       tot=torch.from_numpy(tot), per_ped=None, k=K, bins=B)
    assert sk.pairs == K + 1 and sk.counts().shape == (32, B)
    want = kr.figures(sums, hist, tot, K)
    for gi, g in enumerate(kin.GROUPS):
        assert sk.dev(g) == 0.0 and sk.pit_mean(g) == pytest.approx(0.5, abs=1e-15)
        assert sk.crps(g) == pytest.approx((gi + 1) - 0.5 * (gi + 5)) and sk.draw_mean(g) == pytest.approx(gi + 9)
        assert sk.target_mean(g) == pytest.approx(gi + 13)
        for name, fn in (("crps", sk.crps), ("pit_mean", sk.pit_mean), ("dev", sk.dev), ("draw_mean", sk.draw_mean),
                         ("target_mean", sk.target_mean)):
            assert fn(g) == pytest.approx(want[g][name], abs=1e-12)
    # everything in the last bin: as far from uniform as it gets; no pair: NaN
    hist[:] = 0
    hist[:, :, B - 1] = K + 1
    sk.hist = torch.from_numpy(hist.astype(np.int32))
    assert sk.dev("acc") == pytest.approx(1.0 - 1.0 / B)
    empty = kin.SampleKin(sums=torch.zeros((2, 16)), hist=torch.zeros((2, 32, B), dtype=torch.int32),
                          tot=torch.zeros((2, 8), dtype=torch.int64), per_ped=None, k=K, bins=B)
    assert empty.pairs == 0
    for g in kin.GROUPS:
        assert all(np.isnan(v) for v in (empty.crps(g), empty.pit_mean(g), empty.dev(g), empty.draw_mean(g),
                                         empty.target_mean(g)))
    with pytest.raises(ValueError, match="one of speed, acc, lacc, straight"):
        sk.crps("turn")


def test_python_argument_checks():
    for k in (1, 256):
        with pytest.raises(ValueError, match="2..255"):
            kin.check_k_bins(k, None)
    for b in (4, 65, -1):
        with pytest.raises(ValueError, match="a divisor of k \\+ 1"):
            kin.check_k_bins(20, b)
    assert kin.check_k_bins(20, None) == (20, 21) and kin.check_k_bins(20, 0) == (20, 21)
    assert kin.check_k_bins(255, None) == (255, 32) and kin.check_k_bins(255, 64) == (255, 64)
    assert kin.check_k_bins(2, None) == (2, 3) and kin.check_k_bins(3, 1) == (3, 1)
    assert kin.check_k_bins(130, None) == (130, 1)                   # 131 is prime
    assert [kin.auto_bins(k) for k in (2, 3, 4, 6, 8, 40, 64, 65)] == [3, 4, 5, 7, 9, 1, 13, 22]


# ---------------------------------------------------------------------------
# what the scores are for: the heads differ in how their draws move
# ---------------------------------------------------------------------------
PROP = dict(S=4, F=4, N=128, K=20, B=21, seed=777)
PROP_ROWS = (0, 11, 21, 31)                # one row of each group


def property_check(score, label=""):
    """The property test, for the CPU (the restated samplers) and the device
    alike.  ``score(target_head, scoring_head)`` -> (counts [32, B], dict group
    -> dict(crps, pit_mean)) of targets = target_head's draw for seed + K scored
    under scoring_head's K draws.  Under the same head the ranks of rows 0, 11,
    21 and 31 are uniform (Pearson's chi^2 below the 0.999 quantile at 20 degrees
    of freedom; fixed seeds, so deterministic).  The two Gaussian heads share
    their marginals and differ in how a draw moves: the per-step head's 12
    independent steps zig-zag, so its draws accelerate harder and run less
    straight than the full-covariance head's.  Cross-scored, rows 11 and 31 are
    not uniform, every group's CRPS is larger than under the right head, and
    the mean PIT of the accelerations is below 1/2 for smooth targets among
    zig-zag draws and above it the other way round."""
    quant = rr.chi2_quantile(0.999, PROP["B"] - 1)
    assert abs(quant - 45.31) < 0.15
    own = {}
    for which in kc.HEADS:
        counts, fig = score(which, which)
        x2 = [rr.chi2(counts[j]) for j in PROP_ROWS]
        print(f"{label}{which} scored by itself: chi^2 rows 0 / 11 / 21 / 31 " + " / ".join(f"{v:.1f}" for v in x2)
              + f" (quantile {quant:.1f}), pit acc {fig['acc']['pit_mean']:.3f}, crps "
              + " / ".join(f"{fig[g]['crps']:.3f}" for g in kin.GROUPS))
        assert all(v < quant for v in x2), (which, x2)
        assert abs(fig["acc"]["pit_mean"] - 0.5) < 0.02
        own[which] = fig
    for target, scorer, side in (("fullcov", "per_step", -1), ("per_step", "fullcov", +1)):
        counts, fig = score(target, scorer)
        x2 = [rr.chi2(counts[j]) for j in (11, 31)]
        print(f"{label}{target} targets scored by {scorer}: chi^2 rows 11 / 31 {x2[0]:.1f} / {x2[1]:.1f}, pit acc "
              f"{fig['acc']['pit_mean']:.3f}, crps " + " / ".join(f"{fig[g]['crps']:.3f}" for g in kin.GROUPS))
        assert all(v > quant for v in x2), (target, scorer, x2)
        for g in kin.GROUPS:
            assert fig[g]["crps"] > own[target][g]["crps"], (target, scorer, g)
        assert side * (fig["acc"]["pit_mean"] - 0.5) > 0.1, (target, scorer, fig["acc"]["pit_mean"])


def test_heads_are_told_apart_by_how_their_draws_move():
    S, F, N, K, B, seed = (PROP[k] for k in ("S", "F", "N", "K", "B", "seed"))
    c = kc.inputs(kc.IDS.index("k20"))
    pred = kc.property_setup(S, F, N)
    pairs = np.ones((S, F, N), bool)
    draws, targets = {}, {}
    for which in kc.HEADS:
        dr = kc.sampler(which, c)
        draws[which] = np.stack([dr(pred, seed + k) for k in range(K)]).astype(np.float32)
        targets[which] = kr.band_to_xy(np.asarray(dr(pred, seed + K), np.float32))

    def score(target, scorer):
        R = kr.sample_kin_ref(draws[scorer], targets[target], pairs)
        hist, tot = kr.hist_tot(R["per"], pairs, K, B)
        ties = int((R["fx"] == R["fy"][None]).sum())
        assert ties == 0                                             # no fp32 tie decides a rank here
        return hist.sum(axis=0), kr.figures(R["sums"], hist, tot, K)
    property_check(score)


# ---------------------------------------------------------------------------
# the evaluation's flags
# ---------------------------------------------------------------------------
def test_evaluation_flags():
    from multimodaltraj_2_amd import evaluate
    from multimodaltraj_2_amd.argParser import ArgsParser
    a = ArgsParser().parser.parse_args([])
    assert a.sample_kinematics == 0 and a.kin_bins == 0
    a = ArgsParser().parser.parse_args(["--num_samples", "20", "--sample_kinematics", "1", "--kin_bins", "7"])
    assert a.sample_kinematics == 1 and a.kin_bins == 7
    with pytest.raises(SystemExit):
        ArgsParser().parser.parse_args(["--sample_kinematics", "2"])
    assert evaluate.KIN_FIGURES == tuple(f"kin_{f}_{g}" for f in ("crps", "pit", "dev", "draw", "target")
                                         for g in ("speed", "acc", "lacc", "straight"))
    assert len(evaluate.KIN_FIGURES) == 20 and "kin_draw_acc" in evaluate.KIN_FIGURES
    assert evaluate.FULLCOV_KIN_FIGURES == tuple("fullcov_" + k for k in evaluate.KIN_FIGURES)
    assert evaluate.MIX_KIN_FIGURES == tuple("mix_" + k for k in evaluate.KIN_FIGURES)
    # refused before any data is read or any launch made
    for k, b, word in ((1, 0, "2 <= K <= 255"), (256, 0, "2 <= K <= 255"), (20, 4, "--kin_bins"),
                       (20, 65, "--kin_bins"), (255, 128, "--kin_bins")):
        a.num_samples, a.kin_bins = k, b
        with pytest.raises(ValueError, match=word):
            evaluate.evaluate_best_of_k(a, None, None, log=lambda s: None)
    # the figures of a result, in the stated order, on hand-made counts
    hist = np.full((1, 32, 7), 3, np.int32)
    tot = np.array([[21, 11 * 210, 10 * 210, 10 * 210, 210, 0, 0, 0]], np.int64)
    sums = 21.0 * (np.arange(16, dtype=np.float32)[None] + 1)
    sk = kin.SampleKin(sums=torch.from_numpy(sums), hist=torch.from_numpy(hist), tot=torch.from_numpy(tot),
                       per_ped=None, k=20, bins=7)
    for prefix, names in (("", evaluate.KIN_FIGURES), ("fullcov_", evaluate.FULLCOV_KIN_FIGURES),
                          ("mix_", evaluate.MIX_KIN_FIGURES)):
        fig = evaluate.kin_figures(sk, prefix)
        assert tuple(fig) == names
        assert fig[prefix + "kin_dev_acc"] == 0.0 and fig[prefix + "kin_pit_lacc"] == pytest.approx(0.5)
        assert fig[prefix + "kin_crps_acc"] == pytest.approx(2 - 3.0) and fig[prefix + "kin_draw_speed"] == 9.0
        assert fig[prefix + "kin_target_straight"] == 16.0
