"""CPU: the couple-distance scores (include/g2k_couples.h,
multimodaltraj_2_amd/couples.py, csrc/g2k_couples.hip) — the header, the
module's binding table and the library's exports agree; every validator rejects
bad arguments before touching the GPU; the launch geometry is what
tests/couples_cases.py claims, every branch of it reached; and the checker
tests/couples_ref.py alone: against plain loops, closed forms, and the reason
the scores exist — two laws with the same marginals and different dependence
BETWEEN pedestrians, which no per-pedestrian score can tell apart, are told
apart at once."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib, couples, kin, mixture, modes, ranks, scores
from multimodaltraj_2_amd import build as g2k_build
from oracle import g2k_ref as ref
from tests import couples_cases as cc
from tests import couples_ref as cr
from tests.bestk_ref import BOUNDARY_SEEDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2k_couples.h")
P = 0x10000                    # a non-NULL pointer, 64-byte aligned (never dereferenced)
OK, EINVAL, EUNSUPPORTED = 0, -1, -4
ENTRIES = (("g2k_couple_scores_f32", "couple_scores"), ("g2k_fullcov_couple_scores_f32", "fullcov_couple_scores"),
           ("g2k_mix_couple_scores_f32", "mix_couple_scores"))
L = 12
INF = float("inf")


def _declarations():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(g2k_[a-z0-9_]+)\s*\(([^)]*)\)", src)}


# ---------------------------------------------------------------------------
# the header, the binding and the exports
# ---------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    decl = _declarations()
    assert sorted(decl) == sorted(couples.SYMBOLS)
    for name, args in decl.items():
        assert len(args.split(",")) == len(couples.SYMBOLS[name][1]), name
    # by symbol, after ABI 11: in no other header or table
    for table in (_lib.SYMBOLS, mixture.SYMBOLS, scores.SYMBOLS, modes.SYMBOLS, ranks.SYMBOLS, kin.SYMBOLS):
        assert not set(decl) & set(table)
    for other in ("g2k_hip.h", "g2k_mix.h", "g2k_scores.h", "g2k_modes.h", "g2k_ranks.h", "g2k_kin.h"):
        assert "couple_scores" not in open(os.path.join(ROOT, "include", other)).read()
    lib = couples.load()
    for name, (res, args) in couples.SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.g2k_abi_version() == _lib.ABI_VERSION == 11
    assert couples.load() is lib
    src = open(HEADER).read()
    for macro, value in (("KMIN", couples.KMIN), ("KMAX", couples.KMAX), ("BMAX", couples.BMAX),
                         ("FEATURES", len(couples.FEATURES)), ("SUMS", couples.NSUMS), ("TOT", couples.NTOT)):
        assert int(re.search(rf"G2K_COUPLES_{macro} (\d+)", src).group(1)) == value
    assert (couples.KMIN, couples.KMAX, couples.BMAX) == (cr.K_MIN, cr.K_MAX, cr.B_MAX) == (2, 64, 64)
    assert couples.FEATURES == cr.FEATURES == ("min", "fin")
    assert int(re.search(r"G2K_COUPLES_GEOM_FIELDS (\d+)", src).group(1)) == len(couples.GEOM_FIELDS)
    for i, f in enumerate(couples.GEOM_FIELDS):
        assert int(re.search(rf"G2K_COUPLES_GEOM_{f.upper()} (\d+)", src).group(1)) == i
    assert ("Alignment (bytes) of g2k_couple_scores_f32, g2k_fullcov_couple_scores_f32 and\n"
            " * g2k_mix_couple_scores_f32: targets 8, per_couple 4, per_frame_f 4,\n"
            " * per_frame_i 4, sums 4, hist 4, tot 8, workspace 4.") in src
    assert HEADER in [os.path.abspath(p) for p in g2k_build.HDR]    # hashed, and a change rebuilds


# ---------------------------------------------------------------------------
# the validators: before any HIP call
# ---------------------------------------------------------------------------
DIMS = dict(S=2, F=3, T=8, L=12, D=16, H=64, Nmax=5, W=8, stride=0, flags=0)
NEED = 2 * 3 * (12 + 2 * 7) * 4          # S * F scene-frames, one workgroup each, a row [12 + 2 B] of int32
ARGS = dict(pred=P, targets=2 * P, n_active=3 * P, n_frames=None, ped_mask=None, head=6 * P, seed=7, K=20,
            B=7, reach=0.5, per_couple=7 * P, per_frame_f=12 * P, per_frame_i=13 * P, sums=11 * P, hist=8 * P,
            tot=10 * P, ws=9 * P, ws_bytes=NEED, stream=None)
FLAGS = "{name}: flags %d (0 or G2K_STEP_TARGETS_SHARED)"
NULL = "a required buffer pointer is NULL"
REACH = "reach=%s (> 0, or +inf: every couple)"


def _align4(name, base):
    return (name, [({name: base + 3}, EINVAL, f"{name} must be 4-byte aligned"),
                   ({name: base + 2}, EINVAL, f"{name} must be 4-byte aligned")])


# the checks in the order the library runs them; each fault alone, with its code and full message
CHECKS = [
    ("dims", [({"dims": None}, EINVAL, "dims is NULL")]),
    ("flags", [({"flags": f}, EUNSUPPORTED, FLAGS % f) for f in (1, 4, 6, 256)]),
    ("sizes", [({"Nmax": 0}, EINVAL, "S=2 F=3 Nmax=0"), ({"Nmax": 257}, EINVAL, "S=2 F=3 Nmax=257"),
               ({"S": -1}, EINVAL, "S=-1 F=3 Nmax=5"), ({"F": -1}, EINVAL, "S=2 F=-1 Nmax=5")]),
    ("K", [({"K": 1, "B": 1}, EINVAL, "K=1 (2..64)"), ({"K": 65, "B": 1}, EINVAL, "K=65 (2..64)"),
           ({"K": 0, "B": 1}, EINVAL, "K=0 (2..64)"), ({"K": -5, "B": 1}, EINVAL, "K=-5 (2..64)")]),
    ("B", [({"B": 0}, EINVAL, "B=0 (1..64, a divisor of K + 1 = 21)"),
           ({"B": 4}, EINVAL, "B=4 (1..64, a divisor of K + 1 = 21)"),
           ({"B": 20}, EINVAL, "B=20 (1..64, a divisor of K + 1 = 21)"),
           ({"B": 65, "K": 64}, EINVAL, "B=65 (1..64, a divisor of K + 1 = 65)"),
           ({"B": -1}, EINVAL, "B=-1 (1..64, a divisor of K + 1 = 21)")]),
    ("reach", [({"reach": 0.0}, EINVAL, REACH % "0"), ({"reach": -1.5}, EINVAL, REACH % "-1.5"),
               ({"reach": float("nan")}, EINVAL, None), ({"reach": -INF}, EINVAL, REACH % "-inf")]),
    ("required", [({n: None}, EINVAL, NULL) for n in ("pred", "targets", "n_active", "head", "sums", "hist",
                                                      "tot")]),
    ("targets", [({"targets": 2 * P + 7}, EINVAL, "targets must be 8-byte aligned"),
                 ({"targets": 2 * P + 4}, EINVAL, "targets must be 8-byte aligned")]),
    _align4("per_couple", 7 * P), _align4("per_frame_f", 12 * P), _align4("per_frame_i", 13 * P),
    _align4("sums", 11 * P), _align4("hist", 8 * P),
    ("tot", [({"tot": 10 * P + 7}, EINVAL, "tot must be 8-byte aligned"),
             ({"tot": 10 * P + 4}, EINVAL, "tot must be 8-byte aligned")]),
    ("ws_align", [({"ws": 9 * P + 3}, EINVAL, "workspace must be 4-byte aligned"),
                  ({"ws": 9 * P + 2}, EINVAL, "workspace must be 4-byte aligned")]),
    ("ws_size", [({"ws_bytes": NEED - 1}, EINVAL, f"workspace of {NEED} bytes needed (got {NEED - 1})"),
                 ({"ws": None}, EINVAL, f"workspace of {NEED} bytes needed (got {NEED})"),
                 ({"ws_bytes": 0}, EINVAL, f"workspace of {NEED} bytes needed (got 0)")]),
]
# what returns G2K_OK without a launch, at the weakest alignments the header states
SUCCESSES = ({"S": 0}, {"S": 0, "ws": None, "ws_bytes": 0}, {"S": 0, "F": 0, "ws_bytes": 0},
             {"S": 0, "flags": 2}, {"S": 0, "per_couple": None, "K": 64, "B": 65 // 5}, {"S": 0, "K": 2, "B": 3},
             {"S": 0, "reach": INF}, {"S": 0, "reach": 1e-30},
             {"S": 0, "per_couple": None, "per_frame_f": None, "per_frame_i": None},
             {"S": 0, "targets": 2 * P + 8, "per_couple": 7 * P + 4, "per_frame_f": 12 * P + 4,
              "per_frame_i": 13 * P + 4, "sums": 11 * P + 4, "hist": 8 * P + 4, "tot": 10 * P + 8,
              "ws": 9 * P + 4, "pred": P + 4, "head": 6 * P + 4})
REFUSALS = (({"S": 0, "flags": 4}, EUNSUPPORTED, FLAGS % 4), ({"S": 0, "K": 1, "B": 1}, EINVAL, "K=1 (2..64)"),
            ({"S": 0, "B": 2}, EINVAL, "B=2 (1..64, a divisor of K + 1 = 21)"),
            ({"S": 0, "reach": 0.0}, EINVAL, REACH % "0"),
            ({"S": 0, "tot": None}, EINVAL, NULL), ({"S": 0, "sums": None}, EINVAL, NULL),
            ({"S": 0, "ws": 9 * P + 2}, EINVAL, "workspace must be 4-byte aligned"))


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


def _expect(got, code, message, name):
    if message is None:                                  # NaN: the platform's spelling of it
        assert got[0] == code and re.fullmatch(r"reach=-?nan \(> 0, or \+inf: every couple\)", got[1]), got
    else:
        assert got == (code, message.format(name=name)), got


@pytest.mark.parametrize("symbol,name", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_each_fault_alone_and_in_order(symbol, name):
    lib = couples.load()
    for label, ways in CHECKS:
        for faults, code, message in ways:
            _expect(_call(lib, symbol, faults), code, message, name)
    # every adjacent pair of checks, both faults present: the earlier check's report
    for (label, first), (label2, second) in zip(CHECKS[1:], CHECKS[2:]):
        faults, code, message = first[0]
        both = dict(second[0][0], **faults)
        _expect(_call(lib, symbol, both), code, message, name)


@pytest.mark.parametrize("symbol,name", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_successes_that_launch_nothing(symbol, name):
    lib = couples.load()
    for faults in SUCCESSES:
        rc_, msg = _call(lib, symbol, faults)
        assert rc_ == OK, (faults, msg)
    for faults, code, message in REFUSALS:
        _expect(_call(lib, symbol, faults), code, message, name)


def test_workspace_bytes_and_geometry_queries():
    lib = couples.load()
    size = lib.g2k_couple_scores_workspace_bytes

    def d(**kw):
        return ctypes.byref(_lib.G2KDims(**dict(DIMS, **kw)))
    assert size(d(), 20, 7) == NEED == 624 and size(d(), 20, 1) == 6 * 14 * 4 and size(d(), 63, 64) == 6 * 140 * 4
    assert size(d(F=0), 20, 7) == 2 * 26 * 4 and size(d(S=0), 20, 7) == 0
    # the workgroups of a scene-frame count: Nmax 256 at K 20 has 136 tiles, 8 workgroups
    assert size(d(Nmax=256), 20, 7) == 6 * 8 * 26 * 4
    assert size(None, 20, 7) == -1
    for bad in (dict(Nmax=0), dict(Nmax=257), dict(S=-1), dict(F=-1)):
        assert size(d(**bad), 20, 7) == -1
    assert size(d(), 20, 0) == -1 and size(d(), 20, 65) == -1 and size(d(), 1, 1) == -1 and size(d(), 65, 1) == -1
    out = (ctypes.c_int32 * len(couples.GEOM_FIELDS))()
    geo = lib.g2k_couple_scores_geometry
    for args, msg in (((None, 20, out), "dims is NULL"), ((d(Nmax=257), 20, out), "S=2 F=3 Nmax=257"),
                      ((d(), 1, out), "K=1 (2..64)"), ((d(), 65, out), "K=65 (2..64)"),
                      ((d(), 20, None), "out is NULL")):
        assert geo(*args) == EINVAL and lib.g2k_last_error().decode() == msg
    assert geo(d(), 20, out) == OK and geo(d(S=0), 2, out) == OK and geo(d(flags=1), 64, out) == OK


# ---------------------------------------------------------------------------
# the geometry: what tests/couples_cases.py claims, every branch reached
# ---------------------------------------------------------------------------
LDS = {16: 8 * 32 * 24 * 4 + 24 * 256 * 8 + 2 * 256 * 4 + 16 + 2 * 64 * 4 + 4 * 8 * 4 + 64,
       8: 8 * 32 * 24 * 4 + 66 * 128 * 8 + 2 * 256 * 4 + 16 + 2 * 64 * 4 + 4 * 8 * 4 + 64}


def test_geometry_claims_and_branches():
    reached = set()
    for i, case in enumerate(cc.CASES):
        name, S, F, N, K, B = case[:6]
        c = cc.inputs(i)
        g = couples.couple_scores_geometry(S, F, N, K)
        assert {k: g[k] for k in ("tr", "tiles", "w", "passes")} == c["geom"], (name, g)
        assert g["tc"] == 16 and g["dr"] == 8 and g["cp"] == 16 * g["tr"] and g["tr"] == (16 if K <= 22 else 8)
        assert g["tiles"] == len(cc.tiles_of(N, g["tr"])) and g["passes"] == -(-g["tiles"] // g["w"])
        assert g["w"] == max(1, min(8, g["tiles"], -(-2048 // (S * F))))
        # LDS: the items of a round [8][32][24], the cells [K + 2 at most][CP] of 8 bytes, the members'
        # columns and flags, the waves' counts, the histograms and the waves' partial sums; with the
        # mixture head's 19376 bytes inside gfx950's 160 KB
        assert g["lds_bytes"] == LDS[g["tr"]] and g["lds_bytes"] + 19376 <= 160 * 1024
        assert (K + 2) * g["cp"] * 8 <= {16: 24 * 256 * 8, 8: 66 * 128 * 8}[g["tr"]]
        assert (K + 1) % B == 0 and 1 <= B <= 64
        members = c["members"].sum(axis=2)
        worst = cc.passes_of(i)
        reached.add("16-row tiles" if g["tr"] == 16 else "8-row tiles")
        reached.add("several workgroups" if g["w"] > 1 else "one workgroup")
        reached.add("several passes" if worst > 1 else "one pass")
        if g["w"] > 1 and worst > 1:
            reached.add("several passes on several workgroups")
        if g["w"] == 1 and worst > 1:
            reached.add("every tile on one workgroup")
        if 1 < g["w"] < g["tiles"]:
            reached.add("fewer workgroups than tiles")
        reached.add("a full last round" if (K + 2) % 8 == 0 else "a partial last round")
        for Pn in np.unique(members):
            reached.add({0: "P = 0", 1: "P = 1", 2: "P = 2"}.get(int(Pn), "P > 2"))
            if Pn > 2 and Pn % 16 and Pn % 8:
                reached.add("P no multiple of a tile edge")
            if Pn == 256:
                reached.add("P maximum")
            tiles = cc.tiles_of(int(Pn), g["tr"])
            if any(rb * g["tr"] != cb * 16 and rb * g["tr"] + g["tr"] > cb * 16 for rb, cb in tiles if g["tr"] == 8):
                reached.add("rows inside a column block")
            if any(rb * g["tr"] + g["tr"] <= cb * 16 for rb, cb in tiles):
                reached.add("a full tile")
        if any(int(n) == 0 for n in c["n_active"]):
            reached.add("empty scene")
        if c["n_frames"] is not None and (c["n_frames"] < F).any():
            reached.add("n_frames < F")
        if c["ped_mask"] is not None:
            reached.add("masked")
        if c["shared"]:
            reached.add("shared targets")
        reached.add({2: "K minimum", 64: "K maximum"}.get(K, "K between"))
        reached.add("B = K + 1" if B == K + 1 else "B minimum" if B == 1 else "several ranks per bin")
        reached.add("every couple" if np.isinf(c["reach"]) else "finite reach")
    assert reached == {"16-row tiles", "8-row tiles", "several workgroups", "one workgroup", "several passes",
                       "one pass", "several passes on several workgroups", "every tile on one workgroup",
                       "fewer workgroups than tiles", "a full last round", "a partial last round", "P = 0",
                       "P = 1", "P = 2", "P > 2", "P no multiple of a tile edge", "P maximum",
                       "rows inside a column block", "a full tile", "empty scene", "n_frames < F", "masked",
                       "shared targets", "K minimum", "K maximum", "K between", "B = K + 1", "B minimum",
                       "several ranks per bin", "every couple", "finite reach"}, reached
    assert {c[0]: c[4:6] for c in cc.CASES if c[0] in ("k2", "k20", "reach", "k64")} == {
        "k2": (2, 3), "k20": (20, 21), "reach": (20, 7), "k64": (64, 13)}
    n256 = cc.inputs(cc.IDS.index("n256"))
    assert list(n256["members"].sum(axis=2)[:, 0]) == [256, 130] and 256 * 255 // 2 == 32640
    # the tiles cover every couple a < b < P once, whatever P and the tile's height
    for tr in (16, 8):
        for Pn in (2, 7, 8, 9, 16, 17, 24, 25, 33, 130, 256):
            seen = np.zeros((Pn, Pn), int)
            for rb, cb in cc.tiles_of(Pn, tr):
                a = np.arange(rb * tr, min(Pn, rb * tr + tr))[:, None]
                b = np.arange(cb * 16, min(Pn, cb * 16 + 16))[None, :]
                seen[a, b] += (a < b)
            assert np.array_equal(seen, np.triu(np.ones((Pn, Pn), int), 1)), (tr, Pn)
    # the evaluation's two timing shapes (tools/time_couple_scores.py); F = 0
    assert couples.couple_scores_geometry(384, 1, 32, 20) == dict(tr=16, tc=16, cp=256, dr=8, tiles=3, w=3,
                                                                  passes=1, lds_bytes=LDS[16])
    big = couples.couple_scores_geometry(64, 20, 256, 20)
    assert (big["tiles"], big["w"], big["passes"]) == (136, 2, 68)
    assert couples.couple_scores_geometry(3, 0, 16, 20)["w"] == 1


# ---------------------------------------------------------------------------
# the checker against an independent restatement
# ---------------------------------------------------------------------------
def test_checker_against_plain_loops():
    checked = 0
    for name in ("k2", "shared", "k20"):
        i = cc.IDS.index(name)
        c = cc.inputs(i)
        S, F, N = c["members"].shape
        K = c["K"]
        y = np.broadcast_to(c["targets"], (S, F, N, L, 2))
        mu = cr.band_to_xy(c["pred"])
        for which in cc.HEADS:
            draws = cc.oracle_draws(i, which)
            R = cr.couple_scores_ref(draws, c["targets"], c["pred"], c["members"], K, c["B"], c["reach"])
            x = cr.band_to_xy(draws)
            assert R["ties"] == 0
            acc = np.zeros((S, F, 8))
            for s in range(S):
                for f in range(F):
                    idx = np.flatnonzero(c["members"][s, f])
                    for ai, a in enumerate(idx):
                        for b in idx[ai + 1:]:
                            qm = cr.features_loops(mu[s, f, a], mu[s, f, b])[0]
                            scored = np.isinf(c["reach"]) or np.float32(qm) < np.float32(c["reach"]) * np.float32(c["reach"])
                            if not scored:
                                assert R["per_couple"][s, f, a, b] == 0
                                continue
                            w = cr.couple_loops(x[:, s, f, a], x[:, s, f, b], y[s, f, a], y[s, f, b])
                            assert R["per_couple"][s, f, a, b] == 1 + w[0] + 256 * w[1], (name, which, s, f, a, b)
                            acc[s, f] += w[2:]
                            checked += 1
            np.testing.assert_allclose(R["per_frame_f"], acc, rtol=1e-12, atol=1e-12)
            pc = R["per_couple"]
            assert np.all(np.tril(pc.reshape(-1, N, N)) == 0)
            assert int((pc > 0).sum()) == int(R["tot"][:, 0].sum()) == int(R["per_frame_i"][..., 0].sum())
            P = c["members"].sum(axis=2)
            np.testing.assert_array_equal(R["per_frame_i"][..., 3], P * (P - 1) // 2)
            np.testing.assert_array_equal(R["hist"].sum(axis=2), np.stack([R["tot"][:, 0]] * 2, axis=1))
            # |x - y| >= 0 and the triangle inequality: p <= 2 m, so every crps >= 0
            m, p = R["per_frame_f"][..., 0:2], R["per_frame_f"][..., 2:4]
            assert np.all(m >= 0) and np.all(p >= 0) and np.all(p <= 2 * m + 1e-9)
    assert checked >= 300
    # the features: the vectorised restatement is the loops' bit for bit
    rng = np.random.default_rng(3)
    za, zb = (rng.standard_normal((50, L, 2)).astype(np.float32) for _ in range(2))
    qmin, qfin = cr.features(za, zb)
    assert qmin.dtype == np.float32
    for j in range(50):
        assert [float(qmin[j]), float(qfin[j])] == cr.features_loops(za[j], zb[j])


def carry_check(draws_of, c, label):
    """The boundary-seed rows' CPU side: on the restated draws (``draws_of(carry)``)
    no fp32 tie between a draw and the target, and the checker's integer outputs
    change when the draws are made with the carry dropped."""
    R, D = (cr.couple_scores_ref(draws_of(carry), c["targets"], c["pred"], c["members"], c["K"], c["B"], c["reach"])
            for carry in (True, False))
    assert R["ties"] == 0 and D["ties"] == 0 and R["tot"][:, 0].sum() > 0
    moved = np.abs(D["sums"] - R["sums"]).max()
    print(f"{label}: carry dropped, sums move by {moved:.3g}, {int((D['per_couple'] != R['per_couple']).sum())} "
          f"couples' ranks change")
    assert not np.array_equal(D["per_couple"], R["per_couple"]) and not np.array_equal(D["hist"], R["hist"])
    assert moved > 1e-2


@pytest.mark.parametrize("which", cc.HEADS)
@pytest.mark.parametrize("at", BOUNDARY_SEEDS)
def test_boundary_seeds_have_no_ties_and_see_the_carry(at, which):
    """Case k2 at the seeds whose low word carries at draw 1 (tests/bestk_ref.py;
    tests/test_couple_scores_gpu.py runs the kernel there)."""
    i = cc.IDS.index("k2")
    carry_check(lambda carry: cc.oracle_draws(i, which, BOUNDARY_SEEDS[at], carry), cc.inputs(i),
                f"k2 seed {at} {which}")


def _band(xy):
    """[..., N, L, 2] -> [..., 2L, N]."""
    a = np.moveaxis(np.asarray(xy), -3, -1)                         # [..., L, 2, N]
    return np.concatenate([a[..., 0, :], a[..., 1, :]], axis=-2)


def _line(start, step):
    """A constant-velocity trajectory [L, 2] float32."""
    return (np.asarray(start, np.float32)[None] + np.arange(L, dtype=np.float32)[:, None]
            * np.asarray(step, np.float32)[None]).astype(np.float32)


def _two(xa, xb, ya, yb, ma, mb, K, B, reach=INF):
    """One scene-frame of two members from their draws [K, L, 2], targets and means."""
    draws = _band(np.stack([xa, xb], axis=1)[:, None, None])          # [K, 1, 1, 24, 2]
    tg = np.stack([ya, yb])[None, None]
    pred = _band(np.stack([ma, mb])[None, None])
    return cr.couple_scores_ref(draws.astype(np.float32), tg, pred, np.ones((1, 1, 2), bool), K, B, reach)


def test_closed_forms():
    # two walkers that cross: a from (0, 0) east, b from (11, 0) west, one unit a step: they meet
    # between steps 5 and 6 (distance 1), and end 11 apart
    a, b = _line([0, 0], [1, 0]), _line([11, 0], [-1, 0])
    assert cr.features_loops(a, b) == [1.0, 121.0] and [float(v) for v in cr.features(a, b)] == [1.0, 121.0]
    # K = 2 by hand: draw 0 is the crossing (smin 1, sfin 11), draw 1 keeps them 3 apart throughout;
    # the targets stay 2 apart
    a1, b1 = _line([0, 0], [1, 0]), _line([0, 3], [1, 0])
    ya, yb = _line([0, 0], [0, 1]), _line([2, 0], [0, 1])
    R = _two(np.stack([a, a1]), np.stack([b, b1]), ya, yb, a, b, 2, 3)
    assert R["per_couple"][0, 0, 0, 1] == 1 + 1 + 256 * 0 and R["per_couple"][0, 0, 1, 0] == 0
    assert list(R["per_frame_f"][0, 0]) == [1.0, 5.0, 2.0, 8.0, 2.0, 7.0, 2.0, 2.0]
    assert list(R["per_frame_i"][0, 0]) == [1, 1, 0, 1] and list(R["tot"][0]) == [1, 1, 0, 1]
    assert R["hist"].tolist() == [[[0, 1, 0], [1, 0, 0]]]
    w = cr.couple_loops(np.stack([a, a1]), np.stack([b, b1]), ya, yb)
    assert w == [1, 0, 1.0, 5.0, 2.0, 8.0, 2.0, 7.0, 2.0, 2.0]
    fig = cr.figures(R["sums"], R["hist"], R["tot"], 2)
    assert fig["couples"] == 1 and fig["min"]["crps"] == 0.0 and fig["fin"]["crps"] == 1.0
    assert fig["min"]["pit_mean"] == 0.5 and fig["fin"]["pit_mean"] == pytest.approx(1 / 6)
    # K identical draws: p = 0, d the draw's own feature, every rank 0 or K
    K = 5
    R = _two(np.stack([a] * K), np.stack([b] * K), ya, yb, a, b, K, 6)
    assert list(R["per_frame_f"][0, 0]) == [1.0, 9.0, 0.0, 0.0, 1.0, 11.0, 2.0, 2.0]
    assert R["per_couple"][0, 0, 0, 1] == 1 + K + 256 * 0
    # a target equal to a draw: that draw is not counted by <
    R = _two(np.stack([a, a1, a1]), np.stack([b, b1, b1]), a, b, a, b, 3, 4)
    assert R["per_couple"][0, 0, 0, 1] == 1 + 0 + 256 * 2 and R["ties"] == 2   # fin: the two others end closer
    R = _two(np.stack([a, a1, a1]), np.stack([b, b1, b1]), a1, b1, a, b, 3, 4)
    assert R["per_couple"][0, 0, 0, 1] == 1 + 1 + 256 * 0 and R["ties"] == 4     # only the crossing comes closer
    # reach: the means' closest approach is 1: scored at reach 1.5, not at 1 (strict) nor below
    for reach, n in ((1.5, 1), (1.0, 0), (0.5, 0), (INF, 1)):
        R = _two(np.stack([a, a1]), np.stack([b, b1]), ya, yb, a, b, 2, 3, reach)
        assert R["tot"][0, 0] == n and R["tot"][0, 3] == 1 and (R["sums"].any() == bool(n))
    # one member: no couple
    R = cr.couple_scores_ref(np.zeros((2, 1, 1, 24, 3), np.float32), np.zeros((1, 1, 3, L, 2), np.float32),
                             np.zeros((1, 1, 24, 3), np.float32), np.array([[[False, True, False]]]), 2, 3)
    assert not R["tot"].any() and not R["per_couple"].any()


@pytest.mark.parametrize("K,B", [(20, 21), (20, 7), (64, 13), (2, 3), (3, 1)])
def test_bin_edges_and_the_result_class(K, B):
    """Every rank 0..K once: (K + 1) / B in each bin; the result class's
    figures on hand-made counts."""
    w = (K + 1) // B
    r = np.arange(K + 1)
    hist = np.stack([np.bincount(r * B // (K + 1), minlength=B)] * 2)[None]
    assert np.all(hist == w)
    n = K + 1
    tot = np.array([[n, r.sum(), r.sum(), 2 * n]], np.int64)
    sums = n * (np.arange(8, dtype=np.float64)[None] + 1)
    cs = couples.CoupleScores(sums=torch.from_numpy(sums.astype(np.float32)), hist=torch.from_numpy(hist.astype(np.int32)),
                              tot=torch.from_numpy(tot), per_couple=None, per_frame_f=None, per_frame_i=None,
                              k=K, bins=B)
    assert cs.couples == n and cs.member_couples == 2 * n and cs.counts().shape == (2, B)
    want = cr.figures(sums, hist, tot, K)
    for gi, g in enumerate(couples.FEATURES):
        assert cs.dev(g) == 0.0 and cs.pit_mean(g) == pytest.approx(0.5, abs=1e-15)
        assert cs.crps(g) == pytest.approx((gi + 1) - 0.5 * (gi + 3)) and cs.draw_mean(g) == pytest.approx(gi + 5)
        assert cs.target_mean(g) == pytest.approx(gi + 7)
        for name, fn in (("crps", cs.crps), ("pit_mean", cs.pit_mean), ("dev", cs.dev), ("draw_mean", cs.draw_mean),
                         ("target_mean", cs.target_mean)):
            assert fn(g) == pytest.approx(want[g][name], abs=1e-12)
    hist[:] = 0
    hist[:, :, B - 1] = n
    cs.hist = torch.from_numpy(hist.astype(np.int32))
    assert cs.dev("fin") == pytest.approx(1.0 - 1.0 / B)
    empty = couples.CoupleScores(sums=torch.zeros((2, 8)), hist=torch.zeros((2, 2, B), dtype=torch.int32),
                                 tot=torch.zeros((2, 4), dtype=torch.int64), per_couple=None, per_frame_f=None,
                                 per_frame_i=None, k=K, bins=B)
    assert empty.couples == 0
    for g in couples.FEATURES:
        assert all(np.isnan(v) for v in (empty.crps(g), empty.pit_mean(g), empty.dev(g), empty.draw_mean(g),
                                         empty.target_mean(g)))
    with pytest.raises(ValueError, match="one of min, fin"):
        cs.crps("mean")


def test_python_argument_checks():
    for k in (1, 65):
        with pytest.raises(ValueError, match="2..64"):
            couples.check_k_bins(k, None)
    for b in (4, 65, -1):
        with pytest.raises(ValueError, match="a divisor of k \\+ 1"):
            couples.check_k_bins(20, b)
    assert couples.check_k_bins(20, None) == (20, 21) and couples.check_k_bins(20, 0) == (20, 21)
    assert couples.check_k_bins(64, None) == (64, 13) and couples.check_k_bins(2, None) == (2, 3)
    assert couples.check_k_bins(63, 64) == (63, 64) and couples.check_k_bins(3, 1) == (3, 1)
    assert couples.check_reach(None) == INF and couples.check_reach(INF) == INF and couples.check_reach(2) == 2.0
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="reach"):
            couples.check_reach(bad)


# ---------------------------------------------------------------------------
# what the scores are for: dependence between pedestrians, which no
# per-pedestrian score sees
# ---------------------------------------------------------------------------
PROP = dict(S=4, F=4, N=32, K=20, B=7, seed=4242, sigma=0.5, share=0.8, side=4.0)
# matched: both dev below 0.08 (the five-seed range 0.007..0.034 times 2.3); coupled: dev_fin above 0.2
# (0.28..0.31 over 1.4), dev_min above 0.1 (0.14..0.15 over 1.4), crps_fin below the matched one
DEV_MATCHED, DEV_FIN, DEV_MIN = 0.08, 0.2, 0.1


def property_head():
    head = np.zeros((3, L), np.float32)
    head[:2] = np.float32(np.log(PROP["sigma"]))
    return head


def property_check(score, label=""):
    """``score(kind)`` -> dict feature -> dict(dev, crps, pit_mean) of the
    "matched" targets (one more draw of the head's own independent law) and of
    the "coupled" ones (the same marginals, 80 % of the residual variance
    shared by the pedestrians of a scene-frame) under the per-step head's K
    joint draws."""
    m, c = score("matched"), score("coupled")
    for kind, v in (("matched", m), ("coupled", c)):
        print(f"{label}{kind}: " + ", ".join(f"{g} dev {v[g]['dev']:.4f} crps {v[g]['crps']:.4f} pit "
                                             f"{v[g]['pit_mean']:.4f}" for g in cr.FEATURES))
    assert m["min"]["dev"] < DEV_MATCHED and m["fin"]["dev"] < DEV_MATCHED
    assert c["fin"]["dev"] > DEV_FIN and c["min"]["dev"] > DEV_MIN
    assert c["fin"]["crps"] < m["fin"]["crps"]


def property_targets(pred, kind):
    """[S, F, N, L, 2] float32."""
    if kind == "matched":
        y = ref.gauss_sample(pred, property_head(), PROP["seed"] + PROP["K"])
        return cr.band_to_xy(np.asarray(y, np.float32)).astype(np.float32)
    return cc.coupled_targets(pred, PROP["sigma"], PROP["share"], rng_seed=PROP["seed"])


def test_coupled_targets_are_told_apart():
    S, F, N, K, B, seed = (PROP[k] for k in ("S", "F", "N", "K", "B", "seed"))
    pred = cc.property_setup(S, F, N, PROP["side"])
    members = np.ones((S, F, N), bool)
    draws = np.stack([ref.gauss_sample(pred, property_head(), seed + k) for k in range(K)]).astype(np.float32)
    # the marginals of the two sets of targets are the same law: the residuals' spread agrees
    mu = cr.band_to_xy(pred)
    sd = {k: float((property_targets(pred, k) - mu).std()) for k in ("matched", "coupled")}
    assert abs(sd["matched"] - 0.5) < 0.01 and abs(sd["coupled"] - 0.5) < 0.03

    def score(kind):
        R = cr.couple_scores_ref(draws, property_targets(pred, kind), pred, members, K, B)
        assert R["tot"][:, 0].sum() == S * F * N * (N - 1) // 2
        fig = cr.figures(R["sums"], R["hist"], R["tot"], K)
        return {g: fig[g] for g in cr.FEATURES}
    property_check(score)


# ---------------------------------------------------------------------------
# the evaluation's flags
# ---------------------------------------------------------------------------
def test_evaluation_flags():
    from multimodaltraj_2_amd import evaluate
    from multimodaltraj_2_amd.argParser import ArgsParser
    a = ArgsParser().parser.parse_args([])
    assert a.couple_scores == 0 and a.couple_bins == 0 and a.couple_reach == 0.0
    a = ArgsParser().parser.parse_args(["--num_samples", "20", "--couple_scores", "1", "--couple_bins", "7",
                                        "--couple_reach", "1.5"])
    assert a.couple_scores == 1 and a.couple_bins == 7 and a.couple_reach == 1.5
    with pytest.raises(SystemExit):
        ArgsParser().parser.parse_args(["--couple_scores", "2"])
    assert evaluate.CPL_FIGURES == ("cpl_couples",) + tuple(
        f"cpl_{f}_{g}" for f in ("crps", "pit", "dev", "draw", "target") for g in ("min", "fin"))
    assert len(evaluate.CPL_FIGURES) == 11
    assert evaluate.FULLCOV_CPL_FIGURES == tuple("fullcov_" + k for k in evaluate.CPL_FIGURES)
    assert evaluate.MIX_CPL_FIGURES == tuple("mix_" + k for k in evaluate.CPL_FIGURES)
    # refused before any data is read or any launch made
    for k, b, reach, word in ((1, 0, 0.0, "2 <= K <= 64"), (65, 0, 0.0, "2 <= K <= 64"), (20, 4, 0.0, "--couple_bins"),
                              (20, 65, 0.0, "--couple_bins"), (20, 0, -1.0, "--couple_reach")):
        a.num_samples, a.couple_bins, a.couple_reach = k, b, reach
        with pytest.raises(ValueError, match=word):
            evaluate.evaluate_best_of_k(a, None, None, log=lambda s: None)
    # the figures of a result, in the stated order, on hand-made counts
    hist = np.full((1, 2, 7), 3, np.int32)
    tot = np.array([[21, 210, 210, 30]], np.int64)
    sums = 21.0 * (np.arange(8, dtype=np.float32)[None] + 1)
    cs = couples.CoupleScores(sums=torch.from_numpy(sums), hist=torch.from_numpy(hist), tot=torch.from_numpy(tot),
                              per_couple=None, per_frame_f=None, per_frame_i=None, k=20, bins=7)
    for prefix, names in (("", evaluate.CPL_FIGURES), ("fullcov_", evaluate.FULLCOV_CPL_FIGURES),
                          ("mix_", evaluate.MIX_CPL_FIGURES)):
        fig = evaluate.couple_figures(cs, prefix)
        assert tuple(fig) == names
        assert fig[prefix + "cpl_couples"] == 21 and fig[prefix + "cpl_dev_fin"] == 0.0
        assert fig[prefix + "cpl_pit_min"] == pytest.approx(0.5) and fig[prefix + "cpl_crps_fin"] == pytest.approx(2 - 2.0)
        assert fig[prefix + "cpl_draw_min"] == 5.0 and fig[prefix + "cpl_target_fin"] == 8.0
