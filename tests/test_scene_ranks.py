"""CPU: the scene-level rank calibration (include/g2k_scene_ranks.h,
multimodaltraj_2_amd/sceneranks.py, csrc/g2k_scene_ranks.hip) — the header, the
module's binding table and the library's exports agree; every validator rejects
bad arguments before touching the GPU; the launch geometry is what
tests/scene_ranks_cases.py claims, every branch of it reached; the checker
tests/scene_ranks_ref.py alone: against plain loops, closed forms, its own rank
intervals; and the reason the figures exist — the joint draws of a fitted
scene-coupled head rank a scene's targets uniformly, those of a full-covariance
head with the same marginals do not, and the ranks say in which direction."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib, coupled, couples, kin, mixture, modes, ranks, sceneranks, scores
from multimodaltraj_2_amd import build as g2k_build
from tests import coupled_ref as cor
from tests import couples_cases as cc
from tests import fullcov_ref as fr
from tests import scene_ranks_cases as sc
from tests import scene_ranks_ref as sr
from tests.bestk_ref import BOUNDARY_SEEDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2k_scene_ranks.h")
P = 0x10000                    # a non-NULL pointer, 64-byte aligned (never dereferenced)
OK, EINVAL, EUNSUPPORTED = 0, -1, -4
ENTRIES = (("g2k_scene_ranks_f32", "scene_ranks"), ("g2k_fullcov_scene_ranks_f32", "fullcov_scene_ranks"),
           ("g2k_mix_scene_ranks_f32", "mix_scene_ranks"))
L = 12


def _declarations():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(g2k_[a-z0-9_]+)\s*\(([^)]*)\)", src)}


# ---------------------------------------------------------------------------
# the header, the binding and the exports
# ---------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    decl = _declarations()
    assert sorted(decl) == sorted(sceneranks.SYMBOLS)
    for name, args in decl.items():
        assert len(args.split(",")) == len(sceneranks.SYMBOLS[name][1]), name
    # by symbol, after ABI 11: in no other header or table
    for table in (_lib.SYMBOLS, mixture.SYMBOLS, scores.SYMBOLS, modes.SYMBOLS, ranks.SYMBOLS, kin.SYMBOLS,
                  couples.SYMBOLS, coupled.SYMBOLS):
        assert not set(decl) & set(table)
    for other in ("g2k_hip.h", "g2k_mix.h", "g2k_scores.h", "g2k_modes.h", "g2k_ranks.h", "g2k_kin.h",
                  "g2k_couples.h"):
        assert "scene_ranks" not in open(os.path.join(ROOT, "include", other)).read()
    assert "g2k_coupled_" not in open(HEADER).read()
    # the scene-coupled head's twin: declared in its own header, bound by coupled.py, the same signature
    csrc = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "g2k_coupled.h")).read(), flags=re.S)
    twin = re.search(r"\bg2k_coupled_scene_ranks_f32\s*\(([^)]*)\)", csrc).group(1)
    norm = lambda a: [" ".join(p.split()) for p in a.replace("cpl", "chol").split(",")]
    assert norm(twin) == norm(decl["g2k_fullcov_scene_ranks_f32"])
    assert coupled.SYMBOLS["g2k_coupled_scene_ranks_f32"] is sceneranks.SYMBOLS["g2k_fullcov_scene_ranks_f32"]
    lib = sceneranks.load()
    for name, (res, args) in sceneranks.SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.g2k_abi_version() == _lib.ABI_VERSION == 11
    assert sceneranks.load() is lib
    assert list(coupled.load().g2k_coupled_scene_ranks_f32.argtypes) == sceneranks._SCN[1]
    src = open(HEADER).read()
    for macro, value in (("KMIN", sceneranks.KMIN), ("KMAX", sceneranks.KMAX), ("BMAX", sceneranks.BMAX),
                         ("FEATURES", len(sceneranks.FEATURES)), ("SUMS", sceneranks.NSUMS),
                         ("TOT", sceneranks.NTOT)):
        assert int(re.search(rf"G2K_SCENE_RANKS_{macro} (\d+)", src).group(1)) == value
    assert (sceneranks.KMIN, sceneranks.KMAX, sceneranks.BMAX) == (sr.K_MIN, sr.K_MAX, sr.B_MAX) == (2, 64, 64)
    assert sceneranks.FEATURES == sr.FEATURES == ("typ", "loc", "spr")
    assert int(re.search(r"G2K_SCENE_RANKS_GEOM_FIELDS (\d+)", src).group(1)) == len(sceneranks.GEOM_FIELDS)
    for i, f in enumerate(sceneranks.GEOM_FIELDS):
        assert int(re.search(rf"G2K_SCENE_RANKS_GEOM_{f.upper()} (\d+)", src).group(1)) == i
    assert ("Alignment (bytes) of g2k_scene_ranks_f32, g2k_fullcov_scene_ranks_f32 and\n"
            " * g2k_mix_scene_ranks_f32: targets 8, per_frame_i 4, per_frame_d 8, sums 8,\n"
            " * hist 4, tot 8, workspace 8.") in src
    assert HEADER in [os.path.abspath(p) for p in g2k_build.HDR]    # hashed, and a change rebuilds


# ---------------------------------------------------------------------------
# the validators: before any HIP call
# ---------------------------------------------------------------------------
DIMS = dict(S=2, F=3, T=8, L=12, D=16, H=64, Nmax=5, W=8, stride=0, flags=0)
NEED = 2 * 3 * 64                        # S * F scene-frames, a row of 64 bytes each
ARGS = dict(pred=P, targets=2 * P, n_active=3 * P, n_frames=None, ped_mask=None, head=6 * P, seed=7, K=20,
            B=7, per_frame_i=13 * P, per_frame_d=12 * P, sums=11 * P, hist=8 * P, tot=10 * P, ws=9 * P,
            ws_bytes=NEED, stream=None)
FLAGS = "{name}: flags %d (0 or G2K_STEP_TARGETS_SHARED)"
NULL = "a required buffer pointer is NULL"


def _align(name, base, n):
    return (name, [({name: base + n - 1}, EINVAL, f"{name} must be {n}-byte aligned"),
                   ({name: base + n // 2}, EINVAL, f"{name} must be {n}-byte aligned")])


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
    ("required", [({n: None}, EINVAL, NULL) for n in ("pred", "targets", "n_active", "head", "sums", "hist",
                                                      "tot")]),
    ("targets", [({"targets": 2 * P + 7}, EINVAL, "targets must be 8-byte aligned"),
                 ({"targets": 2 * P + 4}, EINVAL, "targets must be 8-byte aligned")]),
    _align("per_frame_i", 13 * P, 4), _align("per_frame_d", 12 * P, 8), _align("sums", 11 * P, 8),
    _align("hist", 8 * P, 4), _align("tot", 10 * P, 8),
    ("ws_align", [({"ws": 9 * P + 7}, EINVAL, "workspace must be 8-byte aligned"),
                  ({"ws": 9 * P + 4}, EINVAL, "workspace must be 8-byte aligned")]),
    ("ws_size", [({"ws_bytes": NEED - 1}, EINVAL, f"workspace of {NEED} bytes needed (got {NEED - 1})"),
                 ({"ws": None}, EINVAL, f"workspace of {NEED} bytes needed (got {NEED})"),
                 ({"ws_bytes": 0}, EINVAL, f"workspace of {NEED} bytes needed (got 0)")]),
]
# what returns G2K_OK without a launch, at the weakest alignments the header states
SUCCESSES = ({"S": 0}, {"S": 0, "ws": None, "ws_bytes": 0}, {"S": 0, "F": 0, "ws_bytes": 0},
             {"S": 0, "flags": 2}, {"S": 0, "K": 64, "B": 65 // 5}, {"S": 0, "K": 2, "B": 3},
             {"S": 0, "per_frame_i": None, "per_frame_d": None},
             {"S": 0, "targets": 2 * P + 8, "per_frame_i": 13 * P + 4, "per_frame_d": 12 * P + 8,
              "sums": 11 * P + 8, "hist": 8 * P + 4, "tot": 10 * P + 8, "ws": 9 * P + 8, "pred": P + 4,
              "head": 6 * P + 4})
REFUSALS = (({"S": 0, "flags": 4}, EUNSUPPORTED, FLAGS % 4), ({"S": 0, "K": 1, "B": 1}, EINVAL, "K=1 (2..64)"),
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
def test_each_fault_alone_and_in_order(symbol, name, lib=None):
    lib = lib or sceneranks.load()
    for label, ways in CHECKS:
        for faults, code, message in ways:
            assert _call(lib, symbol, faults) == (code, message.format(name=name)), (label, faults)
    # every adjacent pair of checks, both faults present: the earlier check's report
    for (label, first), (label2, second) in zip(CHECKS[1:], CHECKS[2:]):
        faults, code, message = first[0]
        both = dict(second[0][0], **faults)
        assert _call(lib, symbol, both) == (code, message.format(name=name)), (label, label2)


@pytest.mark.parametrize("symbol,name", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_successes_that_launch_nothing(symbol, name, lib=None):
    lib = lib or sceneranks.load()
    for faults in SUCCESSES:
        rc_, msg = _call(lib, symbol, faults)
        assert rc_ == OK, (faults, msg)
    for faults, code, message in REFUSALS:
        assert _call(lib, symbol, faults) == (code, message.format(name=name)), faults


def test_the_coupled_entry_point_faults_like_its_twin():
    """g2k_coupled_scene_ranks_f32 under the whole table of faults, successes
    and refusals, and fault for fault g2k_fullcov_scene_ranks_f32's report."""
    lib = coupled.load()
    sceneranks.load()
    test_each_fault_alone_and_in_order("g2k_coupled_scene_ranks_f32", "coupled_scene_ranks", lib)
    test_successes_that_launch_nothing("g2k_coupled_scene_ranks_f32", "coupled_scene_ranks", lib)
    for label, ways in CHECKS:
        for faults, code, message in ways:
            got = _call(lib, "g2k_coupled_scene_ranks_f32", faults)
            want = _call(lib, "g2k_fullcov_scene_ranks_f32", faults)
            assert got == (want[0], want[1].replace("fullcov_", "coupled_")), (label, faults)


def test_workspace_bytes_and_geometry_queries():
    lib = sceneranks.load()
    size = lib.g2k_scene_ranks_workspace_bytes

    def d(**kw):
        return ctypes.byref(_lib.G2KDims(**dict(DIMS, **kw)))
    assert size(d(), 20, 7) == NEED == 384 and size(d(), 20, 1) == NEED and size(d(), 63, 64) == NEED
    assert size(d(F=0), 20, 7) == 2 * 64 and size(d(S=0), 20, 7) == 0
    assert size(d(Nmax=256), 20, 7) == NEED              # one workgroup per scene-frame whatever P
    assert size(None, 20, 7) == -1
    for bad in (dict(Nmax=0), dict(Nmax=257), dict(S=-1), dict(F=-1)):
        assert size(d(**bad), 20, 7) == -1
    assert size(d(), 20, 0) == -1 and size(d(), 20, 65) == -1 and size(d(), 1, 1) == -1 and size(d(), 65, 1) == -1
    out = (ctypes.c_int32 * len(sceneranks.GEOM_FIELDS))()
    geo = lib.g2k_scene_ranks_geometry
    for args, msg in (((None, 20, out), "dims is NULL"), ((d(Nmax=257), 20, out), "S=2 F=3 Nmax=257"),
                      ((d(), 1, out), "K=1 (2..64)"), ((d(), 65, out), "K=65 (2..64)"),
                      ((d(), 20, None), "out is NULL")):
        assert geo(*args) == EINVAL and lib.g2k_last_error().decode() == msg
    assert geo(d(), 20, out) == OK and geo(d(S=0), 2, out) == OK and geo(d(flags=1), 64, out) == OK


# ---------------------------------------------------------------------------
# the geometry: what tests/scene_ranks_cases.py claims, every branch reached
# ---------------------------------------------------------------------------
def test_geometry_claims_and_branches():
    reached = set()
    for i, case in enumerate(sc.CASES):
        name, S, F, N, K, B = case[:6]
        c = sc.inputs(i)
        g = sceneranks.scene_ranks_geometry(S, F, N, K)
        assert g == sc.geometry(N, K) and g["tm"] == c["tm"], (name, g)
        # a tile's items fit the 520 slots; what goes over them at the end fits too; with the mixture
        # head's 19376 bytes two workgroups fit gfx950's 160 KB
        assert g["tm"] * (K + 1) <= 520 and (g["pairs"] + 29 * (K + 1)) * 8 <= 520 * 28 * 4
        assert 2 * (g["lds_bytes"] + 19376) <= 160 * 1024
        assert (K + 1) % B == 0 and 1 <= B <= 64
        members = c["members"].sum(axis=2)
        reached.add("16-member tiles" if g["tm"] == 16 else "8-member tiles")
        reached.add("one pair a lane" if g["apt"] == 1 else "several pairs a lane")
        if g["apt"] == 9 and g["aft"] == 7:
            reached.add("the most accumulators a lane")
        if g["pairs"] % 256:
            reached.add("lanes without a pair in the last deal")
        reached.add("one round" if K + 1 <= g["dr"] else "a partial last round" if (K + 1) % g["dr"]
                    else "full rounds")
        for Pn in np.unique(members):
            Pn = int(Pn)
            reached.add({0: "P = 0", 1: "P = 1", 2: "P = 2"}.get(Pn, "P > 2"))
            if Pn > g["tm"]:
                reached.add("several tiles")
            if Pn > g["tm"] and Pn % g["tm"]:
                reached.add("a partial last tile")
            if Pn % g["tm"] == 1 and Pn > 1:
                reached.add(f"P one more than a tile of {g['tm']}")
            if Pn and Pn % g["tm"] == 0:
                reached.add(f"P a multiple of {g['tm']}")
            if Pn == 256:
                reached.add("P maximum")
        if c["n_frames"] is not None and (c["n_frames"] < F).any():
            reached.add("n_frames < F")
        if c["ped_mask"] is not None:
            reached.add("masked")
        if c["shared"]:
            reached.add("shared targets")
        reached.add({2: "K minimum", 64: "K maximum", 31: "K = 31", 32: "K = 32"}.get(K, "K between"))
    assert reached == {"16-member tiles", "8-member tiles", "one pair a lane", "several pairs a lane",
                       "the most accumulators a lane", "lanes without a pair in the last deal", "one round",
                       "a partial last round", "full rounds", "P = 0", "P = 1", "P = 2", "P > 2", "several tiles",
                       "a partial last tile", "P one more than a tile of 16", "P one more than a tile of 8",
                       "P a multiple of 16", "P a multiple of 8", "P maximum", "n_frames < F", "masked",
                       "shared targets", "K minimum", "K maximum", "K = 31", "K = 32", "K between"}, reached
    k20 = sc.inputs(sc.IDS.index("k20"))
    assert sorted(set(k20["members"].sum(axis=2).ravel())) == [0, 16, 17, 27]
    assert sorted(set(sc.inputs(0)["members"].sum(axis=2).ravel())) == [0, 1, 2, 8]
    # the timing shapes (tools/time_scene_ranks.py); F = 0
    assert sceneranks.scene_ranks_geometry(384, 1, 32, 20) == sc.geometry(32, 20)
    assert sceneranks.scene_ranks_geometry(64, 20, 256, 20)["tiles"] == 16
    assert sceneranks.scene_ranks_geometry(3, 0, 16, 20)["w"] == 1


# ---------------------------------------------------------------------------
# the checker against an independent restatement
# ---------------------------------------------------------------------------
def test_checker_against_plain_loops():
    checked = 0
    for name in ("k2", "shared"):
        i = sc.IDS.index(name)
        c = sc.inputs(i)
        S, F, N = c["members"].shape
        K = c["K"]
        y = np.broadcast_to(c["targets"], (S, F, N, L, 2)).reshape(S, F, N, 24)
        mu = sr.band_to_items(c["pred"])
        for which in (sc.HEADS if name == "k2" else ("coupled",)):
            x = sr.band_to_items(sc.oracle_draws(i, which))
            R = sr.scene_ranks_ref(sc.oracle_draws(i, which), c["targets"], c["pred"], c["members"], K, c["B"])
            assert R["ties"] == 0 and R["wide"] == 0
            for s in range(S):
                for f in range(F if name == "k2" else 1):
                    idx = np.flatnonzero(c["members"][s, f])
                    if len(idx) < 2:
                        assert not R["per_frame_i"][s, f].any() and not R["per_frame_d"][s, f].any()
                        continue
                    Z = [x[k, s, f, idx] for k in range(K)] + [y[s, f, idx]]
                    w = sr.frame_loops(Z, mu[s, f, idx])
                    np.testing.assert_allclose(R["per_frame_d"][s, f], w[:6], rtol=1e-12, atol=1e-12)
                    assert list(R["per_frame_i"][s, f]) == [len(idx)] + w[6:], (name, which, s, f)
                    checked += 1
            h, t = sr.recount(R["per_frame_i"], K, c["B"])
            np.testing.assert_array_equal(h, R["hist"])
            np.testing.assert_array_equal(t, R["tot"])
            np.testing.assert_array_equal(R["hist"].sum(axis=2), np.stack([R["tot"][:, 0]] * 3, axis=1))
            # m, p >= 0 and the triangle inequality: p <= 2 m, so the energy score >= 0; spr >= 0
            pd = R["per_frame_d"]
            assert np.all(pd >= 0) and np.all(pd[..., 1] <= 2 * pd[..., 0] + 1e-9)
    assert checked >= 12


def _one(Z, M, K, B):
    """One scene-frame from items Z [K + 1, P, 24] and means M [P, 24]."""
    Z, M = np.asarray(Z, np.float32), np.asarray(M, np.float32)
    Pn = Z.shape[1]
    band = lambda a: np.concatenate([a[..., 0::2], a[..., 1::2]], axis=-1).swapaxes(-1, -2)   # [..., 24, P]
    draws = band(Z[:K])[:, None, None]
    tg = Z[K].reshape(1, 1, Pn, L, 2)
    return sr.scene_ranks_ref(draws, tg, band(M)[None, None], np.ones((1, 1, Pn), bool), K, B)


def test_closed_forms():
    # two members, K = 2, means 0.  Draw 0: both members at +1 in coordinate 0 (pure common mode);
    # draw 1: +1 and -1 (pure spread); targets: +2 and +2
    Z = np.zeros((3, 2, 24))
    Z[0, :, 0] = 1.0
    Z[1, 0, 0], Z[1, 1, 0] = 1.0, -1.0
    Z[2, :, 0] = 2.0
    R = _one(Z, np.zeros((2, 24)), 2, 3)
    # D(0,1) = 2, D(0,2) = sqrt 2, D(1,2) = sqrt 10; loc = {2, 0, 8}; spr = {0, 2, 0}
    m, p = (np.sqrt(2) + np.sqrt(10)) / 2, 2.0
    np.testing.assert_allclose(R["per_frame_d"][0, 0], [m, p, 1.0, 8.0, 1.0, 0.0], rtol=1e-15)
    # typ = {2 + sqrt 2, 2 + sqrt 10, sqrt 2 + sqrt 10}: the targets are above draw 0 only
    assert list(R["per_frame_i"][0, 0]) == [2, 1, 2, 0] and list(R["tot"][0]) == [1, 1, 2, 0]
    assert R["hist"].tolist() == [[[0, 1, 0], [0, 0, 1], [1, 0, 0]]]
    fig = sr.figures(R["sums"], R["hist"], R["tot"], 2)
    assert fig["frames"] == 1 and fig["es"] == pytest.approx(m - 1.0)
    assert fig["loc"]["pit"] == pytest.approx(2.5 / 3) and fig["spr"]["pit"] == pytest.approx(0.5 / 3)
    assert fig["loc"]["draw"] == 1.0 and fig["loc"]["target"] == 8.0 and fig["spr"]["target"] == 0.0
    # the features are of the RESIDUALS: shifting the means and every item alike changes nothing
    # (small integers: every operation stays exact)
    M = np.random.default_rng(1).integers(-4, 5, (2, 24)).astype(np.float64)
    R2 = _one(Z + M[None], M, 2, 3)
    np.testing.assert_array_equal(R2["per_frame_i"], R["per_frame_i"])
    np.testing.assert_array_equal(R2["per_frame_d"], R["per_frame_d"])
    # a target equal to a draw is not counted by <, and the interval says that it is a tie
    Z[2] = Z[0]
    R = _one(Z, np.zeros((2, 24)), 2, 3)
    assert list(R["per_frame_i"][0, 0]) == [2, 0, 1, 0] and R["ties"] == 3 and R["wide"] == 3
    assert list(R["lo"][0, 0]) == [0, 1, 0] and list(R["hi"][0, 0]) == [1, 2, 1]
    # one member: not scored
    R = sr.scene_ranks_ref(np.zeros((2, 1, 1, 24, 3), np.float32), np.zeros((1, 1, 3, L, 2), np.float32),
                           np.zeros((1, 1, 24, 3), np.float32), np.array([[[False, True, False]]]), 2, 3)
    assert not R["tot"].any() and not R["per_frame_i"].any() and not R["sums"].any()


def test_the_checker_alone_meets_the_interval_condition():
    """On every case and head the restated samplers' draws leave no rank whose
    interval holds more than one value (the GPU test fails as untestable above
    1 in 1000)."""
    n = 0
    for i in range(len(sc.CASES)):
        c = sc.inputs(i)
        for which in sc.HEADS:
            R = sr.scene_ranks_ref(sc.oracle_draws(i, which), c["targets"], c["pred"], c["members"], c["K"], c["B"])
            assert R["wide"] == 0 and R["ties"] == 0, (sc.IDS[i], which, R["wide"])
            assert R["ranks"] == 3 * int((c["members"].sum(axis=2) >= 2).sum())
            assert np.isfinite(R["per_frame_d"]).all()                  # the poison was never read
            n += R["ranks"]
    assert n == 4 * 3 * 21


@pytest.mark.parametrize("at,which,row", sc.BOUNDARY, ids=sc.BOUNDARY_IDS)
def test_boundary_seeds_meet_the_interval_condition_and_see_the_carry(at, which, row):
    """Case k2 (k20 where tests/scene_ranks_cases.py says why) at the seeds whose
    low word carries at draw 1 (tests/bestk_ref.py; tests/test_scene_ranks_gpu.py
    runs the kernel there): the interval condition as above, and the checker's
    integer outputs change when draw 1 is made with the carry dropped — the GPU
    test would see a kernel that dropped it."""
    i, seed = sc.IDS.index(row), BOUNDARY_SEEDS[at]
    c = sc.inputs(i)
    R = sr.scene_ranks_ref(sc.oracle_draws(i, which, seed), c["targets"], c["pred"], c["members"], c["K"], c["B"])
    assert R["wide"] == 0 and R["ties"] == 0 and R["ranks"] == 3 * int((c["members"].sum(axis=2) >= 2).sum())
    assert np.isfinite(R["per_frame_d"]).all()
    D = sr.scene_ranks_ref(sc.oracle_draws(i, which, seed, carry=False), c["targets"], c["pred"], c["members"],
                           c["K"], c["B"])
    assert D["wide"] == 0 and D["ties"] == 0
    moved = np.abs(D["sums"] - R["sums"]).max()
    print(f"seed {at} {which}: carry dropped, sums move by {moved:.3g}, "
          f"{int((D['per_frame_i'] != R['per_frame_i']).sum())} ranks change")
    assert not (np.array_equal(D["per_frame_i"], R["per_frame_i"]) and np.array_equal(D["hist"], R["hist"])
                and np.array_equal(D["tot"], R["tot"]))
    assert moved > 1e-2


@pytest.mark.parametrize("K,B", [(20, 21), (20, 7), (64, 13), (2, 3), (3, 1)])
def test_bin_edges_and_the_result_class(K, B):
    """Every rank 0..K once: (K + 1) / B in each bin; the result class's
    figures on hand-made counts."""
    r = np.arange(K + 1)
    hist = np.stack([np.bincount(r * B // (K + 1), minlength=B)] * 3)[None]
    assert np.all(hist == (K + 1) // B)
    n = K + 1
    tot = np.array([[n, r.sum(), r.sum(), r.sum()]], np.int64)
    sums = n * (np.arange(6, dtype=np.float64)[None] + 1)
    res = sceneranks.SceneRanks(sums=torch.from_numpy(sums), hist=torch.from_numpy(hist.astype(np.int32)),
                                tot=torch.from_numpy(tot), per_frame_i=None, per_frame_d=None, k=K, bins=B)
    assert res.frames == n and res.counts().shape == (3, B)
    want = sr.figures(sums, hist, tot, K)
    assert res.es == pytest.approx(1 - 0.5 * 2) and res.es == pytest.approx(want["es"], abs=1e-12)
    for g in sceneranks.FEATURES:
        assert res.dev(g) == 0.0 and res.pit(g) == pytest.approx(0.5, abs=1e-15)
        assert res.dev(g) == want[g]["dev"] and res.pit(g) == pytest.approx(want[g]["pit"], abs=1e-15)
    assert (res.draw("loc"), res.target("loc"), res.draw("spr"), res.target("spr")) == (3.0, 4.0, 5.0, 6.0)
    assert res.draw("spr") == want["spr"]["draw"] and res.target("loc") == want["loc"]["target"]
    hist[:] = 0
    hist[:, :, B - 1] = n
    res.hist = torch.from_numpy(hist.astype(np.int32))
    assert res.dev("spr") == pytest.approx(1.0 - 1.0 / B)
    empty = sceneranks.SceneRanks(sums=torch.zeros((2, 6), dtype=torch.float64),
                                  hist=torch.zeros((2, 3, B), dtype=torch.int32),
                                  tot=torch.zeros((2, 4), dtype=torch.int64), per_frame_i=None,
                                  per_frame_d=None, k=K, bins=B)
    assert empty.frames == 0 and np.isnan(empty.es)
    for g in sceneranks.FEATURES:
        assert np.isnan(empty.dev(g)) and np.isnan(empty.pit(g))
    assert np.isnan(empty.draw("loc")) and np.isnan(empty.target("spr"))
    with pytest.raises(ValueError, match="one of typ, loc, spr"):
        res.dev("mean")
    with pytest.raises(ValueError, match="one of loc, spr"):
        res.draw("typ")


def test_python_argument_checks():
    for k in (1, 65):
        with pytest.raises(ValueError, match="2..64"):
            sceneranks.check_k_bins(k, None)
    for b in (4, 65, -1):
        with pytest.raises(ValueError, match="a divisor of k \\+ 1"):
            sceneranks.check_k_bins(20, b)
    assert sceneranks.check_k_bins(20, None) == (20, 21) and sceneranks.check_k_bins(20, 0) == (20, 21)
    assert sceneranks.check_k_bins(64, None) == (64, 13) and sceneranks.check_k_bins(2, None) == (2, 3)
    # GPU tensors only, every head; the coupled head's per-pedestrian refusals stay
    from multimodaltraj_2_amd.nll import GaussianHead
    pred, tg, na = torch.zeros((1, 1, 24, 4)), torch.zeros((1, 1, 4, 12, 2)), torch.full((1,), 4, dtype=torch.int32)
    for h in (GaussianHead(device="cpu"), coupled.CoupledHead(device="cpu")):
        with pytest.raises(ValueError, match="expected a GPU tensor"):
            h.scene_ranks(pred, tg, na, 4)
        with pytest.raises(ValueError, match="2..64"):
            h.scene_ranks(pred, tg, na, 1)
        with pytest.raises(ValueError, match="targets must be"):
            h.scene_ranks(pred, tg[:, :, :3], na, 4)
    with pytest.raises(NotImplementedError, match="marginal"):
        coupled.CoupledHead(device="cpu").sample_ranks(pred, tg, na, 4)


# ---------------------------------------------------------------------------
# what the figures are for: the dependence between the pedestrians of a scene
# ---------------------------------------------------------------------------
def test_the_coupled_head_is_calibrated_and_the_independent_one_is_not():
    """The float64 checker with the device generator's restatement
    (tests/coupled_ref.py, tests/fullcov_ref.py): it cannot pass without a
    figure that sees the whole scene."""
    S, F, N, K, B, seed = (sc.PROP[k] for k in ("S", "F", "N", "K", "B", "seed"))
    pred = cc.property_setup(S, F, N, sc.PROP["side"])
    na = sc.property_n_active()
    assert na.min() == 2 and na.max() == 16 and len(set(na)) == 15
    members = np.broadcast_to((np.arange(N)[None] < na[:, None])[:, None], (S, F, N)).copy()
    fit_tg, tg = (cc.coupled_targets(pred, sc.PROP["sigma"], sc.PROP["share"], rng_seed=sc.PROP[w + "_seed"])
                  for w in ("fit", "score"))
    s = cor.sums(cor.group_residuals(pred, fit_tg, na))
    fit = cor.project(*cor.moments_fit(s["within"], s["between"], s["counts"]))
    share = np.trace(fit["B"]) / np.trace(fit["W"] + fit["B"])
    print(f"fitted share {share:.4f}, clipped {fit['clipped']}")
    assert abs(share - sc.PROP["share"]) < 0.03
    cpl = np.stack([fit["Lw"], fit["Lb"]]).astype(np.float32)
    marg = np.linalg.cholesky(fit["W"] + fit["B"]).astype(np.float32)

    def score(kind):
        with np.errstate(invalid="ignore"):
            if kind == "coupled":
                draws = np.stack([cor.sample(pred, cpl, seed + k) for k in range(K)]).astype(np.float32)
            else:
                draws = np.stack([fr.sample(pred, marg, seed + k) for k in range(K)]).astype(np.float32)
        R = sr.scene_ranks_ref(draws, tg, pred, members, K, B)
        assert R["tot"][:, 0].sum() == S * F and R["wide"] == 0
        return sr.figures(R["sums"], R["hist"], R["tot"], K)
    sc.property_check(score)


# ---------------------------------------------------------------------------
# the evaluation's flags
# ---------------------------------------------------------------------------
def test_evaluation_flags():
    from multimodaltraj_2_amd import evaluate
    from multimodaltraj_2_amd.argParser import ArgsParser
    a = ArgsParser().parser.parse_args([])
    assert a.scene_ranks == 0 and a.scene_bins == 0
    a = ArgsParser().parser.parse_args(["--num_samples", "20", "--scene_ranks", "1", "--scene_bins", "7"])
    assert a.scene_ranks == 1 and a.scene_bins == 7
    with pytest.raises(SystemExit):
        ArgsParser().parser.parse_args(["--scene_ranks", "2"])
    assert evaluate.SCN_FIGURES == ("scn_frames", "scn_es", "scn_dev_typ", "scn_pit_typ", "scn_dev_loc",
                                    "scn_pit_loc", "scn_dev_spr", "scn_pit_spr", "scn_draw_loc",
                                    "scn_target_loc", "scn_draw_spr", "scn_target_spr")
    assert evaluate.FULLCOV_SCN_FIGURES == tuple("fullcov_" + k for k in evaluate.SCN_FIGURES)
    assert evaluate.MIX_SCN_FIGURES == tuple("mix_" + k for k in evaluate.SCN_FIGURES)
    assert evaluate.COUPLED_SCN_FIGURES == tuple("coupled_" + k for k in evaluate.SCN_FIGURES)
    # refused before any data is read or any launch made
    for k, b, word in ((1, 0, "2 <= K <= 64"), (65, 0, "2 <= K <= 64"), (20, 4, "--scene_bins"),
                       (20, 65, "--scene_bins")):
        a.num_samples, a.scene_bins = k, b
        with pytest.raises(ValueError, match=word):
            evaluate.evaluate_best_of_k(a, None, None, log=lambda s: None)
    # the figures of a result, in the stated order, on hand-made counts
    hist = np.full((1, 3, 7), 3, np.int32)
    tot = np.array([[21, 210, 210, 210]], np.int64)
    sums = 21.0 * (np.arange(6, dtype=np.float64)[None] + 1)
    res = sceneranks.SceneRanks(sums=torch.from_numpy(sums), hist=torch.from_numpy(hist), tot=torch.from_numpy(tot),
                                per_frame_i=None, per_frame_d=None, k=20, bins=7)
    for prefix, names in (("", evaluate.SCN_FIGURES), ("fullcov_", evaluate.FULLCOV_SCN_FIGURES),
                          ("mix_", evaluate.MIX_SCN_FIGURES), ("coupled_", evaluate.COUPLED_SCN_FIGURES)):
        fig = evaluate.scene_figures(res, prefix)
        assert tuple(fig) == names
        assert fig[prefix + "scn_frames"] == 21 and fig[prefix + "scn_dev_loc"] == 0.0
        assert fig[prefix + "scn_pit_typ"] == pytest.approx(0.5) and fig[prefix + "scn_es"] == pytest.approx(0.0)
        assert fig[prefix + "scn_draw_loc"] == 3.0 and fig[prefix + "scn_target_spr"] == 6.0
