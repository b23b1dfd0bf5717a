"""CPU: the k-medoid reduction of joint samples to scene modes
(include/g2k_scene_modes.h, multimodaltraj_2_amd/scenemodes.py,
csrc/g2k_scene_modes.hip) — the header, the module's binding table and the
library's exports agree; every validator rejects bad arguments before touching
the GPU, in the header's order; the workspace and geometry queries; the checker
tests/scene_modes_ref.py alone: against plain loops and closed forms; the two
conditions the cases must meet (no decision of the algorithm within 1e-9
without being an exact tie; rounds that move a medoid in k20); and the reason
the figures exist — a few joint draws of a fitted scene-coupled head cover a
scene whose pedestrians move together, those of a full-covariance head with the
same marginals do not."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import (_lib, coupled, couples, kin, mixture, modes, ranks, scenemodes, sceneranks,
                                  scores)
from multimodaltraj_2_amd import build as g2k_build
from tests import coupled_ref as cor
from tests import couples_cases as cc
from tests import fullcov_ref as fr
from tests import scene_modes_cases as mc
from tests import scene_modes_ref as mr
from tests.bestk_ref import BOUNDARY_SEEDS
from tests import scene_ranks_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2k_scene_modes.h")
P = 0x10000                    # a non-NULL pointer, 64-byte aligned (never dereferenced)
OK, EINVAL, EUNSUPPORTED = 0, -1, -4
ENTRIES = (("g2k_scene_modes_f32", "scene_modes"), ("g2k_fullcov_scene_modes_f32", "fullcov_scene_modes"),
           ("g2k_mix_scene_modes_f32", "mix_scene_modes"))
L = 12


def _declarations():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(g2k_[a-z0-9_]+)\s*\(([^)]*)\)", src)}


# ---------------------------------------------------------------------------
# the header, the binding and the exports
# ---------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    decl = _declarations()
    assert sorted(decl) == sorted(scenemodes.SYMBOLS)
    for name, args in decl.items():
        assert len(args.split(",")) == len(scenemodes.SYMBOLS[name][1]), name
    # by symbol, after ABI 11: in no other header or table
    for table in (_lib.SYMBOLS, mixture.SYMBOLS, scores.SYMBOLS, modes.SYMBOLS, ranks.SYMBOLS, kin.SYMBOLS,
                  couples.SYMBOLS, coupled.SYMBOLS, sceneranks.SYMBOLS):
        assert not set(decl) & set(table)
    for other in ("g2k_hip.h", "g2k_mix.h", "g2k_scores.h", "g2k_modes.h", "g2k_ranks.h", "g2k_kin.h",
                  "g2k_couples.h", "g2k_scene_ranks.h"):
        assert "scene_modes" not in open(os.path.join(ROOT, "include", other)).read()
    assert "g2k_coupled_" not in open(HEADER).read()
    # the scene-coupled head's twin: declared in its own header, bound by coupled.py, the same signature
    csrc = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "g2k_coupled.h")).read(), flags=re.S)
    twin = re.search(r"\bg2k_coupled_scene_modes_f32\s*\(([^)]*)\)", csrc).group(1)
    norm = lambda a: [" ".join(p.split()) for p in a.replace("cpl", "chol").split(",")]
    assert norm(twin) == norm(decl["g2k_fullcov_scene_modes_f32"])
    assert coupled.SYMBOLS["g2k_coupled_scene_modes_f32"] is scenemodes.SYMBOLS["g2k_fullcov_scene_modes_f32"]
    lib = scenemodes.load()
    for name, (res, args) in scenemodes.SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.g2k_abi_version() == _lib.ABI_VERSION == 11
    assert scenemodes.load() is lib
    assert list(coupled.load().g2k_coupled_scene_modes_f32.argtypes) == scenemodes._SMD[1]
    src = open(HEADER).read()
    for macro, value in (("MMAX", scenemodes.MMAX), ("KMIN", scenemodes.KMIN), ("KMAX", scenemodes.KMAX),
                         ("ITERS_MAX", scenemodes.ITERS_MAX), ("SUMS", scenemodes.NSUMS),
                         ("TOT", scenemodes.NTOT)):
        assert int(re.search(rf"G2K_SCENE_MODES_{macro} (\d+)", src).group(1)) == value
    assert (scenemodes.MMAX, scenemodes.KMIN, scenemodes.KMAX, scenemodes.ITERS_MAX) == \
        (mr.M_MAX, mr.K_MIN, mr.K_MAX, mr.ITERS_MAX) == (32, 2, 64, 32)
    assert int(re.search(r"G2K_SCENE_MODES_GEOM_FIELDS (\d+)", src).group(1)) == len(scenemodes.GEOM_FIELDS)
    for i, f in enumerate(scenemodes.GEOM_FIELDS):
        assert int(re.search(rf"G2K_SCENE_MODES_GEOM_{f.upper()} (\d+)", src).group(1)) == i
    assert ("Alignment (bytes) of g2k_scene_modes_f32, g2k_fullcov_scene_modes_f32 and\n"
            " * g2k_mix_scene_modes_f32: targets 8, per_frame_i 4, per_frame_d 8, medoids 4,\n"
            " * counts 4, sums 8, tot 8, workspace 8.") in src
    assert HEADER in [os.path.abspath(p) for p in g2k_build.HDR]    # hashed, and a change rebuilds
    assert os.path.join(g2k_build.CSRC, "g2k_scene_modes.hip") in g2k_build.SRC


# ---------------------------------------------------------------------------
# the validators: before any HIP call
# ---------------------------------------------------------------------------
DIMS = dict(S=2, F=3, T=8, L=12, D=16, H=64, Nmax=5, W=8, stride=0, flags=0)
NEED = 2 * 3 * (88 + 8 * 6)              # S * F scene-frames, a row of 88 + 8 M bytes each
ARGS = dict(pred=P, targets=2 * P, n_active=3 * P, n_frames=None, ped_mask=None, head=6 * P, seed=7, K=20,
            M=6, iters=10, miss_radius=ctypes.c_float(1.0), per_frame_i=13 * P, per_frame_d=12 * P,
            medoids=14 * P, counts=15 * P, sums=11 * P, tot=10 * P, ws=9 * P, ws_bytes=NEED, stream=None)
FLAGS = "{name}: flags %d (0 or G2K_STEP_TARGETS_SHARED)"
NULL = "a required buffer pointer is NULL"
f32 = ctypes.c_float


def _align(name, base, n):
    return (name, [({name: base + n - 1}, EINVAL, f"{name} must be {n}-byte aligned"),
                   ({name: base + n // 2}, EINVAL, f"{name} must be {n}-byte aligned")])


# the checks in the order the library runs them; each fault alone, with its code and full message
CHECKS = [
    ("dims", [({"dims": None}, EINVAL, "dims is NULL")]),
    ("flags", [({"flags": f}, EUNSUPPORTED, FLAGS % f) for f in (1, 4, 6, 256)]),
    ("sizes", [({"Nmax": 0}, EINVAL, "S=2 F=3 Nmax=0"), ({"Nmax": 257}, EINVAL, "S=2 F=3 Nmax=257"),
               ({"S": -1}, EINVAL, "S=-1 F=3 Nmax=5"), ({"F": -1}, EINVAL, "S=2 F=-1 Nmax=5")]),
    ("M", [({"M": 0}, EINVAL, "M=0 (1..32)"), ({"M": 33, "K": 40}, EINVAL, "M=33 (1..32)"),
           ({"M": -2}, EINVAL, "M=-2 (1..32)")]),
    ("K", [({"K": 5}, EINVAL, "K=5 (6..64)"), ({"K": 65}, EINVAL, "K=65 (6..64)"),
           ({"K": 1, "M": 1}, EINVAL, "K=1 (2..64)"), ({"K": 0, "M": 1}, EINVAL, "K=0 (2..64)"),
           ({"K": 31, "M": 32}, EINVAL, "K=31 (32..64)"), ({"K": -5}, EINVAL, "K=-5 (6..64)")]),
    ("iters", [({"iters": -1}, EINVAL, "iters=-1 (0..32)"), ({"iters": 33}, EINVAL, "iters=33 (0..32)")]),
    ("miss_radius", [({"miss_radius": f32(-0.5)}, EINVAL, "miss_radius=-0.5 (finite, >= 0)"),
                     ({"miss_radius": f32(float("inf"))}, EINVAL, "miss_radius=inf (finite, >= 0)"),
                     ({"miss_radius": f32(float("nan"))}, EINVAL, "miss_radius=nan (finite, >= 0)")]),
    ("required", [({n: None}, EINVAL, NULL) for n in ("pred", "targets", "n_active", "head", "sums", "tot")]),
    ("targets", [({"targets": 2 * P + 7}, EINVAL, "targets must be 8-byte aligned"),
                 ({"targets": 2 * P + 4}, EINVAL, "targets must be 8-byte aligned")]),
    _align("per_frame_i", 13 * P, 4), _align("per_frame_d", 12 * P, 8), _align("medoids", 14 * P, 4),
    _align("counts", 15 * P, 4), _align("sums", 11 * P, 8), _align("tot", 10 * P, 8),
    ("ws_align", [({"ws": 9 * P + 7}, EINVAL, "workspace must be 8-byte aligned"),
                  ({"ws": 9 * P + 4}, EINVAL, "workspace must be 8-byte aligned")]),
    ("ws_size", [({"ws_bytes": NEED - 1}, EINVAL, f"workspace of {NEED} bytes needed (got {NEED - 1})"),
                 ({"ws": None}, EINVAL, f"workspace of {NEED} bytes needed (got {NEED})"),
                 ({"ws_bytes": 0}, EINVAL, f"workspace of {NEED} bytes needed (got 0)")]),
]
# what returns G2K_OK without a launch, at the weakest alignments the header states
SUCCESSES = ({"S": 0}, {"S": 0, "ws": None, "ws_bytes": 0}, {"S": 0, "F": 0, "ws_bytes": 0},
             {"S": 0, "flags": 2}, {"S": 0, "K": 64, "M": 32, "iters": 32}, {"S": 0, "K": 2, "M": 2, "iters": 0},
             {"S": 0, "K": 2, "M": 1}, {"S": 0, "miss_radius": f32(0.0)},
             {"S": 0, "per_frame_i": None, "per_frame_d": None, "medoids": None, "counts": None},
             {"S": 0, "targets": 2 * P + 8, "per_frame_i": 13 * P + 4, "per_frame_d": 12 * P + 8,
              "medoids": 14 * P + 4, "counts": 15 * P + 4, "sums": 11 * P + 8, "tot": 10 * P + 8,
              "ws": 9 * P + 8, "pred": P + 4, "head": 6 * P + 4})
REFUSALS = (({"S": 0, "flags": 4}, EUNSUPPORTED, FLAGS % 4), ({"S": 0, "K": 1, "M": 1}, EINVAL, "K=1 (2..64)"),
            ({"S": 0, "M": 0}, EINVAL, "M=0 (1..32)"), ({"S": 0, "iters": 33}, EINVAL, "iters=33 (0..32)"),
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
    lib = lib or scenemodes.load()
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
    lib = lib or scenemodes.load()
    for faults in SUCCESSES:
        rc_, msg = _call(lib, symbol, faults)
        assert rc_ == OK, (faults, msg)
    for faults, code, message in REFUSALS:
        assert _call(lib, symbol, faults) == (code, message.format(name=name)), faults


def test_the_coupled_entry_point_faults_like_its_twin():
    """g2k_coupled_scene_modes_f32 under the whole table of faults, successes
    and refusals, and fault for fault g2k_fullcov_scene_modes_f32's report."""
    lib = coupled.load()
    scenemodes.load()
    test_each_fault_alone_and_in_order("g2k_coupled_scene_modes_f32", "coupled_scene_modes", lib)
    test_successes_that_launch_nothing("g2k_coupled_scene_modes_f32", "coupled_scene_modes", lib)
    for label, ways in CHECKS:
        for faults, code, message in ways:
            got = _call(lib, "g2k_coupled_scene_modes_f32", faults)
            want = _call(lib, "g2k_fullcov_scene_modes_f32", faults)
            assert got == (want[0], want[1].replace("fullcov_", "coupled_")), (label, faults)


def test_workspace_bytes_and_geometry_queries():
    lib = scenemodes.load()
    size = lib.g2k_scene_modes_workspace_bytes

    def d(**kw):
        return ctypes.byref(_lib.G2KDims(**dict(DIMS, **kw)))
    assert size(d(), 20, 6) == NEED == 816 and size(d(), 64, 6) == NEED and size(d(), 20, 1) == 6 * 96
    assert size(d(), 64, 32) == 6 * 344
    assert size(d(F=0), 20, 6) == 2 * 136 and size(d(S=0), 20, 6) == 0
    assert size(d(Nmax=256), 20, 6) == NEED              # one workgroup per scene-frame whatever P
    assert size(None, 20, 6) == -1
    for bad in (dict(Nmax=0), dict(Nmax=257), dict(S=-1), dict(F=-1)):
        assert size(d(**bad), 20, 6) == -1
    for k, m in ((20, 0), (20, 33), (1, 1), (65, 6), (5, 6), (31, 32)):
        assert size(d(), k, m) == -1
    out = (ctypes.c_int32 * len(scenemodes.GEOM_FIELDS))()
    geo = lib.g2k_scene_modes_geometry
    for args, msg in (((None, 20, 6, out), "dims is NULL"), ((d(Nmax=257), 20, 6, out), "S=2 F=3 Nmax=257"),
                      ((d(), 20, 0, out), "M=0 (1..32)"), ((d(), 1, 1, out), "K=1 (2..64)"),
                      ((d(), 65, 6, out), "K=65 (6..64)"), ((d(), 20, 6, None), "out is NULL")):
        assert geo(*args) == EINVAL and lib.g2k_last_error().decode() == msg
    assert geo(d(), 20, 6, out) == OK and geo(d(S=0), 2, 1, out) == OK and geo(d(flags=1), 64, 32, out) == OK


def test_geometry_claims_and_branches():
    reached = set()
    for i, (name, _, M, iters) in enumerate(mc.CASES):
        c = mc.inputs(i)
        S, F, N = c["members"].shape
        K = c["K"]
        g = scenemodes.scene_modes_geometry(S, F, N, K, M)
        assert g == mc.geometry(N, K, M) and g["tm"] == c["tm"], (name, g)
        # a tile's items fit the 520 slots; what goes over them at the end fits too; with the mixture
        # head's 19376 bytes two workgroups fit gfx950's 160 KB
        assert g["tm"] * (K + 1) <= 520 and (65 * 65 + 256) * 8 + 160 * 4 <= 520 * 28 * 4
        assert 2 * (g["lds_bytes"] + 19376) <= 160 * 1024
        assert 1 <= M <= 32 and max(M, 2) <= K <= 64 and 0 <= iters <= 32
        members = c["members"].sum(axis=2)
        reached.add("16-member tiles" if g["tm"] == 16 else "8-member tiles")
        reached.add("one pair a lane" if g["apt"] == 1 else "several pairs a lane")
        if g["apt"] == 9:
            reached.add("the most accumulators a lane")
        for Pn in np.unique(members):
            Pn = int(Pn)
            reached.add({0: "P = 0", 1: "P = 1", 2: "P = 2"}.get(Pn, "P > 2"))
            if Pn > g["tm"] and Pn % g["tm"]:
                reached.add("a partial last tile")
            if Pn == 256:
                reached.add("P maximum")
        if c["n_frames"] is not None and (c["n_frames"] < F).any():
            reached.add("n_frames < F")
        if c["ped_mask"] is not None:
            reached.add("masked")
        if c["shared"]:
            reached.add("shared targets")
        reached.add({2: "K minimum", 64: "K maximum", 31: "K = 31", 32: "K = 32"}.get(K, "K between"))
        reached.add({1: "M = 1", 32: "M maximum"}.get(M, "M between"))
        if M == K:
            reached.add("every draw a medoid")
        if iters == 0:
            reached.add("BUILD only")
    assert reached == {"16-member tiles", "8-member tiles", "one pair a lane", "several pairs a lane",
                       "the most accumulators a lane", "P = 0", "P = 1", "P = 2", "P > 2", "a partial last tile",
                       "P maximum", "n_frames < F", "masked", "shared targets", "K minimum", "K maximum",
                       "K = 31", "K = 32", "K between", "M = 1", "M maximum", "M between",
                       "every draw a medoid", "BUILD only"}, reached
    assert mc.IDS == ["k2", "k2_m1", "k20", "k64", "n256", "shared", "k31", "k32", "iters0", "m1"]
    # the timing shapes (tools/time_scene_modes.py); F = 0
    assert scenemodes.scene_modes_geometry(384, 1, 32, 20, 6) == mc.geometry(32, 20, 6)
    assert scenemodes.scene_modes_geometry(64, 20, 256, 64, 6)["tiles"] == 32
    assert scenemodes.scene_modes_geometry(3, 0, 16, 20, 6)["w"] == 1


# ---------------------------------------------------------------------------
# the checker against an independent restatement
# ---------------------------------------------------------------------------
def test_checker_against_plain_loops():
    checked = 0
    for name, heads, frames in (("k2", mc.HEADS, None), ("k2_m1", ("mix",), None), ("shared", ("coupled",), 1),
                                ("iters0", ("fullcov",), 1), ("m1", ("per_step",), 1)):
        i = mc.IDS.index(name)
        c = mc.inputs(i)
        S, F, N = c["members"].shape
        K, M, iters = c["K"], c["M"], c["iters"]
        y = np.broadcast_to(c["targets"], (S, F, N, L, 2))
        for which in heads:
            x = mr.band_to_steps(mc.oracle_draws(i, which))
            R = mr.scene_modes_ref(mc.oracle_draws(i, which), c["targets"], c["members"], K, M, iters, c["radius"])
            assert not R["ambiguous"].any()
            for s in range(S):
                for f in range(frames or F):
                    idx = np.flatnonzero(c["members"][s, f])
                    if len(idx) < 1:
                        assert not R["per_frame_i"][s, f].any() and not R["per_frame_d"][s, f].any()
                        assert not R["medoids"][s, f].any() and not R["counts"][s, f].any()
                        continue
                    Z = [x[k, s, f, idx] for k in range(K)] + [y[s, f, idx]]
                    wi, wd, wm, wc = mr.frame_loops(Z, K, M, iters)
                    assert list(R["per_frame_i"][s, f]) == wi, (name, which, s, f)
                    assert list(R["medoids"][s, f]) == wm and list(R["counts"][s, f]) == wc
                    np.testing.assert_allclose(R["per_frame_d"][s, f], wd, rtol=1e-12, atol=1e-12)
                    checked += 1
            # what every result obeys: the medoids distinct draws, the counts K, all <= cA <= raw when
            # the first M draws are the modes' superset, w in (0, 1]
            pi, pd = R["per_frame_i"], R["per_frame_d"]
            sc_ = pi[..., 0] > 0
            assert np.all(R["counts"][sc_].sum(axis=1) == K)
            assert all(len(set(m)) == M for m in R["medoids"][sc_])
            assert np.all(pd[sc_][:, 6] <= pd[sc_][:, 0]) and np.all(pd[sc_][:, 6] <= pd[sc_][:, 5])
            assert np.all(pd[sc_][:, 2] > 0) and np.all(pd[sc_][:, 2] <= 1)
            if M == K:                                          # every draw a medoid: cA is the floor, cost 0
                assert np.all(pd[sc_][:, 0] == pd[sc_][:, 6]) and np.all(pd[sc_][:, 4] == 0)
                assert np.all(R["counts"][sc_] == 1)
    assert checked >= 25


def _one(Z, K, M, iters, radius=1.0):
    """One scene-frame from items Z [K + 1, P, L, 2]."""
    Z = np.asarray(Z, np.float32)
    Pn = Z.shape[1]
    band = lambda a: np.concatenate([a[..., 0], a[..., 1]], axis=-1).swapaxes(-1, -2)     # [..., 24, P]
    return mr.scene_modes_ref(band(Z[:K])[:, None, None], Z[K][None, None], np.ones((1, 1, Pn), bool), K, M,
                              iters, radius)


def test_closed_forms():
    # two members standing still; draw k puts both at x = off[k] at every step: A(j, l) = 24 |off_j - off_l|
    off = np.array([0.0, 1.0, 10.0, 11.0, 12.0, 4.0])             # the last: the targets
    Z = np.zeros((6, 2, L, 2))
    Z[..., 0] = off[:, None, None]
    R = _one(Z, 5, 2, 10, radius=2.5)
    # row sums 34, 31, 22, 23, 26 (x 24): m_0 = draw 2; dmin = 10, 9, 0, 1, 2; the gains of draws 0 and 1
    # are both 18 (draws 3 and 4: 2): the lowest index, draw 0
    # round 1: clusters {2, 3, 4} and {0, 1}; draw 3 has the lowest sum (2 against 3 and 3) and takes over,
    # draws 0 and 1 tie (1 and 1) and draw 0 stays; round 2 changes nothing
    assert list(R["medoids"][0, 0]) == [3, 0] and list(R["counts"][0, 0]) == [3, 2]
    assert list(R["per_frame_i"][0, 0]) == [2, 1, 1, 2] and R["moved"][0, 0] == 1
    d = R["per_frame_d"][0, 0]
    # |4 - 0| = 4 < |4 - 11| = 7: mode 1 with 2 of the 5 draws; cost (0 + 1 + 1 + 0 + 1) / 5
    np.testing.assert_allclose(d, [4.0, 4.0, 0.4, 0.4, 0.6, 3.0, 3.0, 4.0], rtol=1e-15)
    assert R["tot"].tolist() == [[1, 2, 1, 2]]                    # mx = 4 > 2.5: missed
    np.testing.assert_allclose(R["sums"][0], [8.0, 8.0, 0.36, 0.36, 1.2, 6.0, 6.0, 0.0], rtol=1e-15)
    fig = mr.figures(R["sums"], R["tot"])
    assert fig["jade"] == 4.0 and fig["brier_jade"] == pytest.approx(4.36) and fig["miss_rate"] == 1.0
    assert fig["raw_jade"] == 3.0 and fig["all_jade"] == 3.0 and fig["rounds"] == 2.0
    assert fig["cost"] == pytest.approx(0.6)
    # BUILD only: the medoids stay 2 and 0
    R0 = _one(Z, 5, 2, 0, radius=4.0)
    assert list(R0["medoids"][0, 0]) == [2, 0] and list(R0["per_frame_i"][0, 0]) == [2, 1, 1, 0]
    assert R0["per_frame_d"][0, 0][0] == 4.0 and R0["tot"][0, 2] == 0     # mx = 4 <= 4: not missed
    # no member: not scored
    R = mr.scene_modes_ref(np.zeros((2, 1, 1, 24, 3), np.float32), np.zeros((1, 1, 3, L, 2), np.float32),
                           np.zeros((1, 1, 3), bool), 2, 2, 3, 1.0)
    assert not R["tot"].any() and not R["per_frame_i"].any() and not R["sums"].any() and R["frames"] == 0


def test_the_cases_meet_their_two_conditions():
    """On every case and head the restated samplers' draws leave no argmin or
    argmax of the algorithm with its two best candidates within 1e-9 relative
    without being bit-equal (the GPU test leaves such scene-frames out, and
    fails above 1 %); in k20 rounds move a medoid under every head, with the
    seed of tests/scene_ranks_cases.py unchanged; the exact tie of k2's two row
    sums takes draw 0; the poison is never read; both sides of the miss
    radius occur."""
    frames = missed = 0
    for i, (name, _, M, iters) in enumerate(mc.CASES):
        c = mc.inputs(i)
        for which in mc.HEADS:
            R = mr.scene_modes_ref(mc.oracle_draws(i, which), c["targets"], c["members"], c["K"], M, iters,
                                   c["radius"])
            assert not R["ambiguous"].any(), (name, which)
            assert R["frames"] == int((c["members"].sum(axis=2) >= 1).sum())
            assert np.isfinite(R["per_frame_d"]).all() and np.isfinite(R["sums"]).all()
            frames += R["frames"]
            missed += int(R["tot"][:, 2].sum())
            scored = R["per_frame_i"][..., 0] > 0
            if name == "k20":
                assert R["moved"].sum() >= 1, which
            if name == "iters0":
                assert not R["per_frame_i"][..., 3].any()
            if name == "k2":
                assert np.all(R["medoids"][scored][:, 0] == 0) and np.all(R["medoids"][scored][:, 1] == 1)
            if name in ("n256", "k32", "k2"):
                assert np.all(R["counts"][scored] == 1)
    assert frames == 4 * (5 + 5 + 6 + 2 + 1 + 6 + 1 + 2 + 6 + 6) and 0 < missed < frames


@pytest.mark.parametrize("which", mc.HEADS)
@pytest.mark.parametrize("at", BOUNDARY_SEEDS)
def test_boundary_seeds_meet_the_conditions_and_see_the_carry(at, which):
    """Case k2 at the seeds whose low word carries at draw 1 (tests/bestk_ref.py;
    tests/test_scene_modes_gpu.py runs the kernel there): no ambiguous argmin or
    argmax, the poison never read, k2's own claims (the exact tie takes draw 0;
    M = K: every draw a medoid), and the checker's integer outputs change when
    draw 1 is made with the carry dropped."""
    i, seed = mc.IDS.index("k2"), BOUNDARY_SEEDS[at]
    c = mc.inputs(i)
    R, D = (mr.scene_modes_ref(mc.oracle_draws(i, which, seed, carry), c["targets"], c["members"], c["K"], c["M"],
                               c["iters"], c["radius"]) for carry in (True, False))
    for v in (R, D):
        assert not v["ambiguous"].any()
        assert v["frames"] == int((c["members"].sum(axis=2) >= 1).sum())
        assert np.isfinite(v["per_frame_d"]).all() and np.isfinite(v["sums"]).all()
        scored = v["per_frame_i"][..., 0] > 0
        assert np.all(v["medoids"][scored][:, 0] == 0) and np.all(v["medoids"][scored][:, 1] == 1)
        assert np.all(v["counts"][scored] == 1)
    changed = {k: int((R[k] != D[k]).sum()) for k in ("per_frame_i", "medoids", "counts", "tot")}
    moved = np.abs(R["sums"] - D["sums"]).max()
    print(f"k2 seed {at} {which}: carry dropped, integers changed {changed}, sums move by {moved:.3g}")
    assert changed["per_frame_i"] + changed["tot"] > 0 and moved > 1e-2


def test_the_result_class():
    sums = np.array([[6.0, 3.0, 0.5, 0.25, 1.5, 9.0, 4.5, 0.0], [6.0, 3.0, 0.5, 0.25, 1.5, 9.0, 4.5, 0.0]])
    tot = np.array([[2, 3, 1, 3], [2, 3, 0, 5]], np.int64)
    res = scenemodes.SceneModes(sums=torch.from_numpy(sums), tot=torch.from_numpy(tot), per_frame_i=None,
                                per_frame_d=None, medoids=None, counts=None, k=20, modes=6, iters=10,
                                miss_radius=1.0)
    want = mr.figures(sums, tot)
    assert res.frames == 4 and res.totals() == [4, 6, 1, 8]
    assert (res.jade, res.jfde, res.cost, res.raw_jade, res.all_jade) == (2.0, 1.0, 0.5, 3.0, 1.5)
    assert res.brier_jade == 2.25 and res.brier_jfde == 1.125 and res.miss_rate == 0.25 and res.rounds == 2.0
    for k, v in want.items():
        assert getattr(res, {"miss_rate": "miss_rate"}.get(k, k)) == v, k
    empty = scenemodes.SceneModes(sums=torch.zeros((2, 8), dtype=torch.float64),
                                  tot=torch.zeros((2, 4), dtype=torch.int64), per_frame_i=None, per_frame_d=None,
                                  medoids=None, counts=None, k=20, modes=6)
    assert empty.frames == 0
    for k in ("jade", "jfde", "brier_jade", "brier_jfde", "miss_rate", "cost", "raw_jade", "all_jade", "rounds"):
        assert np.isnan(getattr(empty, k)), k
    with pytest.raises(ValueError, match="want_modes"):
        res.trajectories(None, torch.zeros((2, 2, 24, 3)))


def test_python_argument_checks():
    assert scenemodes.check_args(20, 6, 10, 1) == (20, 6, 10, 1.0)
    assert scenemodes.check_args(2, 1, 0, 0.0) == (2, 1, 0, 0.0) and scenemodes.check_args(64, 32, 32, 2.5)
    for k, m, word in ((20, 0, "modes = 0: 1..32"), (40, 33, "modes = 33: 1..32"), (5, 6, "k = 5: 6..64"),
                       (1, 1, "k = 1: 2..64"), (65, 6, "k = 65: 6..64")):
        with pytest.raises(ValueError, match=word):
            scenemodes.check_args(k, m, 10, 1.0)
    for it in (-1, 33):
        with pytest.raises(ValueError, match="0..32"):
            scenemodes.check_args(20, 6, it, 1.0)
    for r in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="finite and >= 0"):
            scenemodes.check_args(20, 6, 10, r)
    # GPU tensors only, every head; the coupled head's per-pedestrian refusals stay
    from multimodaltraj_2_amd.fullcov import FullCovHead
    from multimodaltraj_2_amd.mixture import MixtureHead
    from multimodaltraj_2_amd.nll import GaussianHead
    pred, tg, na = torch.zeros((1, 1, 24, 4)), torch.zeros((1, 1, 4, 12, 2)), torch.full((1,), 4, dtype=torch.int32)
    for h in (GaussianHead(device="cpu"), FullCovHead(device="cpu"), MixtureHead(device="cpu"),
              coupled.CoupledHead(device="cpu")):
        with pytest.raises(ValueError, match="expected a GPU tensor"):
            h.scene_modes(pred, tg, na, 4, 2)
        with pytest.raises(ValueError, match="k = 1: 2..64"):
            h.scene_modes(pred, tg, na, 1, 1)
        with pytest.raises(ValueError, match="targets must be"):
            h.scene_modes(pred, tg[:, :, :3], na, 4, 2)
    with pytest.raises(NotImplementedError, match="marginal"):
        coupled.CoupledHead(device="cpu").sample_modes(pred, tg, na, 4, 2)


# ---------------------------------------------------------------------------
# what the figures are for: a few joint draws that cover a scene
# ---------------------------------------------------------------------------
def test_the_coupled_heads_modes_cover_the_scene_and_the_independent_ones_do_not():
    """The float64 checker with the device generator's restatement
    (tests/coupled_ref.py, tests/fullcov_ref.py): it cannot pass without a
    reduction of JOINT draws."""
    S, F, N, K, M, iters, seed = (mc.PROP[k] for k in ("S", "F", "N", "K", "M", "iters", "seed"))
    pred = cc.property_setup(S, F, N, mc.PROP["side"])
    na = sc.property_n_active()
    members = np.broadcast_to((np.arange(N)[None] < na[:, None])[:, None], (S, F, N)).copy()
    fit_tg, tg = (cc.coupled_targets(pred, mc.PROP["sigma"], mc.PROP["share"], rng_seed=mc.PROP[w + "_seed"])
                  for w in ("fit", "score"))
    s = cor.sums(cor.group_residuals(pred, fit_tg, na))
    fit = cor.project(*cor.moments_fit(s["within"], s["between"], s["counts"]))
    cpl = np.stack([fit["Lw"], fit["Lb"]]).astype(np.float32)
    marg = np.linalg.cholesky(fit["W"] + fit["B"]).astype(np.float32)

    def score(kind):
        with np.errstate(invalid="ignore"):
            if kind == "coupled":
                draws = np.stack([cor.sample(pred, cpl, seed + k) for k in range(K)]).astype(np.float32)
            else:
                draws = np.stack([fr.sample(pred, marg, seed + k) for k in range(K)]).astype(np.float32)
        R = mr.scene_modes_ref(draws, tg, members, K, M, iters, mc.PROPERTY["radius"])
        assert R["frames"] == S * F and not R["ambiguous"].any()
        return mr.figures(R["sums"], R["tot"])
    mc.property_check(score)


# ---------------------------------------------------------------------------
# the evaluation's flags
# ---------------------------------------------------------------------------
def test_evaluation_flags():
    from multimodaltraj_2_amd import evaluate
    from multimodaltraj_2_amd.argParser import ArgsParser
    a = ArgsParser().parser.parse_args([])
    assert a.scene_modes == 0 and a.scene_modes_iters == 10 and a.miss_radius == 0.0
    a = ArgsParser().parser.parse_args(["--num_samples", "20", "--scene_modes", "6", "--scene_modes_iters", "3",
                                        "--miss_radius", "1.5"])
    assert a.scene_modes == 6 and a.scene_modes_iters == 3 and a.miss_radius == 1.5
    assert evaluate.SMD_FIGURES == ("smd_frames", "smd_jade", "smd_jfde", "smd_brier_jade", "smd_brier_jfde",
                                    "smd_miss", "smd_cost", "smd_raw_jade", "smd_all_jade", "smd_rounds")
    assert evaluate.FULLCOV_SMD_FIGURES == tuple("fullcov_" + k for k in evaluate.SMD_FIGURES)
    assert evaluate.MIX_SMD_FIGURES == tuple("mix_" + k for k in evaluate.SMD_FIGURES)
    assert evaluate.COUPLED_SMD_FIGURES == tuple("coupled_" + k for k in evaluate.SMD_FIGURES)
    # refused before any data is read or any launch made
    for k, m, it, r, word in ((20, 33, 10, 1.0, "1 <= M <= 32"), (5, 6, 10, 1.0, r"max\(M, 2\) <= K <= 64"),
                              (65, 6, 10, 1.0, r"max\(M, 2\) <= K <= 64"), (1, 1, 10, 1.0, r"max\(M, 2\) <= K"),
                              (20, 6, 33, 1.0, "--scene_modes_iters"), (20, 6, -1, 1.0, "--scene_modes_iters"),
                              (20, 6, 10, -1.0, "--miss_radius"), (20, 6, 10, float("inf"), "--miss_radius")):
        a.num_samples, a.scene_modes, a.scene_modes_iters, a.miss_radius = k, m, it, r
        with pytest.raises(ValueError, match=word):
            evaluate.evaluate_best_of_k(a, None, None, log=lambda s: None)
    # the figures of a result, in the stated order, on hand-made sums
    sums = np.array([[12.0, 6.0, 1.0, 0.5, 3.0, 18.0, 9.0, 0.0]])
    tot = np.array([[4, 6, 1, 8]], np.int64)
    res = scenemodes.SceneModes(sums=torch.from_numpy(sums), tot=torch.from_numpy(tot), per_frame_i=None,
                                per_frame_d=None, medoids=None, counts=None, k=20, modes=6, iters=10,
                                miss_radius=1.0)
    for prefix, names in (("", evaluate.SMD_FIGURES), ("fullcov_", evaluate.FULLCOV_SMD_FIGURES),
                          ("mix_", evaluate.MIX_SMD_FIGURES), ("coupled_", evaluate.COUPLED_SMD_FIGURES)):
        fig = evaluate.scene_mode_figures(res, prefix)
        assert tuple(fig) == names
        assert [fig[k] for k in names] == [4, 2.0, 1.0, 2.25, 1.125, 0.25, 0.5, 3.0, 1.5, 2.0]
        line = evaluate._scene_mode_line("scene modes", res, 2, fig, prefix)
        assert line.startswith("scene modes of the 20 joint draws on dataset 2: 4 scenes reduced to 6 modes")
