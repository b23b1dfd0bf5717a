"""CPU: the contract table of the sampled evaluations' host paths — the 15
``*_f32`` entry points (best-of-K, joint best-of-K, KDE-NLL, sample scores and
sample modes of the per-step, the full-covariance and the mixture head), their
``*_workspace_bytes`` functions and the three geometry queries.

Every case returns before any HIP call, so nothing here needs a GPU: pointers
are made-up integers of the stated alignment and are never dereferenced (the
geometry queries' ``out`` is real: a success writes it).

Per entry point, a family's ``checks`` are its validator's checks IN THE ORDER
THE LIBRARY RUNS THEM.  A check lists one or more ways to commit exactly that
fault, each with the code and the FULL message expected:
  * every fault alone (everything else valid);
  * every adjacent pair of checks, both faults present (the first way of
    each): the earlier check's code and message — this pins the order;
  * the successes that launch nothing (S = 0; for KDE-NLL also F = 0 with S > 0).
The codes and messages are literals recorded from the library as it was before
the entry points moved into the files of their kernels; a literal that had to
change to follow the library would be a change of behaviour."""
import ctypes
from dataclasses import dataclass

import pytest

from multimodaltraj_2_amd import _lib, mixture, modes, scores

OK, EINVAL, EUNSUPPORTED = 0, -1, -4
P = 0x10000                    # a non-NULL pointer, 64-byte aligned; P * i are distinct ones
DIMS = dict(S=2, F=3, T=8, L=12, D=16, H=64, Nmax=5, W=8, stride=0, flags=0)
INF, NAN = float("inf"), float("nan")

DIMS_NULL = ("dims", [({"dims": None}, EINVAL, "dims is NULL")])
BAND = ("flags", [({"flags": 1}, EUNSUPPORTED, "{name} reads pred_path_band [S, F, 2L, Nmax]"),
                  ({"flags": 3}, EUNSUPPORTED, "{name} reads pred_path_band [S, F, 2L, Nmax]")])
SHARED_ONLY = ("flags", [({"flags": 1}, EUNSUPPORTED, "{name}: flags 1 (0 or G2K_STEP_TARGETS_SHARED)"),
                         ({"flags": 4}, EUNSUPPORTED, "{name}: flags 4 (0 or G2K_STEP_TARGETS_SHARED)"),
                         ({"flags": 6}, EUNSUPPORTED, "{name}: flags 6 (0 or G2K_STEP_TARGETS_SHARED)"),
                         ({"flags": 256}, EUNSUPPORTED,
                          "{name}: flags 256 (0 or G2K_STEP_TARGETS_SHARED)")])
SIZES = ("sizes", [({"Nmax": 0}, EINVAL, "S=2 F=3 Nmax=0"), ({"Nmax": 257}, EINVAL, "S=2 F=3 Nmax=257"),
                   ({"S": -1}, EINVAL, "S=-1 F=3 Nmax=5"), ({"F": -1}, EINVAL, "S=2 F=-1 Nmax=5")])
TARGETS = ("targets", [({"targets": 2 * P + 4}, EINVAL, "targets must be 8-byte aligned")])
PER_PED = ("per_ped", [({"per_ped": 7 * P + 8}, EINVAL, "per_ped must be 16-byte aligned"),
                       ({"per_ped": 7 * P + 4}, EINVAL, "per_ped must be 16-byte aligned")])
OUT_NULL = ("out", [({"out": None}, EINVAL, "out is NULL")])


def required(*names):
    return ("required", [({n: None}, EINVAL, "a required buffer pointer is NULL") for n in names])


def workspace(align, need, suffix=""):
    """The two workspace checks: a named workspace's alignment, then (S > 0)
    its presence and size."""
    return [("ws_align", [({"ws": 9 * P + align // 2}, EINVAL, f"workspace must be {align}-byte aligned")]),
            ("ws_size", [({"ws_bytes": need - 1}, EINVAL,
                          f"workspace of {need} bytes needed (got {need - 1}){suffix}"),
                         ({"ws": None}, EINVAL, f"workspace of {need} bytes needed (got {need}){suffix}"),
                         ({"ws_bytes": 0}, EINVAL, f"workspace of {need} bytes needed (got 0){suffix}")])]


@dataclass(frozen=True)
class Family:
    entries: tuple                 # (symbol, the name its messages use)
    args: dict                     # the valid call after dims, in call order
    checks: list                   # (label, [(faults, code, message), ...]) in the library's order
    successes: tuple = ()          # faults-style overrides of calls that return G2K_OK without a launch
    refusals: tuple = ()           # (faults, code, message): what still fails when nothing would launch


_PAIRS = dict(pred=P, targets=2 * P, n_active=3 * P, n_frames=None, ped_mask=None, head=6 * P, seed=7)
_EMPTY = ({"S": 0}, {"S": 0, "ws": None, "ws_bytes": 0}, {"S": 0, "F": 0, "ws_bytes": 0})
_ANY_FLAG = ({"S": 0, "flags": 2}, {"S": 0, "flags": 4 | 8}, {"S": 0, "flags": 2 | 256})

BEST_OF_K = Family(
    entries=(("g2k_best_of_k_f32", "best_of_k"), ("g2k_fullcov_best_of_k_f32", "fullcov_best_of_k"),
             ("g2k_mix_best_of_k_f32", "mix_best_of_k")),
    args=dict(_PAIRS, K=4, per_ped=7 * P, best=8 * P, out=10 * P, ws=9 * P, ws_bytes=192, stream=None),
    checks=[DIMS_NULL, BAND, SIZES,
            ("K", [({"K": 0}, EINVAL, "K=0 (1..4096)"), ({"K": 4097}, EINVAL, "K=4097 (1..4096)"),
                   ({"K": -3}, EINVAL, "K=-3 (1..4096)")]),
            required("pred", "targets", "n_active", "head", "out"), TARGETS, PER_PED,
            *workspace(4, 192)],
    successes=_EMPTY + _ANY_FLAG + ({"S": 0, "per_ped": None, "best": None, "K": 4096},),
    refusals=(({"S": 0, "K": 0}, EINVAL, "K=0 (1..4096)"),
              ({"S": 0, "ws": 9 * P + 2}, EINVAL, "workspace must be 4-byte aligned")))

KDE_NLL = Family(
    entries=(("g2k_kde_nll_f32", "kde_nll"), ("g2k_fullcov_kde_nll_f32", "fullcov_kde_nll"),
             ("g2k_mix_kde_nll_f32", "mix_kde_nll")),
    args=dict(_PAIRS, K=4, log_floor=-20.0, per_ped=7 * P, out=10 * P, ws=9 * P, ws_bytes=192,
              stream=None),
    checks=[DIMS_NULL, BAND, SIZES,
            ("K", [({"K": 3}, EINVAL, "K=3 (4..4096)"), ({"K": 4097}, EINVAL, "K=4097 (4..4096)"),
                   ({"K": 0}, EINVAL, "K=0 (4..4096)")]),
            ("log_floor", [({"log_floor": INF}, EINVAL, "log_floor=inf (finite)"),
                           ({"log_floor": -INF}, EINVAL, "log_floor=-inf (finite)"),
                           ({"log_floor": NAN}, EINVAL, "log_floor=nan (finite)")]),
            required("pred", "targets", "n_active", "head", "out"), TARGETS, PER_PED,
            *workspace(4, 192)],
    # F = 0 with S > 0 launches nothing either (its workspace: one row a scene, 64 bytes)
    successes=_EMPTY + _ANY_FLAG + ({"F": 0}, {"F": 0, "ws_bytes": 64}, {"S": 0, "per_ped": None}),
    refusals=(({"F": 0, "ws_bytes": 63}, EINVAL, "workspace of 64 bytes needed (got 63)"),
              ({"S": 0, "K": 3}, EINVAL, "K=3 (4..4096)")))

JOINT_EVAL = Family(
    entries=(("g2k_joint_eval_f32", "joint_eval"), ("g2k_fullcov_joint_eval_f32", "fullcov_joint_eval"),
             ("g2k_mix_joint_eval_f32", "mix_joint_eval")),
    args=dict(_PAIRS, K=4, radius=0.05, per_frame_f=7 * P, per_frame_i=8 * P, sums_f=10 * P,
              sums_i=11 * P, ws=9 * P, ws_bytes=1920, stream=None),
    checks=[DIMS_NULL, BAND, SIZES,
            ("K", [({"K": 0}, EINVAL, "K=0 (1..4096)"), ({"K": 4097}, EINVAL, "K=4097 (1..4096)")]),
            ("radius", [({"radius": -1.0}, EINVAL, "radius=-1 (finite, >= 0)"),
                        ({"radius": INF}, EINVAL, "radius=inf (finite, >= 0)"),
                        ({"radius": NAN}, EINVAL, "radius=nan (finite, >= 0)")]),
            required("pred", "targets", "n_active", "head", "sums_f", "sums_i"), TARGETS,
            ("sums_i", [({"sums_i": 11 * P + 4}, EINVAL, "sums_i must be 8-byte aligned")]),
            *workspace(4, 1920, ", 4-byte aligned")],
    successes=_EMPTY + _ANY_FLAG + ({"S": 0, "per_frame_f": None, "per_frame_i": None, "radius": 0.0},),
    refusals=(({"S": 0, "sums_i": None}, EINVAL, "a required buffer pointer is NULL"),))

_K_SCORES = ("K", [({"K": 1}, EINVAL, "K=1 (2..256)"), ({"K": 257}, EINVAL, "K=257 (2..256)")])
SAMPLE_SCORES = Family(
    entries=(("g2k_sample_scores_f32", "sample_scores"),
             ("g2k_fullcov_sample_scores_f32", "fullcov_sample_scores"),
             ("g2k_mix_sample_scores_f32", "mix_sample_scores")),
    args=dict(_PAIRS, K=4, per_ped=7 * P, out=10 * P, ws=9 * P, ws_bytes=192, stream=None),
    checks=[DIMS_NULL, SHARED_ONLY, SIZES, _K_SCORES,
            required("pred", "targets", "n_active", "head", "out"), TARGETS, PER_PED,
            *workspace(4, 192)],
    successes=_EMPTY + ({"S": 0, "flags": 2}, {"S": 0, "per_ped": None, "K": 256}),
    refusals=(({"S": 0, "flags": 4}, EUNSUPPORTED, "{name}: flags 4 (0 or G2K_STEP_TARGETS_SHARED)"),))

_M_MODES = ("M", [({"M": 0}, EINVAL, "M=0 (1..32)"), ({"M": 33, "K": 64}, EINVAL, "M=33 (1..32)")])
_K_MODES = ("K", [({"K": 1}, EINVAL, "K=1 (M=2..256)"), ({"K": 257}, EINVAL, "K=257 (M=2..256)")])
SAMPLE_MODES = Family(
    entries=(("g2k_sample_modes_f32", "sample_modes"),
             ("g2k_fullcov_sample_modes_f32", "fullcov_sample_modes"),
             ("g2k_mix_sample_modes_f32", "mix_sample_modes")),
    args=dict(_PAIRS, K=4, M=2, iters=3, miss_radius=0.0, per_ped=7 * P, centres=8 * P, weights=12 * P,
              out=10 * P, ws=9 * P, ws_bytes=384, stream=None),
    checks=[DIMS_NULL, SHARED_ONLY, SIZES, _M_MODES, _K_MODES,
            ("iters", [({"iters": -1}, EINVAL, "iters=-1 (0..64)"), ({"iters": 65}, EINVAL, "iters=65 (0..64)")]),
            ("miss_radius", [({"miss_radius": -1.0}, EINVAL, "miss_radius=-1 (finite, >= 0)"),
                             ({"miss_radius": INF}, EINVAL, "miss_radius=inf (finite, >= 0)"),
                             ({"miss_radius": NAN}, EINVAL, "miss_radius=nan (finite, >= 0)")]),
            required("pred", "targets", "n_active", "head", "out"), TARGETS, PER_PED,
            *workspace(8, 384)],
    successes=_EMPTY + ({"S": 0, "flags": 2}, {"S": 0, "per_ped": None, "centres": None, "weights": None}),
    refusals=(({"S": 0, "flags": 8}, EUNSUPPORTED, "{name}: flags 8 (0 or G2K_STEP_TARGETS_SHARED)"),))

# the geometry queries: host arithmetic, so a valid call is a success that launches nothing
_GEOM_OUT = (ctypes.c_int32 * 8)()
BESTK_GEOMETRY = Family(
    entries=(("g2k_best_of_k_geometry", ""),), args=dict(K=4, out=_GEOM_OUT),
    checks=[DIMS_NULL, SIZES,
            ("K", [({"K": 0}, EINVAL, "K=0 (1..4096)"), ({"K": 4097}, EINVAL, "K=4097 (1..4096)")]),
            OUT_NULL],
    successes=({}, {"S": 0}, {"flags": 1}))
SCORES_GEOMETRY = Family(
    entries=(("g2k_sample_scores_geometry", ""),), args=dict(K=4, out=_GEOM_OUT),
    checks=[DIMS_NULL, SIZES, _K_SCORES, OUT_NULL], successes=({}, {"S": 0}, {"flags": 1}))
MODES_GEOMETRY = Family(
    entries=(("g2k_sample_modes_geometry", ""),), args=dict(K=4, M=2, out=_GEOM_OUT),
    checks=[DIMS_NULL, SIZES, _M_MODES, _K_MODES, OUT_NULL], successes=({}, {"S": 0}, {"flags": 1}))

FAMILIES = (BEST_OF_K, JOINT_EVAL, KDE_NLL, SAMPLE_SCORES, SAMPLE_MODES, BESTK_GEOMETRY, SCORES_GEOMETRY,
            MODES_GEOMETRY)
ENTRY_POINTS = [pytest.param(fam, symbol, name, id=symbol) for fam in FAMILIES
                for symbol, name in fam.entries]

# *_workspace_bytes: (dims overrides or None for a NULL dims) -> bytes.  Best-of-K, joint and KDE-NLL
# return -1 only for a NULL dims or a negative S / F; the scores' and the modes' look at Nmax too.
def _ws_old(need):
    return ((None, -1), ({"S": -1}, -1), ({"F": -1}, -1), ({"Nmax": 0}, need), ({"Nmax": 257}, need),
            ({}, need), ({"S": 0}, 0))


def _ws_new(need):
    return ((None, -1), ({"S": -1}, -1), ({"F": -1}, -1), ({"Nmax": 0}, -1), ({"Nmax": 257}, -1),
            ({}, need), ({"S": 0}, 0))


WORKSPACE_BYTES = {
    "g2k_best_of_k_workspace_bytes": _ws_old(192) + (({"F": 0}, 64),),
    "g2k_fullcov_best_of_k_workspace_bytes": _ws_old(192) + (({"F": 0}, 64),),
    "g2k_mix_best_of_k_workspace_bytes": _ws_old(192) + (({"F": 0}, 64),),
    "g2k_kde_nll_workspace_bytes": _ws_old(192) + (({"F": 0}, 64),),
    "g2k_fullcov_kde_nll_workspace_bytes": _ws_old(192) + (({"F": 0}, 64),),
    "g2k_mix_kde_nll_workspace_bytes": _ws_old(192) + (({"F": 0}, 64),),
    # 8 units a scene-frame at these shapes, one row of 10 int32 each
    "g2k_joint_eval_workspace_bytes": _ws_old(1920) + (({"F": 0}, 80),),
    "g2k_fullcov_joint_eval_workspace_bytes": _ws_old(1920) + (({"F": 0}, 80),),
    "g2k_mix_joint_eval_workspace_bytes": _ws_old(1920) + (({"F": 0}, 80),),
    "g2k_sample_scores_workspace_bytes": _ws_new(192) + (({"F": 0}, 64),),
    "g2k_sample_modes_workspace_bytes": _ws_new(384) + (({"F": 0}, 128),),
}


@pytest.fixture(scope="module")
def lib():
    mixture.load()
    scores.load()
    return modes.load()            # one handle: every header's symbols bound on it


def _call(lib, fam, symbol, faults):
    dims, args, null_dims = dict(DIMS), dict(fam.args), False
    for key, value in faults.items():
        if key == "dims":
            null_dims = True
        elif key in dims:
            dims[key] = value
        else:
            assert key in args, (symbol, key)
            args[key] = value
    d = None if null_dims else ctypes.byref(_lib.G2KDims(**dims))
    rc = getattr(lib, symbol)(d, *args.values())
    return rc, (lib.g2k_last_error() or b"").decode()


def test_the_table_covers_every_sampled_entry_point():
    tables = dict(_lib.SYMBOLS, **mixture.SYMBOLS, **scores.SYMBOLS, **modes.SYMBOLS)
    stems = ("best_of_k", "joint_eval", "kde_nll", "sample_scores", "sample_modes")
    sampled = {s for s in tables if any(stem in s for stem in stems)}
    covered = {symbol for fam in FAMILIES for symbol, _ in fam.entries} | set(WORKSPACE_BYTES)
    assert covered == sampled
    assert sum(s.endswith("_f32") for s in covered) == 15


@pytest.mark.parametrize("fam, symbol, name", ENTRY_POINTS)
def test_each_fault_alone(lib, fam, symbol, name):
    for label, ways in fam.checks:
        for faults, code, message in ways:
            rc, msg = _call(lib, fam, symbol, faults)
            assert (rc, msg) == (code, message.format(name=name)), (symbol, label, faults)


@pytest.mark.parametrize("fam, symbol, name", ENTRY_POINTS)
def test_adjacent_faults_report_the_earlier_check(lib, fam, symbol, name):
    pairs = 0
    for (label, first), (label2, second) in zip(fam.checks, fam.checks[1:]):
        if label == "dims":
            continue               # a NULL dims has nothing else to be wrong in
        faults, code, message = first[0]
        both = dict(second[0][0], **faults)
        assert len(both) == len(faults) + len(second[0][0]), (label, label2, "the faults overlap")
        rc, msg = _call(lib, fam, symbol, both)
        assert (rc, msg) == (code, message.format(name=name)), (symbol, label, label2, both)
        pairs += 1
    assert pairs == len(fam.checks) - 2


@pytest.mark.parametrize("fam, symbol, name", ENTRY_POINTS)
def test_successes_that_launch_nothing(lib, fam, symbol, name):
    assert fam.successes
    for faults in fam.successes:
        rc, msg = _call(lib, fam, symbol, faults)
        assert rc == OK, (symbol, faults, msg)
    for faults, code, message in fam.refusals:
        rc, msg = _call(lib, fam, symbol, faults)
        assert (rc, msg) == (code, message.format(name=name)), (symbol, faults)


@pytest.mark.parametrize("symbol", sorted(WORKSPACE_BYTES))
def test_workspace_bytes(lib, symbol):
    size = getattr(lib, symbol)
    for over, want in WORKSPACE_BYTES[symbol]:
        d = None if over is None else ctypes.byref(_lib.G2KDims(**dict(DIMS, **over)))
        assert size(d) == want, (symbol, over)
