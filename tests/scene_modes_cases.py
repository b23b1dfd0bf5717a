"""The inputs of the scene-mode tests (tests/test_scene_modes.py checks every
claim below on the CPU; tests/test_scene_modes_gpu.py runs the kernels on
them): the smallest shapes that reach each path of scene_modes_kernel
(csrc/g2k_scene_modes.hip).  Its geometry is scene_ranks_kernel's — one
workgroup owns a scene-frame and walks its P compacted members in tiles of TM =
16 (K <= 31) or 8 (K >= 32), the K (K + 1) / 2 pair sums dealt to the 256 lanes
— so the shapes, the head parameters and the NaN poison (columns >= n_active,
masked columns, frames >= n_frames, the factors above their diagonals) are
those of tests/scene_ranks_cases.py, taken from there by name; what this file
adds is M, the rounds and the miss radius.  A scene-frame is scored from P = 1
on, so case k2 (P = 8, 2, 1, 0) has one scored frame more than there.

Case k20's seed: with scene_ranks_cases' own seed the restated samplers' draws
already give scene-frames whose rounds move a medoid (under every head), so the
seed is unchanged.  Test helper, not a test module."""
import functools

from tests import scene_ranks_cases as sc

HEADS = sc.HEADS
RADIUS = 2.0

#  name      the shape of   M   iters  what it reaches
CASES = [
    # the minimum K; M = K = 2: both draws are medoids, and the two row sums of BUILD's first step are
    # one number (A(0, 1)): the exact tie takes draw 0; P = 8, 2, 1 and 0; n_frames < F
    ("k2",     "k2",     2,  10),
    ("k2_m1",  "k2",     1,  10),
    # the evaluation's K and M; masked columns; P = 27 / 17 / 16; rounds that move a medoid
    ("k20",    "k20",    6,  10),
    # the maximum K: 8-member tiles, 2080 pairs (9 to a lane at most)
    ("k64",    "k64",    16, 10),
    # dense: P = 256, sixteen tiles; M = K: every draw is a medoid
    ("n256",   "n256",   5,  10),
    ("shared", "shared", 6,  10),
    # either side of the tile height's K boundary; k32 with the maximum M = K = 32
    ("k31",    "k31",    6,  10),
    ("k32",    "k32",    32, 10),
    # BUILD only
    ("iters0", "k20",    6,  0),
    # one mode: the medoid of all the draws
    ("m1",     "k20",    1,  10),
]
IDS = [c[0] for c in CASES]


def geometry(N, K, M):
    """What g2k_scene_modes_geometry must report for Nmax = N, K and M."""
    tm = 16 if K <= 31 else 8
    pairs = K * (K + 1) // 2
    return dict(tm=tm, dr=256 // tm, tiles=-(-N // tm), w=1, pairs=pairs, apt=-(-pairs // 256),
                row_bytes=88 + 8 * M, lds_bytes=520 * 28 * 4 + 256 * 4 + 16)


def base(i):
    """The index of case i's shape in tests/scene_ranks_cases.py."""
    return sc.IDS.index(CASES[i][1])


@functools.lru_cache(maxsize=None)
def inputs(i):
    """Case i -> scene_ranks_cases.inputs' dict of its shape (pred, targets,
    head, chol, mix, cpl, n_active, n_frames, ped_mask, members, K, seed,
    shared, tm) with M, iters and radius."""
    _, _, M, iters = CASES[i]
    return dict(sc.inputs(base(i)), M=M, iters=iters, radius=RADIUS)


def oracle_draws(i, which, seed=None, carry=True):
    """[K, S, F, 24, N] float32: the restated sampler's draws for seeds seed +
    k (scene_ranks_cases': computed once for both families' tests; ``seed`` and
    ``carry`` as there)."""
    return sc.oracle_draws(base(i), which, seed, carry)


# ---------------------------------------------------------------------------
# the property: what the figures are for
# ---------------------------------------------------------------------------
PROP = dict(sc.PROP, M=6, iters=10)
PROPERTY = dict(radius=1.0, jade=0.792, miss=0.446)


def property_check(score, label=""):
    """``score(kind)`` -> scene_modes_ref.figures-like dict of the scoring
    targets under the modes of the K joint draws of the "coupled" head fitted
    on the other set and of the "fullcov" head fitted on the same data.  The
    thresholds are PROPERTY's, set from the NumPy run over five sample seeds
    (4242 + 1000 i; DESIGN.md 6q has the figures): each midway between the two
    laws' five-seed means, at the radius where the miss rates differ most —
    minJADE_6 0.7536 (standard deviation 0.003, range 0.7504..0.7577) against
    0.8305 (0.001, 0.8289..0.8319); the miss rate at 1.0 0.239 (0.012,
    0.219..0.246) against 0.654 (0.015, 0.637..0.670).  The gaps to the
    thresholds, 0.034 and 0.19 at the least, are 11 and 12 standard deviations
    (and more than three times the ranges).  The third claim has no threshold:
    minJADE_6 of the modes is never below that of all K draws, and below that
    of the first 6 raw draws by 0.0105..0.0177 (coupled; standard deviation of
    the difference 0.0028) and 0.0079..0.0118 (full covariance; 0.0015)."""
    co, fc = score("coupled"), score("fullcov")
    for kind, v in (("coupled", co), ("fullcov", fc)):
        print(f"{label}{kind}: " + ", ".join(f"{k} {v[k]:.4f}" for k in (
            "frames", "jade", "jfde", "brier_jade", "miss_rate", "cost", "raw_jade", "all_jade", "rounds")))
    t = PROPERTY
    assert co["jade"] < t["jade"] < fc["jade"], (co["jade"], fc["jade"])
    assert co["miss_rate"] < t["miss"] < fc["miss_rate"], (co["miss_rate"], fc["miss_rate"])
    for v in (co, fc):
        assert v["all_jade"] <= v["jade"] <= v["raw_jade"], v
    return co, fc
