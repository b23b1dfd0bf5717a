"""The cells of the evaluation and train reductions that only production
sizes reach, as data (tests/test_eval_cells.py proves the claims on the CPU
from the library's own planning calls; tests/test_eval_cells_gpu.py,
tests/test_train_gpu.py and tests/test_ops_domain_gpu.py run the cells against
the float64 checkers; the KDE pair runs "ks32-fill" through tests/kde_cases.py).

A cell is a shape plus the geometry it is there to reach.  The claim is what
the cell is FOR; when a constant of a kernel moves, test_eval_cells.py fails
instead of the cell silently running some other trip count.  A claim is never
edited to follow the library: the shape is moved until the claim holds again.

Per-pair family (best_of_k_kernel<Head>, kde_nll_kernel<Head>; bestk_geom):
claim = KS lanes per pair, FC frames per workgroup, C workgroups per scene,
the fewest and the most draws a lane makes, whether K alone would let KS grow
further (the fill limit S F Nmax KS < 2 * 256 * 1024 stops it: the production
geometry), and the workgroups of g2k_bestk_rows_kernel / g2k_kde_rows_kernel
(ceil(S 8 / 256), launched only when C > 1).
Stats family (g2k_head_stats_kernel + g2k_head_stats_rows_kernel, g2k_fullcov_
stats_kernel + g2k_fullcov_rows_kernel; calib_geom / fullcov_geom): claim = W
workgroups (= workspace rows), U slots per workgroup.
Joint family (joint_kernel / joint_wave_kernel + g2k_joint_rows_kernel;
joint_geom): claim = waves per unit, KD units per scene-frame, and for the
one-wave kernel the lanes per group GL and the passes of slice 0's item list
(targets, mean, K draws) over the 64 / GL groups; the frames lane 0 of the rows
kernel adds (F > 64: two).
Train family (g2k_grad_rows_kernel<false / true>): claim = the gradient rows
(S x workgroups per scene; S for g2k_nll_f32), the trips of the r0 loop (256
rows each) and the rows of the last trip.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from tests import fullcov_joint_ref as fj
from tests.bestk_ref import pair_mask

SEED = (7 << 32) + 99
LEVELS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99)


# ---------------------------------------------------------------------------
# per-pair family
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class PairCell:
    id: str
    S: int
    F: int
    Nmax: int
    K: int
    n_active: tuple
    n_frames: tuple | None
    masked: bool
    sigma: float
    rng: int
    claim: dict = field(default_factory=dict)


def _pc(ks, fc, c, draws, by_fill, row_wgs):
    return dict(ks=ks, fc=fc, c=c, draws=draws, by_fill=by_fill, row_wgs=row_wgs)


# one scene at Nmax, one empty, the rest <= 6 (the real-data evaluation's crowd); the last
# scene (the rows kernels' second workgroup) has six pedestrians in both frames
KS32_N_ACTIVE = (3, 256, 0) + (1, 2, 3, 4, 5, 6) * 5
KS32_N_FRAMES = (2, 2, 2, 1, 2, 0) + (1, 2, 2) * 9

PER_PAIR = [
    # KS 8; K = 9 is no multiple of it: lane 0 makes two draws, the others one
    PairCell("ks8", 2, 2, 9, 9, (9, 4), (2, 1), True, 0.3, 301,
             _pc(8, 2, 1, (1, 2), False, 0)),
    # KS 32 because 33 * 2 * 256 * 16 < 2^19 <= ... * 32 (K = 64 alone would give 64);
    # C 2 and S 8 = 264 > 256: the rows kernels' second workgroup
    PairCell("ks32-fill", 33, 2, 256, 64, KS32_N_ACTIVE, KS32_N_FRAMES, True, 0.3, 302,
             _pc(32, 1, 2, (2, 2), True, 2)),
    # KS at its cap: one draw per lane, then two and three (K = 130)
    PairCell("ks64", 1, 1, 16, 64, (2,), None, False, 0.3, 303, _pc(64, 1, 1, (1, 1), False, 0)),
    PairCell("ks64-k130", 1, 1, 16, 130, (2,), None, False, 0.3, 304, _pc(64, 1, 1, (2, 3), False, 0)),
]


def dense_factor(rng, sigma):
    """Diagonal in [0.5, 1.5] sigma, off-diagonals of the same scale, NaN above
    (tests/test_fullcov_gpu.py's)."""
    Lm = sigma * rng.uniform(-1.0, 1.0, (24, 24))
    Lm[np.arange(24), np.arange(24)] = sigma * rng.uniform(0.5, 1.5, 24)
    Lm[np.triu_indices(24, 1)] = np.nan
    return Lm.astype(np.float32)


def _head(rng, sigma):
    return np.stack([np.log(sigma) + 0.2 * rng.standard_normal(12),
                     np.log(sigma) + 0.2 * rng.standard_normal(12),
                     0.5 * rng.standard_normal(12)]).astype(np.float32)


def _pred_targets(rng, S, F, N, sigma):
    pred = rng.standard_normal((S, F, 24, N)).astype(np.float32)
    base = pred.reshape(S, F, 2, 12, N).transpose(0, 1, 4, 3, 2)
    tg = (base + sigma * rng.standard_normal((S, F, N, 12, 2))).astype(np.float32)
    return pred, np.ascontiguousarray(tg)


def pair_inputs(c: PairCell):
    """Host arrays in the form of tests/test_best_of_k_gpu.py: targets = pred +
    sigma N(0, 1), a per-step head around sigma and a dense factor of that
    scale with NaN above the diagonal."""
    rng = np.random.default_rng(c.rng)
    pred, tg = _pred_targets(rng, c.S, c.F, c.Nmax, c.sigma)
    head = _head(rng, c.sigma)
    pm = (rng.random((c.S, c.Nmax)) > 0.2).astype(np.uint8) if c.masked else None
    return dict(pred=pred, targets=tg, head=head, chol=dense_factor(rng, c.sigma),
                n_active=np.array(c.n_active, np.int32),
                n_frames=None if c.n_frames is None else np.array(c.n_frames, np.int32),
                ped_mask=pm, K=c.K, seed=SEED)


# ---------------------------------------------------------------------------
# stats family
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class StatsCell:
    id: str
    S: int
    F: int
    Nmax: int
    rng: int
    claim: dict = field(default_factory=dict)


STATS = [
    # 17 rows: thread j = 1 of g2k_head_stats_rows_kernel holds slice 16; the
    # second trip (r0 = 16) of g2k_fullcov_rows_kernel, one row, 15 clamped loads
    StatsCell("w17", 17, 2, 256, 311, dict(w=17, u=512)),
    # 33 rows: the second trip (r0 += 32) of g2k_head_stats_rows_kernel; three of the other
    StatsCell("w33", 33, 2, 256, 312, dict(w=33, u=512)),
    # the cap of 256 workgroups with U = 544 > 512: 544 % 256 = 32, so a
    # workgroup's range ends inside a scene-frame
    StatsCell("cap", 17, 32, 256, 313, dict(w=256, u=544)),
]


def known_factor(rng):
    """tests/test_fullcov_gpu.py's: residuals r = L z with a banded L of scale 0.05."""
    Lm = np.zeros((24, 24))
    for i in range(24):
        for j in range(i + 1):
            Lm[i, j] = 0.05 * (1.0 if i == j else 0.6 ** ((i - j + 1) // 2)) * (0.5 + rng.random())
    return Lm


def stats_inputs(c: StatsCell):
    """Random n_active and n_frames including 0, one full scene, a random
    mask; residuals drawn from a known full-covariance factor; every element
    of pred and targets that is not a pair holds NaN (a finite output proves
    it was never read)."""
    rng = np.random.default_rng(c.rng)
    S, F, N = c.S, c.F, c.Nmax
    nact = rng.integers(0, N + 1, S)
    nfr = rng.integers(0, F + 1, S)
    nact[0], nfr[0] = N, F                                 # one full scene
    nact[1], nfr[3] = 0, 0                                 # apart: no trip of 16 rows without a pair
    nact[S - 1], nfr[S - 1] = max(nact[S - 1], N // 2), F  # the last workgroups' rows carry pairs
    nact, nfr = nact.astype(np.int32), nfr.astype(np.int32)
    pm = (rng.random((S, N)) > 0.2).astype(np.uint8)
    Lk = known_factor(rng)
    pred = rng.standard_normal((S, F, 24, N)).astype(np.float32)
    r = rng.standard_normal((S, F, N, 24)) @ Lk.T
    tg = np.empty((S, F, N, 12, 2))
    tg[..., 0] = np.transpose(pred[:, :, :12], (0, 1, 3, 2)) + r[..., 0::2]
    tg[..., 1] = np.transpose(pred[:, :, 12:], (0, 1, 3, 2)) + r[..., 1::2]
    tg = np.ascontiguousarray(tg.astype(np.float32))
    head = np.stack([np.log(0.08) + 0.2 * rng.standard_normal(12),
                     np.log(0.08) + 0.2 * rng.standard_normal(12),
                     0.5 * rng.standard_normal(12)]).astype(np.float32)
    chol = np.tril(Lk * rng.uniform(0.8, 1.25, (24, 24))).astype(np.float32)
    chol[np.triu_indices(24, 1)] = np.nan
    m = pair_mask(S, F, N, nact, nfr, pm)
    np.transpose(pred, (0, 1, 3, 2))[~m] = np.nan          # a view: pred itself
    tg[~m] = np.nan
    return dict(pred=pred, targets=tg, head=head, chol=chol, n_active=nact, n_frames=nfr,
                ped_mask=pm, pairs=int(m.sum()))


# ---------------------------------------------------------------------------
# joint family
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class JointCell:
    id: str
    S: int
    F: int
    Nmax: int
    K: int
    n_active: tuple
    n_frames: tuple | None
    masked: bool
    rng: int
    claim: dict = field(default_factory=dict)


SIGMA, RADIUS = 0.3, 0.3

JOINT = [
    # S F = 520 >= 512 above Nmax 64: one unit makes all K = 3 draws (plus the
    # targets and the mean), four waves; F = 65: lane 0 of g2k_joint_rows_kernel
    # adds frames 0 and 64
    JointCell("kd1-waves", 8, 65, 65, 3, (65, 64, 33, 2, 0, 65, 17, 1),
              (65, 64, 65, 1, 65, 0, 65, 65), True, 201,
              dict(waves=4, kd=1, gl=0, passes=0, lane0_frames=2)),
    # S F = 2048: one unit, one wave; P <= 4: groups of 16 lanes, so the seven
    # items (targets, mean, five draws) take two passes over the four groups
    JointCell("kd1-wave", 64, 32, 4, 5, tuple(int(v) for v in (np.arange(64) * 7 + 3) % 5), None,
              False, 202, dict(waves=1, kd=1, gl=16, passes=2, lane0_frames=1)),
]


def joint_inputs(c: JointCell):
    """Host arrays in the form of tests/test_joint_eval_gpu.py, plus the walk
    factor of tests/test_fullcov_joint_gpu.py (NaN above the diagonal)."""
    rng = np.random.default_rng(c.rng)
    pred, tg = _pred_targets(rng, c.S, c.F, c.Nmax, SIGMA)
    head = _head(rng, SIGMA)
    pm = (rng.random((c.S, c.Nmax)) > 0.2).astype(np.uint8) if c.masked else None
    chol = fj.nan_above(fj.walk_factor(SIGMA, np.random.default_rng(c.rng + 1000)))
    return dict(pred=pred, targets=tg, head=head, chol=chol, n_active=np.array(c.n_active, np.int32),
                n_frames=None if c.n_frames is None else np.array(c.n_frames, np.int32), ped_mask=pm,
                K=c.K, seed=SEED)


# ---------------------------------------------------------------------------
# train family
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class TrainCell:
    id: str
    S: int
    split: int
    Nmax: int
    F: int
    H: int
    claim: dict = field(default_factory=dict)      # rows, trips, last (rows of the last trip)


ROWS_PER_TRIP = 256            # g2k_grad_rows_kernel: 32 slices x 8 loads in flight

TRAIN = [
    TrainCell("rows260", 65, 4, 7, 5, 64, dict(rows=260, trips=2, last=4)),
    TrainCell("rows516", 129, 4, 7, 5, 64, dict(rows=516, trips=3, last=4)),
]
# g2k_nll_f32: one row per scene through the same kernel
NLL = TrainCell("nll-rows257", 257, 1, 3, 1, 64, dict(rows=257, trips=2, last=1))


def train_n_frames(c: TrainCell):
    """Frames per scene including 0, 1 and fewer than the split (a workgroup
    without a frame), one scene with every frame; the last scene (the rows of
    the last trip) has every frame too."""
    nf = np.random.default_rng(400 + c.S).integers(0, c.F + 1, c.S).astype(np.int32)
    nf[:4] = [c.F, 0, 1, 3]
    nf[-1] = c.F
    return nf


def train_mask(c: TrainCell):
    m = np.ones((c.S, c.Nmax), bool)
    m[1::3, 1::2] = False
    return m
