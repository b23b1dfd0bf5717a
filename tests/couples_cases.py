"""The inputs of the couple-score tests (tests/test_couple_scores.py checks every
geometry claim below on the CPU; tests/test_couple_scores_gpu.py runs the
kernels on them): the smallest shapes that reach each path of
couple_scores_kernel's geometry (csrc/g2k_couples.hip).  A pass of a workgroup
is a tile of TR row members x 16 column members of the compacted members, TR =
16 for K <= 22 and 8 above; only tiles that hold a couple a < b exist; TILES of
them when every column is a member, dealt round-robin to W = min(8, TILES,
ceil(2048 / (S F))) workgroups per scene-frame, PASSES = ceil(TILES / W); the
K + 2 items of a tile (the draws, the targets, the mean) are made 8 to a round.
Head parameters and the mixture block as tests/ranks_cases.py; columns >=
n_active, masked columns and frames >= n_frames hold NaN.  Test helper, not a
test module."""
import functools

import numpy as np

from tests import fullcov_ref
from tests import mix_eval_ref as me
from tests.bestk_ref import draw_seed, pair_mask
from tests.ranks_cases import HEADS, SEED, sampler   # noqa: F401 (re-exported)

L = 12
INF = float("inf")

#  name     S     F  Nmax K   B   n_active        n_frames      mask   shared reach  geometry, and what it reaches
CASES = [
    # the minimum K (4 items: half a round); P = 8, 2, 1 and 0 in one launch; an empty scene; n_frames < F
    ("k2",    4,    2, 8,   2,  3,  [8, 2, 1, 0],   [2, 1, 2, 0], False, False, INF, dict(tr=16, tiles=1, w=1, passes=1)),
    # the evaluation's K (22 items: a partial third round), one rank per bin; masked members; an empty
    # scene; one diagonal tile
    ("k20",   3,    2, 16,  20, 21, [16, 7, 0],     [2, 1, 0],    True,  False, INF, dict(tr=16, tiles=1, w=1, passes=1)),
    # three ranks per bin; three tiles (two diagonal, one full) on three workgroups; P = 21: no multiple
    # of a tile edge; a finite reach that scores some couples
    ("reach", 2,    5, 32,  20, 7,  [32, 21],       None,         False, False, 0.5, dict(tr=16, tiles=3, w=3, passes=1)),
    # a reach that scores none
    ("none",  1,    2, 16,  20, 7,  [12],           None,         False, False, 1e-3, dict(tr=16, tiles=1, w=1, passes=1)),
    # the maximum K (66 items: nine rounds): 8-row tiles, the second one's rows start inside a column block
    ("k64",   1,    1, 16,  64, 13, [13],           None,         False, False, INF, dict(tr=8, tiles=2, w=2, passes=1)),
    # the smallest K with 8-row tiles; 11 tiles on 8 workgroups: two passes; P no multiple of 8
    ("k23",   1,    2, 40,  23, 8,  [37],           None,         False, False, INF, dict(tr=8, tiles=11, w=8, passes=2)),
    # G2K_STEP_TARGETS_SHARED with several frames; 8 items: one full round; a finite reach
    ("shared", 2,   3, 16,  6,  7,  [16, 9],        [3, 2],       True,  True,  0.5, dict(tr=16, tiles=1, w=1, passes=1)),
    # the largest 16-row K (24 items: three full rounds); the minimum B
    ("k22",   1,    1, 16,  22, 1,  [16],           None,         False, False, INF, dict(tr=16, tiles=1, w=1, passes=1)),
    # dense: P = 256 (32 640 couples) and 130; 136 tiles on 8 workgroups: 17 passes
    ("n256",  2,    1, 256, 4,  5,  [256, 130],     None,         False, False, INF, dict(tr=16, tiles=136, w=8, passes=17)),
    # fewer workgroups than tiles, more than one: 10 tiles on 8
    ("deal",  64,   4, 64,  2,  1,  "random",       None,         True,  False, 0.3, dict(tr=16, tiles=10, w=8, passes=2)),
    # one workgroup per scene-frame takes every tile: 3 passes
    ("one",   2048, 1, 32,  3,  2,  "random",       None,         False, False, INF, dict(tr=16, tiles=3, w=1, passes=3)),
]
IDS = [c[0] for c in CASES]


def tiles_of(P, tr, tc=16):
    """The tiles (rb, cb) that hold a couple a < b < P, a in row block rb, b in
    column block cb, in the kernel's order."""
    out = []
    for rb in range(-(-P // tr)):
        for cb in range(-(-P // tc)):
            if max(cb * tc, rb * tr + 1) < min(P, (cb + 1) * tc):
                out.append((rb, cb))
    return out


@functools.lru_cache(maxsize=None)
def inputs(i):
    """Case i -> dict(pred, targets, head [3, 12], chol [24, 24], mix [8, 608],
    n_active, n_frames, ped_mask, members [S, F, N], K, B, seed, shared, reach,
    geom), float32 / int32 / uint8 host arrays."""
    _, S, F, N, K, B, nact, nfr, masked, shared, reach, geom = CASES[i]
    rng = np.random.default_rng(7300 + i)
    sx, sy = rng.uniform(0.1, 1.5, L), rng.uniform(0.1, 1.5, L)
    rho = rng.uniform(-0.9, 0.9, L)
    head = np.stack([np.log(sx), np.log(sy), np.arctanh(rho)]).astype(np.float32)
    Bf = fullcov_ref.block_factor(head)
    T = 0.7 ** np.abs(np.subtract.outer(np.arange(L), np.arange(L)))
    chol = np.linalg.cholesky(Bf @ np.kron(T, np.eye(2)) @ Bf.T).astype(np.float32)
    w = rng.uniform(0.2, 1.0, 3)
    bs = 1.5 * rng.standard_normal((3, 2 * L))
    mix = me.make_block(w, bs, [chol] * 3, me.SLOTS3)
    pred = rng.standard_normal((S, F, 2 * L, N)).astype(np.float32)
    Ft = 1 if shared else F
    mu = pred[:, :Ft].reshape(S, Ft, 2, L, N).transpose(0, 1, 4, 3, 2)        # [S, Ft, N, L, 2]
    sig = np.stack([sx, sy], axis=-1)                                         # [L, 2]
    tg = (mu + sig * rng.standard_normal((S, Ft, N, L, 2))).astype(np.float32)
    if isinstance(nact, str):
        n_active = rng.integers(0, N + 1, S).astype(np.int32)
        n_active[0], n_active[-1] = N, 0
    else:
        n_active = np.array(nact, np.int32)
    pm = None
    if masked:
        pm = (rng.random((S, N)) > 0.25).astype(np.uint8)
        pm[:, 0] = 1
    n_frames = None if nfr is None else np.array(nfr, np.int32)
    members = pair_mask(S, F, N, n_active, n_frames, pm)
    # never read: poison
    pred[~np.broadcast_to(members[:, :, None, :], pred.shape)] = np.nan
    tg[~np.broadcast_to(members.any(axis=1)[:, None, :, None, None] if shared
                        else members[:, :, :, None, None], tg.shape)] = np.nan
    return dict(pred=pred, targets=np.ascontiguousarray(tg), head=head, chol=chol, mix=mix,
                n_active=n_active, n_frames=n_frames, ped_mask=pm, members=members, K=K, B=B,
                seed=SEED + 40 + i, shared=shared, reach=reach, geom=geom)


def passes_of(i):
    """The passes of case i's fullest workgroup under its claimed geometry and
    its largest P: the live tiles of P dealt round-robin to w workgroups."""
    c = inputs(i)
    g = c["geom"]
    P = int(c["members"].sum(axis=2).max())
    return -(-len(tiles_of(P, g["tr"])) // g["w"])


@functools.lru_cache(maxsize=None)
def oracle_draws(i, which, seed=None, carry=True):
    """[K, S, F, 24, N] float32: the checkers' restatement of the sampler's
    draws for seeds seed + k (``seed`` None: the case's own), rounded to the
    sampler's fp32; ``carry=False``: tests/bestk_ref.draw_seed's."""
    c = inputs(i)
    draw = sampler(which, c)
    seed = c["seed"] if seed is None else seed
    with np.errstate(invalid="ignore"):
        d = [draw(c["pred"], draw_seed(seed, k, carry)) for k in range(c["K"])]
    return np.stack(d).astype(np.float32)


def property_setup(S=4, F=4, N=32, side=4.0, rng_seed=5):
    """The property test's predictions: constant-velocity means from a box of
    side ``side``, slope 0.4 N(0, 1) per coordinate -> pred [S, F, 24, N]."""
    rng = np.random.default_rng(rng_seed)
    start = rng.uniform(0.0, side, (S, F, 2, 1, N))
    slope = 0.4 * rng.standard_normal((S, F, 2, 1, N))
    path = start + slope * np.arange(L)[None, None, None, :, None]            # [S, F, 2, L, N]
    return path.reshape(S, F, 2 * L, N).astype(np.float32)


def coupled_targets(pred, sigma, share, rng_seed):
    """Targets [S, F, N, L, 2] float32 around pred with the head's marginals
    (N(0, sigma^2) per coordinate and step) whose residuals share ``share`` of
    their variance among the pedestrians of a scene-frame; share 0: the head's
    own independent law."""
    rng = np.random.default_rng(rng_seed)
    S, F, _, N = pred.shape
    mu = np.stack([pred[:, :, :L], pred[:, :, L:]], axis=-1).transpose(0, 1, 3, 2, 4)   # [S, F, N, L, 2]
    common = rng.standard_normal((S, F, 1, L, 2))
    own = rng.standard_normal((S, F, N, L, 2))
    return (mu + sigma * (np.sqrt(share) * common + np.sqrt(1.0 - share) * own)).astype(np.float32)
