"""The inputs of the sample-modes tests (tests/test_sample_modes.py checks
every geometry claim below on the CPU and reduces the oracle's draws;
tests/test_sample_modes_gpu.py runs the kernels on them).  The shapes are the
smallest that reach each path of sample_modes_kernel (csrc/g2k_modes.hip): a
workgroup of 256 lanes takes G = min(256 // K, 64 // M, 32) pairs per pass, a
lane owns (pair, draw), FC = clamp(4 G // Nmax, 1, F) frames per workgroup, C =
ceil(F / FC) workgroups per scene (C > 1: the rows kernel).  Head parameters
as tests/score_cases.py: sigma in [0.1, 1.5], |rho| <= 0.9, the AR(1) 0.7
full-covariance factor; the mixture is tests/mix_eval_ref.py's block (slots
{0, 2, 5}, NaN in everything never read).  Columns >= n_active of pred and
targets hold NaN: a finite result never read them.  Test helper, not a test
module."""
import functools

import numpy as np

from oracle import g2k_ref as ref
from tests import fullcov_ref
from tests import mix_eval_ref as me
from tests import mixture_ref as mr
from tests.bestk_ref import draw_seed, pair_mask

L = 12
SEED = (11 << 32) + 977
HEADS = ("per_step", "fullcov", "mix")
MISS_RADIUS = 0.75          # about the median cF of the cases: both sides of the count are reached

#  name         S  F  Nmax K    M   iters n_active     n_frames   mask   shared  geometry {G, FC, C}, passes
#                                                                                of the fullest workgroup
CASES = [
    # the centre is the mean of the draws, w = 1; G at its cap of 32
    ("m1",        1, 1, 8,   4,   1,  1,  [8],         None,      False, False, dict(g=32, fc=1, c=1), 1),
    # every draw its own cluster: centres = draws, w = 1/8, inertia 0; G = 64 // M
    ("mk",        1, 1, 8,   8,   8,  3,  [5],         None,      False, False, dict(g=8, fc=1, c=1), 1),
    # no iteration: the centres are the first 5 draws; FC cut by F
    ("it0",       1, 2, 8,   20,  5,  0,  [6],         None,      False, False, dict(g=12, fc=2, c=1), 1),
    # an empty scene; 7 pairs at G = 4: a partial last group (3 of 4); a pair's lanes at exactly one
    # wave; two workgroups per scene
    ("eval",      3, 2, 16,  64,  5,  10, [16, 7, 0],  [2, 1, 0], True,  False, dict(g=4, fc=1, c=2), 4),
    # a pair's lanes past one wave; odd K
    ("k65",       1, 1, 16,  65,  3,  8,  [3],         None,      False, False, dict(g=3, fc=1, c=1), 1),
    # the maximum K: one pair fills the workgroup, a pass per pair; 20 centres
    ("k256",      1, 1, 16,  256, 20, 5,  [3],         None,      False, False, dict(g=1, fc=1, c=1), 3),
    # the M cap: the largest centre block of a pair, G = 64 // 32 = 2 (80 of 256 lanes draw), and a
    # partial last group (1 of 2)
    ("m32",       1, 1, 8,   40,  32, 2,  [5],         None,      False, False, dict(g=2, fc=1, c=1), 3),
    # three passes per workgroup and five workgroups per scene: the rows kernel
    ("passes",    2, 5, 32,  20,  4,  4,  [32, 21],    None,      False, False, dict(g=12, fc=1, c=5), 3),
    # G2K_STEP_TARGETS_SHARED; several frames in one workgroup
    ("shared",    2, 3, 16,  8,   2,  3,  [16, 9],     [3, 2],    True,  True,  dict(g=32, fc=3, c=1), 2),
    # dense shapes, more pairs than lanes: 256 pairs at G = 32 (192 of 256 lanes draw)
    ("n256",      2, 1, 256, 6,   2,  4,  [256, 130],  None,      True,  False, dict(g=32, fc=1, c=1), 8),
    # a last chunk shorter than FC: F = 3 at FC = 2
    ("tail",      1, 3, 12,  40,  3,  3,  [5],         [3],       False, False, dict(g=6, fc=2, c=2), 2),
    # every draw equals the mean (sigma underflows to 0; a zero factor): all draws tie at distance 0
    # and go to centre 0, centres 1..3 are empty and keep their place.  The only case that reaches
    # the empty-cluster branch.  The per-step and the full-covariance head only: a mixture's draws
    # differ by their components' offsets
    ("collapsed", 1, 2, 8,   16,  4,  3,  [6],         None,      False, False, dict(g=16, fc=2, c=1), 1),
]
IDS = [c[0] for c in CASES]
# The row run at the boundary seed A (tests/bestk_ref.py: draw 1's seed carries out of the low word).  The
# smallest row, m1, has one centre: its integer outputs (mA = mF = 0, live = 1) are the same whatever the
# draws, so they could not tell a dropped carry; the next-smallest, mk, is taken for every head.
BOUNDARY_ROW = "mk"


def heads_of(i):
    return HEADS[:2] if IDS[i] == "collapsed" else HEADS


ALL = [(i, w) for i in range(len(CASES)) for w in heads_of(i)]
ALL_IDS = [f"{IDS[i]}-{w}" for i, w in ALL]


@functools.lru_cache(maxsize=None)
def inputs(i):
    """Case i -> dict(pred, targets, head [3, 12], chol [24, 24], mix [8, 608],
    n_active, n_frames, ped_mask, pairs [S, F, N], K, M, iters, seed, shared,
    geom, passes), float32 / int32 / uint8 host arrays."""
    name, S, F, N, K, M, iters, nact, nfr, masked, shared, geom, passes = CASES[i]
    rng = np.random.default_rng(7300 + i)
    sx, sy = rng.uniform(0.1, 1.5, L), rng.uniform(0.1, 1.5, L)
    rho = rng.uniform(-0.9, 0.9, L)
    head = np.stack([np.log(sx), np.log(sy), np.arctanh(rho)]).astype(np.float32)
    # the full-covariance head: the same marginals, AR(1) 0.7 across the steps
    B = fullcov_ref.block_factor(head)
    T = 0.7 ** np.abs(np.subtract.outer(np.arange(L), np.arange(L)))
    chol = np.linalg.cholesky(B @ np.kron(T, np.eye(2)) @ B.T).astype(np.float32)
    w = rng.uniform(0.2, 1.0, 3)
    bs = 1.5 * rng.standard_normal((3, 2 * L))
    mix = me.make_block(w, bs, [chol] * 3, me.SLOTS3)
    if name == "collapsed":
        head = np.stack([np.full(L, -200.0), np.full(L, -200.0), np.zeros(L)]).astype(np.float32)
        chol = np.zeros((2 * L, 2 * L), np.float32)
    pred = rng.standard_normal((S, F, 2 * L, N)).astype(np.float32)
    Ft = 1 if shared else F
    mu = pred[:, :Ft].reshape(S, Ft, 2, L, N).transpose(0, 1, 4, 3, 2)        # [S, Ft, N, L, 2]
    sig = np.stack([sx, sy], axis=-1)                                         # [L, 2]
    tg = (mu + sig * rng.standard_normal((S, Ft, N, L, 2))).astype(np.float32)
    n_active = np.array(nact, np.int32)
    for s in range(S):                       # never read: poison
        pred[s, :, :, n_active[s]:] = np.nan
        tg[s, :, n_active[s]:] = np.nan
    pm = None
    if masked:
        pm = (rng.random((S, N)) > 0.25).astype(np.uint8)
        pm[:, 0] = 1
    n_frames = None if nfr is None else np.array(nfr, np.int32)
    return dict(pred=pred, targets=np.ascontiguousarray(tg), head=head, chol=chol, mix=mix,
                n_active=n_active, n_frames=n_frames, ped_mask=pm,
                pairs=pair_mask(S, F, N, n_active, n_frames, pm), K=K, M=M, iters=iters, seed=SEED + i,
                shared=shared, geom=geom, passes=passes)


def passes_of(i):
    """The passes of case i's fullest workgroup under its claimed geometry: a
    workgroup walks the nfc * n_active slots of its frames (masked pedestrians
    included), G at a time."""
    c = inputs(i)
    S, F = c["pred"].shape[:2]
    g = c["geom"]
    worst = 0
    for s in range(S):
        nf = F if c["n_frames"] is None else int(c["n_frames"][s])
        for ch in range(g["c"]):
            nfc = min(max(nf - ch * g["fc"], 0), min(g["fc"], F - ch * g["fc"]))
            worst = max(worst, -(-nfc * int(c["n_active"][s]) // g["g"]))
    return worst


@functools.lru_cache(maxsize=None)
def oracle_draws(i, which, seed=None, carry=True):
    """[K, S, F, 24, N] float32: the checkers' restatement of the sampler's
    draws for seeds seed + k (oracle/g2k_ref.py gauss_sample, tests/
    fullcov_ref.py sample, tests/mixture_ref.py sample; ``seed`` None: the
    case's own), rounded to the sampler's fp32; ``carry=False``:
    tests/bestk_ref.draw_seed's."""
    c = inputs(i)
    seeds = [draw_seed(c["seed"] if seed is None else seed, k, carry) for k in range(c["K"])]
    with np.errstate(invalid="ignore"):
        if which == "per_step":
            d = [ref.gauss_sample(c["pred"], c["head"], s) for s in seeds]
        elif which == "fullcov":
            d = [fullcov_ref.sample(c["pred"], c["chol"], s) for s in seeds]
        else:
            d = [mr.sample(c["pred"], c["mix"], s)[0] for s in seeds]
    return np.stack(d).astype(np.float32)


@functools.lru_cache(maxsize=None)
def oracle_modes(i, which):
    """tests/modes_ref.py on the oracle's draws of case i (computed once)."""
    from tests import modes_ref
    c = inputs(i)
    return modes_ref.sample_modes_ref(oracle_draws(i, which), c["targets"], c["pairs"], c["M"],
                                      c["iters"], MISS_RADIUS)
