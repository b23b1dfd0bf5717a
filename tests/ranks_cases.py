"""The inputs of the sample-rank tests (tests/test_sample_ranks.py checks every
geometry claim below on the CPU and ranks the oracle's draws;
tests/test_sample_ranks_gpu.py runs the kernels on them).  The table is
tests/score_cases.py's — the smallest shapes that reach each path of a kernel
with sample_scores_kernel's geometry, which sample_ranks_kernel
(csrc/g2k_ranks.hip) has: G = min(256 // K, 32) pairs per pass, a lane owns
(pair, draw), FC = clamp(4 G // Nmax, 1, F) frames per workgroup, C = ceil(F /
FC) workgroups per scene (C > 1: the rows kernel) — with K inside 4..255 (k2
and k3 become k4, k256 becomes k255) and a bin count B per case: B = K + 1 (one
rank per bin), proper divisors, the maximum 64 and the minimum 1.  Head
parameters, the mixture block and the NaN poison in columns >= n_active as
there.  Test helper, not a test module."""
import functools

import numpy as np

from oracle import g2k_ref as ref
from tests import fullcov_ref
from tests import mix_eval_ref as me
from tests import mixture_ref as mr
from tests.bestk_ref import MASK64, draw_seed, pair_mask

L = 12
SEED = (11 << 32) + 8765
HEADS = ("per_step", "fullcov", "mix")

#  name      S  F  Nmax K    B   n_active     n_frames   mask   shared  geometry {G, FC, C}, passes of the
#                                                                       fullest workgroup, and what it reaches
CASES = [
    # the minimum K; G at its cap of 32 (K < 8); one rank per bin
    ("k4",     2, 2, 8,  4,   5,  [8, 5],      [2, 1],    True,  False, dict(g=32, fc=2, c=1), 1),
    # the evaluation's K; an empty scene; 32 pairs at G = 12: a partial last group (8 of 12); pairs
    # whose lanes straddle two waves
    ("k20",    3, 2, 16, 20,  21, [16, 7, 0],  [2, 1, 0], True,  False, dict(g=12, fc=2, c=1), 3),
    # three passes per workgroup and five workgroups per scene: the rows kernel; three ranks per bin
    ("passes", 2, 5, 32, 20,  7,  [32, 21],    None,      False, False, dict(g=12, fc=1, c=5), 3),
    # a pair's lanes at one wave exactly, and past it
    ("k64",    1, 1, 16, 64,  13, [2],         None,      False, False, dict(g=4, fc=1, c=1), 1),
    ("k65",    1, 1, 16, 65,  33, [3],         None,      False, False, dict(g=3, fc=1, c=1), 1),
    # the maximum K: one pair fills the workgroup, a pass per pair; the maximum B
    ("k255",   1, 1, 16, 255, 64, [3],         None,      False, False, dict(g=1, fc=1, c=1), 3),
    # G2K_STEP_TARGETS_SHARED; several frames in one workgroup
    ("shared", 2, 3, 16, 8,   3,  [16, 9],     [3, 2],    True,  True,  dict(g=32, fc=3, c=1), 2),
    # dense shapes, more pairs than lanes: 256 pairs at G = 32 (the cap: 192 of 256 lanes draw)
    ("n256",   2, 1, 256, 6,  7,  [256, 130],  None,      True,  False, dict(g=32, fc=1, c=1), 8),
    # FC cut by F and a last chunk shorter than FC: F = 3 at FC = 2; the minimum B
    ("tail",   1, 3, 12,  40, 1,  [5],         [3],       False, False, dict(g=6, fc=2, c=2), 2),
]
IDS = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def inputs(i):
    """Case i -> dict(pred, targets, head [3, 12], chol [24, 24], mix [8, 608],
    n_active, n_frames, ped_mask, pairs [S, F, N], K, B, seed, shared, geom,
    passes), float32 / int32 / uint8 host arrays."""
    _, S, F, N, K, B, nact, nfr, masked, shared, geom, passes = CASES[i]
    rng = np.random.default_rng(6100 + i)
    sx, sy = rng.uniform(0.1, 1.5, L), rng.uniform(0.1, 1.5, L)
    rho = rng.uniform(-0.9, 0.9, L)
    head = np.stack([np.log(sx), np.log(sy), np.arctanh(rho)]).astype(np.float32)
    # the full-covariance head: the same marginals, AR(1) 0.7 across the steps
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
                pairs=pair_mask(S, F, N, n_active, n_frames, pm), K=K, B=B, seed=SEED + i, shared=shared,
                geom=geom, passes=passes)


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


def sampler(which, c):
    """(pred, seed) -> one draw [S, F, 24, N] of head ``which`` with case c's
    parameters: the checkers' restatement of the head's sampler."""
    if which == "per_step":
        return lambda pred, seed: ref.gauss_sample(pred, c["head"], seed & MASK64)
    if which == "fullcov":
        return lambda pred, seed: fullcov_ref.sample(pred, c["chol"], seed & MASK64)
    return lambda pred, seed: mr.sample(pred, c["mix"], seed & MASK64)[0]


def scaled(which, c, by):
    """Case c with head ``which``'s factor (sigma; the Cholesky factor; the
    components' factors, offsets and weights as they are) scaled by ``by``."""
    c = dict(c)
    if which == "per_step":
        c["head"] = c["head"].copy()
        c["head"][:2] += np.float32(np.log(by))
    elif which == "fullcov":
        c["chol"] = (c["chol"] * by).astype(np.float32)
    else:
        c["mix"] = c["mix"].copy()
        c["mix"][:, 32:] *= np.float32(by)
    return c


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
