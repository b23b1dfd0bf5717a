"""The inputs of the KDE-NLL tests (tests/test_kde_nll.py measures the GPU
gate and the clip-boundary share on them with the oracle's draws;
tests/test_kde_nll_gpu.py runs the kernels on them).  The shapes are the
smallest that reach each path of kde_nll_kernel (csrc/g2k_kde.hip; KS = lanes
per pair, g2k_bestk_geom.h).  sigma in [0.1, 1.5], |rho| <= 0.9.  Columns >=
n_active of pred and targets hold NaN: a finite result never read them.  Test
helper, not a test module."""
import functools

import numpy as np

from oracle import g2k_ref as ref
from tests import eval_cells as ec
from tests import fullcov_ref
from tests.bestk_ref import MASK64, pair_mask

L = 12
SEED = (5 << 32) + 1234
HEADS = ("per_step", "fullcov")

#  name      S  F  Nmax K    n_active     n_frames   mask   shared displaced   what it reaches
CASES = [
    ("k5",     3, 2, 16, 5,   [16, 7, 0],  [2, 1, 0], True,  False, False),  # K not a multiple of KS (4)
    ("chunks", 2, 5, 32, 20,  [32, 21],    None,      False, False, False),  # 5 chunks: the rows kernel
    ("k64",    1, 1, 16, 64,  [2],         None,      False, False, False),  # KS at its cap (64)
    ("k200",   1, 1, 16, 200, [3],         None,      False, False, False),  # several draws per lane
    ("k4",     2, 2, 8,  4,   [8, 5],      [2, 2],    True,  False, False),  # the minimum K
    ("shared", 2, 3, 16, 8,   [16, 9],     [3, 2],    True,  True,  False),  # G2K_STEP_TARGETS_SHARED
    ("far",    2, 2, 16, 20,  [16, 11],    None,      False, False, True),   # targets >= 4 sigma away: clips
    # tests/eval_cells.py "ks32-fill": KS 32 cut by the fill limit (K alone would give 64), two
    # chunks per scene and S 8 > 256: the rows kernel's second workgroup
    ("ks32fill", 33, 2, 256, 64, list(ec.KS32_N_ACTIVE), list(ec.KS32_N_FRAMES), True, False, False),
]
IDS = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def inputs(i):
    """Case i -> dict(pred, targets, head [3, 12], chol [24, 24], n_active,
    n_frames, ped_mask, pairs [S, F, N], K, seed, shared), float32 / int32 /
    uint8 host arrays."""
    _, S, F, N, K, nact, nfr, masked, shared, far = CASES[i]
    rng = np.random.default_rng(4100 + i)
    sx, sy = rng.uniform(0.1, 1.5, L), rng.uniform(0.1, 1.5, L)
    rho = rng.uniform(-0.9, 0.9, L)
    head = np.stack([np.log(sx), np.log(sy), np.arctanh(rho)]).astype(np.float32)
    # the full-covariance head: the same marginals, AR(1) 0.7 across the steps
    B = fullcov_ref.block_factor(head)
    T = 0.7 ** np.abs(np.subtract.outer(np.arange(L), np.arange(L)))
    chol = np.linalg.cholesky(B @ np.kron(T, np.eye(2)) @ B.T).astype(np.float32)
    pred = rng.standard_normal((S, F, 2 * L, N)).astype(np.float32)
    Ft = 1 if shared else F
    mu = pred[:, :Ft].reshape(S, Ft, 2, L, N).transpose(0, 1, 4, 3, 2)        # [S, Ft, N, L, 2]
    sig = np.stack([sx, sy], axis=-1)                                         # [L, 2]
    if far:
        ang = rng.uniform(0, 2 * np.pi, (S, Ft, N, L))
        r = rng.uniform(4.0, 7.0, (S, Ft, N, L))
        off = np.stack([np.cos(ang), np.sin(ang)], axis=-1) * r[..., None]
    else:
        off = rng.standard_normal((S, Ft, N, L, 2))
    tg = (mu + sig * off).astype(np.float32)
    n_active = np.array(nact, np.int32)
    for s in range(S):                       # never read: poison
        pred[s, :, :, n_active[s]:] = np.nan
        tg[s, :, n_active[s]:] = np.nan
    pm = None
    if masked:
        pm = (rng.random((S, N)) > 0.25).astype(np.uint8)
        pm[:, 0] = 1
    n_frames = None if nfr is None else np.array(nfr, np.int32)
    return dict(pred=pred, targets=np.ascontiguousarray(tg), head=head, chol=chol, n_active=n_active,
                n_frames=n_frames, ped_mask=pm, pairs=pair_mask(S, F, N, n_active, n_frames, pm),
                K=K, seed=SEED + i, shared=shared)


@functools.lru_cache(maxsize=None)
def oracle_draws(i, which):
    """[K, S, F, 24, N] float32: the oracle's restatement of the sampler's
    draws for seeds seed + k (oracle/g2k_ref.py gauss_sample, tests/
    fullcov_ref.py sample), rounded to the sampler's fp32."""
    c = inputs(i)
    with np.errstate(invalid="ignore"):
        if which == "per_step":
            d = [ref.gauss_sample(c["pred"], c["head"], (c["seed"] + k) & MASK64) for k in range(c["K"])]
        else:
            d = [fullcov_ref.sample(c["pred"], c["chol"], (c["seed"] + k) & MASK64)
                 for k in range(c["K"])]
    return np.stack(d).astype(np.float32)
