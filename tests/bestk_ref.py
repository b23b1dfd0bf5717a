"""float64 checker of the best-of-K sampling evaluation (g2k_best_of_k_f32;
csrc/g2k_bestk.hip states the definition): K draws of oracle.g2k_ref
.gauss_sample at seeds (seed + k) mod 2^64, each pair's ADE / FDE per draw
(ade_l2 / fde_l2 of oracle/g2k_ref.py:400-401 applied to a draw), the
independent minima and the lowest index attaining each.  Test helper, not a
test module."""
import numpy as np

from oracle import g2k_ref as ref

L = 12
MASK64 = (1 << 64) - 1
# The seeds at which draw 1's 64-bit seed, which the kernels form in 32-bit halves (lo = seed_lo + k, hi =
# seed_hi + (lo < seed_lo)), carries out of the low word: A's draw 0 has the low word all ones and draw 1
# is 2^32; W's draw 1 wraps to seed 0.
SEED_A, SEED_W = (1 << 32) - 1, MASK64
BOUNDARY_SEEDS = {"A": SEED_A, "W": SEED_W}


def draw_seed(seed, k, carry=True):
    """Draw k's seed, (seed + k) mod 2^64; ``carry=False``: what a kernel that
    dropped the carry would use — the high word left at seed >> 32."""
    s = (int(seed) + k) & MASK64
    return s if carry else ((int(seed) & MASK64) >> 32 << 32) | (s & 0xFFFFFFFF)


def pair_mask(S, F, N, n_active, n_frames=None, ped_mask=None):
    """[S, F, N] bool: f < n_frames[s], n < n_active[s], ped_mask[s][n] != 0."""
    n_active = np.clip(np.asarray(n_active), 0, N)
    nf = np.full(S, F) if n_frames is None else np.clip(np.asarray(n_frames), 0, F)
    m = (np.arange(F)[None, :, None] < nf[:, None, None]) & \
        (np.arange(N)[None, None, :] < n_active[:, None, None])
    if ped_mask is not None:
        m = m & (np.asarray(ped_mask)[:, None, :] != 0)
    return m


def draw_errors(x, targets):
    """x [S, F, 2L, N] (band layout), targets [S, F or 1, N, L, 2] ->
    (ADE [S, F, N], FDE [S, F, N])."""
    xy = np.stack([x[:, :, :L], x[:, :, L:]], axis=-1)              # [S, F, L, N, 2]
    d = np.linalg.norm(np.transpose(xy, (0, 1, 3, 2, 4)) - np.asarray(targets, np.float64), axis=-1)
    return d.mean(axis=-1), d[..., L - 1]


def best_of_k_ref(pred, targets, n_active, head, seed, K, n_frames=None, ped_mask=None):
    """-> dict(per_ped [S, F, N, 4] = {minADE, minFDE, kA, kF} (zeros for
    non-pairs), out [S, 8], pairs [S, F, N] bool, ade_k / fde_k [K, S, F, N])."""
    pred = np.asarray(pred, np.float64)
    S, F, _, N = pred.shape
    m = pair_mask(S, F, N, n_active, n_frames, ped_mask)
    ade_k = np.empty((K, S, F, N))
    fde_k = np.empty((K, S, F, N))
    for k in range(K):
        ade_k[k], fde_k[k] = draw_errors(ref.gauss_sample(pred, head, (int(seed) + k) & MASK64), targets)
    kA, kF = ade_k.argmin(axis=0), fde_k.argmin(axis=0)              # the first (lowest) minimum
    per = np.stack([ade_k.min(axis=0), fde_k.min(axis=0), kA.astype(np.float64), kF.astype(np.float64)],
                   axis=-1) * m[..., None]
    pa, pf = draw_errors(pred, targets)
    out = np.zeros((S, 8))
    out[:, 0] = per[..., 0].sum(axis=(1, 2))
    out[:, 1] = per[..., 1].sum(axis=(1, 2))
    out[:, 2] = m.sum(axis=(1, 2))
    out[:, 3] = (pa * m).sum(axis=(1, 2))
    out[:, 4] = (pf * m).sum(axis=(1, 2))
    out[:, 5] = K
    return dict(per_ped=per, out=out, pairs=m, ade_k=ade_k, fde_k=fde_k)
