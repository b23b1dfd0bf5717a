"""float64 checker of the joint best-of-K evaluation of the full-covariance
head (g2k_fullcov_joint_eval_f32; csrc/g2k_joint.hip states the
definition): tests/joint_ref.joint_eval_ref with one change — joint sample k is
tests/fullcov_ref.sample at seed (seed + k) mod 2^64 and factor ``chol``.  Built
from the parts of the existing checkers (draw_errors, pair_mask, min_dist,
count); returns the same dictionary, the col_lo / col_hi / amb_* bracket fields
included.  Test helper, not a test module."""
import numpy as np

from tests import fullcov_ref as fr
from tests.bestk_ref import L, MASK64, draw_errors, pair_mask
from tests.joint_ref import EPS, count, min_dist


def _band_xy(x):
    """[S, F, 2L, N] (band layout) -> [S, F, L, N, 2]."""
    return np.stack([x[:, :, :L], x[:, :, L:]], axis=-1)


def walk_factor(sigma, rng):
    """A test factor [24, 24] f32: L[i][j] = sigma / sqrt(12) for j <= i with
    i - j even (a random walk per coordinate whose last step has standard
    deviation sigma), plus tril(0.05 sigma N(0, 1)) so that every entry of the
    triangle is exercised; diagonal |.| + 0.02 sigma.  Zeros above the diagonal
    (the GPU tests put NaN there: those entries are never read)."""
    i, j = np.indices((fr.DIM, fr.DIM))
    Lm = np.where((j <= i) & ((i - j) % 2 == 0), sigma / np.sqrt(12.0), 0.0)
    Lm = Lm + np.tril(0.05 * sigma * rng.standard_normal((fr.DIM, fr.DIM)))
    d = np.arange(fr.DIM)
    Lm[d, d] = np.abs(Lm[d, d]) + 0.02 * sigma
    return Lm.astype(np.float32)


def nan_above(chol):
    """The factor with NaN above the diagonal."""
    out = np.array(chol, np.float32)
    out[np.triu_indices(fr.DIM, 1)] = np.nan
    return out


def joint_eval_ref(pred, targets, n_active, chol, seed, K, radius, n_frames=None, ped_mask=None,
                   eps=EPS):
    """-> the dictionary of tests/joint_ref.joint_eval_ref."""
    pred = np.asarray(pred, np.float64)
    targets = np.asarray(targets, np.float64)
    S, F, _, N = pred.shape
    m = pair_mask(S, F, N, n_active, n_frames, ped_mask)
    P = m.sum(axis=2)
    couples = m[:, :, :, None] & m[:, :, None, :] & np.triu(np.ones((N, N), bool), 1)
    PP = couples.sum(axis=(2, 3))
    assert np.array_equal(PP, P * (P - 1) // 2)
    Pd = np.maximum(P, 1)
    jade_k, jfde_k = np.zeros((K, S, F)), np.zeros((K, S, F))
    col_k, col_lo, col_hi, amb_k = (np.zeros((K, S, F), np.int64) for _ in range(4))
    for k in range(K):
        x = fr.sample(pred, chol, (int(seed) + k) & MASK64)
        a, f = draw_errors(x, targets)
        jade_k[k] = (a * m).sum(axis=2) / Pd
        jfde_k[k] = (f * m).sum(axis=2) / Pd
        col_k[k], col_lo[k], col_hi[k], amb_k[k] = count(min_dist(_band_xy(x)), couples, radius, eps)
    col_pred, pred_lo, pred_hi, amb_pred = count(min_dist(_band_xy(pred)), couples, radius, eps)
    tg = np.broadcast_to(targets, (S, F, N, L, 2)).transpose(0, 1, 3, 2, 4)
    col_gt, gt_lo, gt_hi, amb_gt = count(min_dist(tg), couples, radius, eps)
    on = P > 0
    kJA, kJF = jade_k.argmin(axis=0), jfde_k.argmin(axis=0)          # the first (lowest) minimum
    pf = np.stack([jade_k.min(axis=0), jfde_k.min(axis=0), kJA.astype(np.float64),
                   kJF.astype(np.float64)], axis=-1) * on[..., None]
    col_best = np.take_along_axis(col_k, kJA[None], axis=0)[0]
    pi = np.stack([P, PP, col_pred, col_gt, col_k.sum(axis=0), col_best], axis=-1).astype(np.int64)
    pi = pi * on[..., None]
    sums_f = np.zeros((S, 4))
    sums_f[:, 0] = (P * pf[..., 0]).sum(axis=1)
    sums_f[:, 1] = (P * pf[..., 1]).sum(axis=1)
    sums_f[:, 2] = K
    return dict(per_frame_f=pf, per_frame_i=pi, sums_f=sums_f, sums_i=pi.sum(axis=1), members=m,
                jade_k=jade_k, jfde_k=jfde_k, col_k=col_k, col_lo=col_lo, col_hi=col_hi, amb_k=amb_k,
                pred_lo=pred_lo, pred_hi=pred_hi, amb_pred=amb_pred, gt_lo=gt_lo, gt_hi=gt_hi,
                amb_gt=amb_gt)


def recount(xs, members, radius, rel):
    """The device's own draws recounted in float64: xs [K, S, F, 24, N] (f32
    coordinates, band layout; non-members may hold anything), members [S, F, N]
    -> (lo, hi, amb) [K, S, F]: the member couples below radius (1 - rel),
    below radius (1 + rel), and between the two."""
    xs = np.asarray(xs, np.float64)
    K, S, F, _, N = xs.shape
    couples = members[:, :, :, None] & members[:, :, None, :] & np.triu(np.ones((N, N), bool), 1)
    lo, hi = np.zeros((K, S, F), np.int64), np.zeros((K, S, F), np.int64)
    for k in range(K):
        x = np.where(members[:, :, None, :], xs[k], 0.0)
        d = min_dist(_band_xy(x))
        lo[k] = ((d < radius * (1.0 - rel)) & couples).sum(axis=(2, 3))
        hi[k] = ((d < radius * (1.0 + rel)) & couples).sum(axis=(2, 3))
    return lo, hi, hi - lo
