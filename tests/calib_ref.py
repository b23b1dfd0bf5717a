"""float64 checker of the head calibration (g2k_head_stats_f32;
csrc/g2k_calib.hip states the definition): the per-step residual moments over
the pairs, the squared Mahalanobis distance q and the NLL of a given head (the
formula of oracle.g2k_ref.bivariate_nll), the counts of q <= r2 per level, and
the closed-form maximum-likelihood head with its clamps.  Non-pairs are never
touched (they may hold NaN).  Test helper, not a test module."""
import numpy as np

from oracle import g2k_ref as ref
from tests.bestk_ref import pair_mask

L = 12
VAR_FLOOR = 1e-12
RHO_MAX = 1.0 - 1e-6


def levels_r2(levels):
    """Level p -> the chi^2(2) radius: q <= -2 ln(1 - p) holds with probability p."""
    return -2.0 * np.log1p(-np.asarray(levels, np.float64))


def residuals(pred, targets, n_active, n_frames=None, ped_mask=None):
    """-> (dx [P, L], dy [P, L]) float64 over the P pairs, in (s, f, n) order."""
    pred = np.asarray(pred)
    targets = np.asarray(targets)
    S, F, _, N = pred.shape
    m = pair_mask(S, F, N, n_active, n_frames, ped_mask)
    if targets.shape[1] != F:                                   # shared targets [S, 1, N, L, 2]
        targets = np.broadcast_to(targets, (S, F) + targets.shape[2:])
    tg = targets[m].astype(np.float64)                          # [P, L, 2]
    pr = np.transpose(pred, (0, 1, 3, 2))[m].astype(np.float64)  # [P, 2L]
    return tg[:, :, 0] - pr[:, :L], tg[:, :, 1] - pr[:, L:]


def fit_from_moments(n, sxx, syy, sxy):
    """The closed-form head [3, L] (float64) from the per-step sums."""
    n, sxx, syy, sxy = (np.asarray(v, np.float64) for v in (n, sxx, syy, sxy))
    fit = np.zeros((3, len(n)))
    for t in range(len(n)):
        if n[t] <= 0:
            continue
        fit[0, t] = 0.5 * np.log(max(sxx[t] / n[t], VAR_FLOOR))
        fit[1, t] = 0.5 * np.log(max(syy[t] / n[t], VAR_FLOOR))
        rho = 0.0
        if sxx[t] != 0.0 and syy[t] != 0.0:
            rho = sxy[t] / np.sqrt(sxx[t] * syy[t])
        fit[2, t] = np.arctanh(min(max(rho, -RHO_MAX), RHO_MAX))
    return fit


def q_nll(dx, dy, head):
    """-> (q [P, L], nll [P, L]) of the residuals under head [3, L]."""
    head = np.asarray(head, np.float64)
    sx, sy, rho = np.exp(head[0]), np.exp(head[1]), np.tanh(head[2])
    c = 1.0 - rho * rho
    a, b = dx / sx, dy / sy
    q = (a * a + b * b - 2 * rho * a * b) / c
    return q, ref.LOG_2PI + head[0] + head[1] + 0.5 * np.log(c) + q / 2


def head_stats_ref(pred, targets, n_active, head=None, r2=(), n_frames=None, ped_mask=None):
    """-> dict(stats [L, 8], abs [L, 8] (the sums of |term|: the scale of a
    summation-order difference), inside [L, NL] int64, fit [3, L] float64,
    q [P, L] or None, pairs)."""
    dx, dy = residuals(pred, targets, n_active, n_frames, ped_mask)
    P = dx.shape[0]
    r2 = np.asarray(r2, np.float64).reshape(-1)
    stats = np.zeros((L, 8))
    mag = np.zeros((L, 8))
    terms = [np.ones_like(dx), dx, dy, dx * dx, dy * dy, dx * dy]
    q = None
    if head is not None:
        q, nll = q_nll(dx, dy, head)
        terms += [nll, q]
    for i, v in enumerate(terms):
        stats[:, i] = v.sum(axis=0)
        mag[:, i] = np.abs(v).sum(axis=0)
    inside = np.zeros((L, len(r2)), np.int64)
    if q is not None:
        inside[:] = (q[:, :, None] <= r2[None, None, :]).sum(axis=0)
    fit = fit_from_moments(stats[:, 0], stats[:, 3], stats[:, 4], stats[:, 5])
    return dict(stats=stats, abs=mag, inside=inside, fit=fit, q=q, pairs=P)
