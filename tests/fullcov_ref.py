"""float64 checker of the full-covariance trajectory head (csrc/g2k_fullcov.hip
states the definition): coordinate i = 2 t + c, the draw x = mu + L z with the
normals of oracle.g2k_ref.gauss_sample (zero mean, unit head: it returns the
Box-Muller pair itself), each pair's ADE / FDE per draw and the lowest index
attaining each minimum (as tests/bestk_ref.py), the residuals' moments, the
ridged Cholesky fit, z = solve(L, r), the innovations q_t, the NLL and the
counts.  Non-pairs are never touched (they may hold NaN); entries of L above
the diagonal are never read.  Test helper, not a test module."""
import math

import numpy as np

from oracle import g2k_ref as ref
from tests.bestk_ref import MASK64, draw_errors, pair_mask

L = 12
DIM = 24
RIDGE_REL, RIDGE_ABS = 1e-6, 1e-12
_UNIT = np.zeros((3, L))


def chi2_even_quantile(p, dof):
    """The checker's own chi^2 quantile for even dof: Newton on the closed-form CDF."""
    m = dof // 2
    if m == 1:
        return -2.0 * math.log1p(-p)
    x = float(dof)
    for _ in range(200):
        h = 0.5 * x
        terms = [1.0]
        for j in range(1, m):
            terms.append(terms[-1] * h / j)
        cdf = 1.0 - math.exp(-h) * sum(terms)
        pdf = 0.5 * math.exp(-h) * terms[-1]
        step = (cdf - p) / pdf
        x -= step
        if abs(step) <= 1e-15 * x:
            break
    return x


def levels_r2(levels):
    """[2, NL]: the chi^2(2) radii (a step's innovation) and the chi^2(24) radii."""
    return np.array([[chi2_even_quantile(p, 2) for p in levels],
                     [chi2_even_quantile(p, DIM) for p in levels]], np.float64).reshape(2, -1)


def lower(chol):
    """The factor's lower triangle in float64 (what lies above is not read)."""
    return np.tril(np.where(np.tri(DIM, dtype=bool), np.asarray(chol, np.float64), 0.0))


def block_factor(head):
    """The per-step head [3, 12] as a block-diagonal factor (float64)."""
    h = np.asarray(head, np.float64)
    sx, sy, rho = np.exp(h[0]), np.exp(h[1]), np.tanh(h[2])
    Lm = np.zeros((DIM, DIM))
    for t in range(L):
        Lm[2 * t, 2 * t] = sx[t]
        Lm[2 * t + 1, 2 * t] = sy[t] * rho[t]
        Lm[2 * t + 1, 2 * t + 1] = sy[t] * np.sqrt(1 - rho[t] * rho[t])
    return Lm


def normals(shape, seed):
    """z [S, F, N, 24] for pred of ``shape`` [S, F, 24, N]: z[2t], z[2t+1] = (e1, e2) of step t."""
    e = ref.gauss_sample(np.zeros(shape), _UNIT, int(seed) & MASK64)      # [S, F, 24, N]: e1 rows, e2 rows
    z = np.empty((shape[0], shape[1], shape[3], DIM))
    z[..., 0::2] = np.transpose(e[:, :, :L], (0, 1, 3, 2))
    z[..., 1::2] = np.transpose(e[:, :, L:], (0, 1, 3, 2))
    return z


def sample(pred, chol, seed):
    """g2k_fullcov_sample_f32 -> [S, F, 24, N] (band layout), float64."""
    pred = np.asarray(pred, np.float64)
    x = normals(pred.shape, seed) @ lower(chol).T                        # [S, F, N, 24] time-major
    out = pred.copy()
    out[:, :, :L] += np.transpose(x[..., 0::2], (0, 1, 3, 2))
    out[:, :, L:] += np.transpose(x[..., 1::2], (0, 1, 3, 2))
    return out


def best_of_k_ref(pred, targets, n_active, chol, seed, K, n_frames=None, ped_mask=None):
    """-> dict(per_ped, out, pairs, ade_k, fde_k) as tests/bestk_ref.best_of_k_ref."""
    pred = np.asarray(pred, np.float64)
    S, F, _, N = pred.shape
    m = pair_mask(S, F, N, n_active, n_frames, ped_mask)
    ade_k = np.empty((K, S, F, N))
    fde_k = np.empty((K, S, F, N))
    for k in range(K):
        ade_k[k], fde_k[k] = draw_errors(sample(pred, chol, (int(seed) + k) & MASK64), targets)
    kA, kF = ade_k.argmin(axis=0), fde_k.argmin(axis=0)
    per = np.stack([ade_k.min(axis=0), fde_k.min(axis=0), kA.astype(np.float64), kF.astype(np.float64)],
                   axis=-1) * m[..., None]
    pa, pf = draw_errors(pred, targets)
    out = np.zeros((S, 8))
    out[:, 0] = per[..., 0].sum(axis=(1, 2))
    out[:, 1] = per[..., 1].sum(axis=(1, 2))
    out[:, 2] = m.sum(axis=(1, 2))
    out[:, 3] = np.where(m, pa, 0.0).sum(axis=(1, 2))
    out[:, 4] = np.where(m, pf, 0.0).sum(axis=(1, 2))
    out[:, 5] = K
    return dict(per_ped=per, out=out, pairs=m, ade_k=ade_k, fde_k=fde_k)


def residuals(pred, targets, n_active, n_frames=None, ped_mask=None):
    """-> r [P, 24] float64 over the P pairs, in (s, f, n) order, time-major."""
    pred = np.asarray(pred)
    targets = np.asarray(targets)
    S, F, _, N = pred.shape
    m = pair_mask(S, F, N, n_active, n_frames, ped_mask)
    if targets.shape[1] != F:
        targets = np.broadcast_to(targets, (S, F) + targets.shape[2:])
    tg = targets[m].astype(np.float64)                                   # [P, 12, 2]
    pr = np.transpose(pred, (0, 1, 3, 2))[m].astype(np.float64)          # [P, 24] band
    r = np.empty((tg.shape[0], DIM))
    r[:, 0::2] = tg[:, :, 0] - pr[:, :L]
    r[:, 1::2] = tg[:, :, 1] - pr[:, L:]
    return r


def ridged(M, n):
    C = np.array(M, np.float64) / n
    i = np.arange(DIM)
    C[i, i] = C[i, i] * (1 + RIDGE_REL) + RIDGE_ABS
    return C


def fit_from_moments(M, n):
    """The closed-form factor (float64): chol(ridged M / n); the identity when n = 0."""
    return np.linalg.cholesky(ridged(M, n)) if n > 0 else np.eye(DIM)


def stats_ref(pred, targets, n_active, chol=None, r2=None, n_frames=None, ped_mask=None):
    """-> dict(moments [25, 24], stats [12, 4], inside [13, NL] int64, fit
    [24, 24] float64, C (the ridged M / n, or None), q_t [P, 12] and q [P] (or
    None), pairs)."""
    r = residuals(pred, targets, n_active, n_frames, ped_mask)
    P = r.shape[0]
    moments = np.zeros((DIM + 1, DIM))
    moments[:DIM] = r.T @ r
    moments[DIM] = r.sum(axis=0)
    stats = np.zeros((L, 4))
    stats[:, 0] = P
    r2 = np.zeros((2, 0)) if r2 is None else np.asarray(r2, np.float64).reshape(2, -1)
    inside = np.zeros((L + 1, r2.shape[1]), np.int64)
    qt = q = None
    if chol is not None:
        Lm = lower(chol)
        z = np.linalg.solve(Lm, r.T).T if P else np.zeros((0, DIM))
        qt = z[:, 0::2] ** 2 + z[:, 1::2] ** 2                           # [P, 12]
        q = qt.sum(axis=1)
        d = np.log(np.diag(Lm))
        nll = ref.LOG_2PI + d[0::2][None] + d[1::2][None] + qt / 2
        stats[:, 1] = nll.sum(axis=0)
        stats[:, 2] = qt.sum(axis=0)
        inside[:L] = (qt[:, :, None] <= r2[0][None, None, :]).sum(axis=0)
        inside[L] = (q[:, None] <= r2[1][None, :]).sum(axis=0)
    return dict(moments=moments, stats=stats, inside=inside, fit=fit_from_moments(moments[:DIM], P),
                C=ridged(moments[:DIM], P) if P else None, q_t=qt, q=q, pairs=P)
