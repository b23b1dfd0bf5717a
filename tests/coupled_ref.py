"""float64 checker of the scene-coupled head (include/g2k_coupled.h states the
definition): r_gi = c_g + e_gi over the members of a scene-frame.  The within-
and between-group sums, the counts, the method-of-moments fit with its
projection, the whitener (A, lambda), both NLLs from the whitened residuals, a
dense (24 P x 24 P) Gaussian density to hold them against, and the sampler (the
generator restatement is tests/fullcov_ref.py's, the scene-frame's normals its
column 0 under the salted seed).  Non-members are never touched (they may hold
NaN); entries of the factors above the diagonal are never read.  Test helper,
not a test module."""
import numpy as np

from tests import fullcov_ref as fr
from tests.bestk_ref import MASK64, pair_mask

L = 12
DIM = 24
SALT = 0x9E3779B97F4A6000
LOG_2PI = float(np.log(2.0 * np.pi))


def group_residuals(pred, targets, n_active, n_frames=None, ped_mask=None):
    """-> list of r [P, 24] float64, one per scene-frame (s, f) in order, P >= 0."""
    pred, targets = np.asarray(pred), np.asarray(targets)
    S, F, _, N = pred.shape
    m = pair_mask(S, F, N, n_active, n_frames, ped_mask)
    if targets.shape[1] != F:
        targets = np.broadcast_to(targets, (S, F) + targets.shape[2:])
    out = []
    for s in range(S):
        for f in range(F):
            idx = np.flatnonzero(m[s, f])
            tg = targets[s, f, idx].astype(np.float64)                     # [P, 12, 2]
            pr = pred[s, f][:, idx].T.astype(np.float64)                   # [P, 24] band
            r = np.empty((len(idx), DIM))
            r[:, 0::2] = tg[:, :, 0] - pr[:, :L]
            r[:, 1::2] = tg[:, :, 1] - pr[:, L:]
            out.append(r)
    return out


def sums(groups):
    """-> dict(within, between [24, 24], counts [4] int64 {N, G, groups with P >= 2, sum P^2})."""
    ssw, ssb = np.zeros((DIM, DIM)), np.zeros((DIM, DIM))
    c = np.zeros(4, np.int64)
    for r in groups:
        P = len(r)
        if P == 0:
            continue
        rb = r.mean(axis=0)
        e = r - rb
        ssw += e.T @ e
        ssb += P * np.outer(rb, rb)
        c += [P, 1, P >= 2, P * P]
    return dict(within=ssw, between=ssb, counts=c)


def sums_loops(groups):
    """``sums`` by plain loops over the members and the coordinates."""
    ssw = [[0.0] * DIM for _ in range(DIM)]
    ssb = [[0.0] * DIM for _ in range(DIM)]
    c = [0, 0, 0, 0]
    for r in groups:
        P = len(r)
        if P == 0:
            continue
        rb = [sum(float(r[i][a]) for i in range(P)) / P for a in range(DIM)]
        for a in range(DIM):
            for b in range(DIM):
                for i in range(P):
                    ssw[a][b] += (float(r[i][a]) - rb[a]) * (float(r[i][b]) - rb[b])
                ssb[a][b] += P * rb[a] * rb[b]
        c[0] += P
        c[1] += 1
        c[2] += 1 if P >= 2 else 0
        c[3] += P * P
    return dict(within=np.array(ssw), between=np.array(ssb), counts=np.array(c, np.int64))


def moments_fit(within, between, counts):
    """W = SSW / (N - G) and the raw B = (SSB - G W) / N."""
    N, G = int(counts[0]), int(counts[1])
    W = within / (N - G)
    return W, (between - G * W) / N


def project(W, B_raw):
    """The fit's host half -> dict(Lw, Lb, A, lam, clipped, B): W ridged as the
    full-covariance fit, Lw = chol(W), Lw^-1 B_raw Lw^-T = V diag(l) V^T,
    negative l clipped, B = Lw V diag(l+) V^T Lw^T, Lb = chol(ridged B) or zeros."""
    Wr = fr.ridged(W, 1.0)
    Lw = np.linalg.cholesky(Wr)
    Li = np.linalg.solve(Lw, np.eye(DIM))
    M = Li @ B_raw @ Li.T
    l, V = np.linalg.eigh(0.5 * (M + M.T))
    lam = np.where(l > 0.0, l, 0.0)
    H = Lw @ V
    B = (H * lam) @ H.T
    Lb = np.linalg.cholesky(fr.ridged(B, 1.0)) if lam.max() > 0.0 else np.zeros((DIM, DIM))
    return dict(Lw=Lw, Lb=Lb, A=V.T @ Li, lam=lam, clipped=int((l < 0.0).sum()), B=B, W=Wr)


def whitener(Lw, Lb):
    """(A, lam) of given factors: A W A^T = I, A B A^T = diag(lam)."""
    Lw, Lb = fr.lower(Lw), fr.lower(Lb)
    Li = np.linalg.solve(Lw, np.eye(DIM))
    M = Li @ (Lb @ Lb.T) @ Li.T
    l, V = np.linalg.eigh(0.5 * (M + M.T))
    return V.T @ Li, np.where(l > 0.0, l, 0.0)


def nll_stats(groups, A, lam):
    """stats [6] of include/g2k_coupled.h from the whitened residuals y = A r."""
    qw = qb = lg = qi = 0.0
    n = 0
    for r in groups:
        P = len(r)
        if P == 0:
            continue
        y = r @ A.T
        yb = y.mean(axis=0)
        qw += ((y - yb) ** 2).sum()
        qb += (P * yb * yb / (1.0 + P * lam)).sum()
        lg += np.log1p(P * lam).sum()
        qi += (y * y / (1.0 + lam)).sum()
        n += P
    return np.array([0.5 * (qw + qb + lg), 0.5 * (qi + n * np.log1p(lam).sum()), qw, qb, lg, 0.0])


def group_nll(r, A, lam, log_det_lw):
    """One group's exact joint NLL, its constant included."""
    P = len(r)
    return float(nll_stats([r], A, lam)[0] + P * (L * LOG_2PI + log_det_lw))


def group_nll_independent(r, A, lam, log_det_lw):
    P = len(r)
    return float(nll_stats([r], A, lam)[1] + P * (L * LOG_2PI + log_det_lw))


def dense_nll(r, W, B):
    """-log N(vec(r); 0, I_P (x) W + 1 1^T (x) B): the 24 P x 24 P Gaussian."""
    P = len(r)
    C = np.kron(np.eye(P), W) + np.kron(np.ones((P, P)), B)
    v = r.reshape(-1)
    sign, logdet = np.linalg.slogdet(C)
    assert sign > 0
    return float(0.5 * (v @ np.linalg.solve(C, v) + logdet + P * DIM * LOG_2PI))


def stats_ref(pred, targets, n_active, whiten=None, n_frames=None, ped_mask=None):
    """g2k_coupled_stats_f32 -> dict(within, between, counts, stats); ``whiten``
    None or (A, lam)."""
    g = group_residuals(pred, targets, n_active, n_frames, ped_mask)
    out = sums(g)
    out["stats"] = np.zeros(6) if whiten is None else nll_stats(g, whiten[0], whiten[1])
    return out


def shared_part(shape, Lb, seed):
    """c [S, F, 1, 24]: Lb times the scene-frame's normals, the pair the
    generator forms for column 0's element under seed XOR SALT."""
    zc = fr.normals(shape, (int(seed) & MASK64) ^ SALT)[:, :, :1]           # [S, F, 1, 24]
    return zc @ fr.lower(Lb).T


def sample(pred, cpl, seed):
    """g2k_coupled_sample_f32 -> [S, F, 24, N] (band layout), float64."""
    pred = np.asarray(pred, np.float64)
    x = fr.normals(pred.shape, seed) @ fr.lower(cpl[0]).T + shared_part(pred.shape, cpl[1], seed)
    out = pred.copy()
    out[:, :, :L] += np.transpose(x[..., 0::2], (0, 1, 3, 2))
    out[:, :, L:] += np.transpose(x[..., 1::2], (0, 1, 3, 2))
    return out
