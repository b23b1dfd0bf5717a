"""float64 checker of the Gaussian-mixture trajectory head (include/g2k_mix.h
states the definition), over tests/fullcov_ref.py and the oracle's
gauss_sample: the parameter block, the max-shifted mixture log density and the
responsibilities, one EM step, the deterministic start, the selector (pcg_hash
and the f32 casts of u and cw exactly), the draw and best-of-K.  It imports
nothing from the package.  Dead slots (w == 0) are never read: they may hold
NaN.  Test helper, not a test module."""
import math

import numpy as np

from oracle import g2k_ref as ref
from tests import fullcov_ref as fr
from tests.bestk_ref import MASK64, draw_errors, pair_mask

SLOTS, PITCH, OFF_B, OFF_L = 8, 608, 8, 32
DIM, L = fr.DIM, fr.L
SEL_SALT = 0x9E3779B9
LOG_2PI = math.log(2.0 * math.pi)


def block(weights, means=None, chols=None):
    """[8, 608] float32 from up to 8 (w, b [24], L [24, 24]); slots past the
    given ones are dead (zeros)."""
    p = np.zeros((SLOTS, PITCH), np.float32)
    for m, w in enumerate(weights):
        p[m, 0] = w
        if means is not None:
            p[m, OFF_B:OFF_L] = means[m]
        p[m, OFF_L:] = np.asarray(np.eye(DIM) if chols is None else chols[m], np.float32).reshape(-1)
    return p


def live(mix):
    return np.asarray(mix, np.float32)[:, 0] != 0


def unpack(mix):
    """-> w [8], b [8, 24], Lm [8, 24, 24] float64; zeros for dead slots, whose
    other floats are not read; the factors' lower triangles only."""
    mix = np.asarray(mix, np.float32)
    lv = live(mix)
    w = np.where(lv, mix[:, 0].astype(np.float64), 0.0)
    b = np.zeros((SLOTS, DIM))
    Lm = np.zeros((SLOTS, DIM, DIM))
    for m in np.flatnonzero(lv):
        b[m] = mix[m, OFF_B:OFF_L].astype(np.float64)
        Lm[m] = fr.lower(mix[m, OFF_L:].reshape(DIM, DIM))
    return w, b, Lm


def log_density(r, mix):
    """r [P, 24] -> dict(l [P], lm [P, 8] (-inf for dead slots), gamma [P, 8],
    hard [P]): the definition, in float64."""
    w, b, Lm = unpack(mix)
    lv = live(mix)
    sumw = 0.0
    for m in range(SLOTS):
        sumw += w[m]
    P = r.shape[0]
    lm = np.full((P, SLOTS), -np.inf)
    for m in np.flatnonzero(lv):
        z = np.linalg.solve(Lm[m], (r - b[m]).T).T if P else np.zeros((0, DIM))
        q = (z * z).sum(axis=1)
        lm[:, m] = math.log(w[m] / sumw) - 12.0 * LOG_2PI - np.log(np.diag(Lm[m])).sum() - 0.5 * q
    lmax = lm.max(axis=1) if P else np.zeros(0)
    l = lmax + np.log(np.exp(lm - lmax[:, None]).sum(axis=1))
    gamma = np.exp(lm - l[:, None])
    return dict(l=l, lm=lm, gamma=gamma, hard=gamma.argmax(axis=1) if P else np.zeros(0, np.int64))


def em_step(r, mix):
    """One EM step over the residuals r [P, 24] -> dict(moments [8, 25, 24],
    resp [8, 2], total [4], mix_out [8, 608] float32, C (per slot: the ridged
    covariance the new factor factors, or None), gamma, hard, l)."""
    mix = np.asarray(mix, np.float32)
    lv = live(mix)
    w, b, Lm = unpack(mix)
    P = r.shape[0]
    d = log_density(r, mix)
    g = d["gamma"]
    moments = np.zeros((SLOTS, DIM + 1, DIM))
    resp = np.zeros((SLOTS, 2))
    out = np.zeros((SLOTS, PITCH), np.float32)
    C = [None] * SLOTS
    for m in np.flatnonzero(lv):
        moments[m, :DIM] = (r * g[:, m, None]).T @ r
        moments[m, DIM] = g[:, m] @ r
        N = g[:, m].sum()
        resp[m] = N, (d["hard"] == m).sum()
        if P == 0:
            out[m, 0] = mix[m, 0]
        else:
            out[m, 0] = np.float32(N / P)
        if P == 0 or N < 1.0:
            out[m, OFF_B:OFF_L] = mix[m, OFF_B:OFF_L]
            out[m, OFF_L:] = Lm[m].astype(np.float32).reshape(-1)
            continue
        bn = moments[m, DIM] / N
        Cm = moments[m, :DIM] / N - np.outer(bn, bn)
        i = np.arange(DIM)
        Cm[i, i] = Cm[i, i] * (1 + fr.RIDGE_REL) + fr.RIDGE_ABS
        C[m] = Cm
        out[m, OFF_B:OFF_L] = bn.astype(np.float32)
        out[m, OFF_L:] = np.linalg.cholesky(Cm).astype(np.float32).reshape(-1)
    total = np.array([P, d["l"].sum(), 0.0, 0.0])
    return dict(moments=moments, resp=resp, total=total, mix_out=out, C=C, gamma=g, hard=d["hard"],
                l=d["l"])


def em_ref(pred, targets, n_active, mix, n_frames=None, ped_mask=None):
    """g2k_mix_em_f32 on the launch's inputs."""
    return em_step(fr.residuals(pred, targets, n_active, n_frames, ped_mask), mix)


def norm_ppf(p):
    """The standard-normal quantile by bisection on erfc (float64)."""
    lo, hi = -40.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if 0.5 * math.erfc(-mid / math.sqrt(2.0)) < p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def init_from(C, fit_chol, M):
    """The deterministic start: C [24, 24] the uncentred second moments,
    fit_chol their (ridged) factor as float32 -> block [8, 608]."""
    C = np.asarray(C, np.float64)
    lam, vec = np.linalg.eigh(0.5 * (C + C.T))
    v = vec[:, -1]
    if v[np.argmax(np.abs(v))] < 0:
        v = -v
    s = math.sqrt(max(lam[-1], 0.0))
    means = [(norm_ppf((m + 0.5) / M) * s * v) for m in range(M)]
    chol = np.tril(np.asarray(fit_chol, np.float32))
    return block([np.float32(1.0 / M)] * M, means, [chol] * M)


# ---------------------------------------------------------------------------
# the selector and the draw
# ---------------------------------------------------------------------------
def selector_u(shape, seed):
    """u [S, F, N] float32 for pred of ``shape`` [S, F, 24, N]: drawn once per
    trajectory from step 0's key, hashed twice."""
    S, F, _, N = shape
    sf = np.arange(S * F, dtype=np.uint64)[:, None]
    e0 = (sf * np.uint64(L) * np.uint64(N) + np.arange(N, dtype=np.uint64)[None]).reshape(-1)
    seed = int(seed) & MASK64
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    key0 = ref._pcg(lo ^ ref._pcg(hi ^ (e0 >> np.uint64(32)))) ^ (e0 & np.uint64(0xFFFFFFFF))
    h = ref._pcg((ref._pcg(key0) + np.uint64(SEL_SALT)) & np.uint64(0xFFFFFFFF))
    u = ((h >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    assert u.dtype == np.float32
    return u.reshape(S, F, N)


def cum_weights(mix):
    """cw [8] float32: the f32 of the float64 running sum of w / sum w, the
    last live slot's forced to 1."""
    mix = np.asarray(mix, np.float32)
    lv = live(mix)
    w = np.where(lv, mix[:, 0].astype(np.float64), 0.0)
    sumw = 0.0
    for m in range(SLOTS):
        sumw += w[m]
    cw = np.zeros(SLOTS, np.float32)
    c = 0.0
    for m in range(SLOTS):
        c += w[m] / sumw
        cw[m] = np.float32(c)
    cw[np.flatnonzero(lv)[-1]] = np.float32(1.0)
    return cw


def components(shape, mix, seed):
    """comp [S, F, N]: the first live m with u < cw[m] (the last live slot
    when there is none)."""
    u = selector_u(shape, seed)
    cw, lv = cum_weights(mix), live(mix)
    comp = np.full(u.shape, np.flatnonzero(lv)[-1], np.int32)
    for m in range(SLOTS - 1, -1, -1):
        if lv[m]:
            comp[u < cw[m]] = m
    return comp


def sample(pred, mix, seed):
    """g2k_mix_sample_f32 -> (out [S, F, 24, N] float64 (band layout), comp [S, F, N])."""
    mix = np.asarray(mix, np.float32)
    pred32 = np.asarray(pred, np.float32)
    comp = components(pred32.shape, mix, seed)
    z = fr.normals(pred32.shape, seed)                                   # [S, F, N, 24]
    mu = np.empty(z.shape, np.float32)                                    # time-major
    mu[..., 0::2] = np.transpose(pred32[:, :, :L], (0, 1, 3, 2))
    mu[..., 1::2] = np.transpose(pred32[:, :, L:], (0, 1, 3, 2))
    x = np.zeros(z.shape)
    for m in np.flatnonzero(live(mix)):
        sel = comp == m
        if not sel.any():
            continue
        a = (mu[sel] + mix[m, OFF_B:OFF_L][None]).astype(np.float64)      # one f32 add
        x[sel] = a + z[sel] @ fr.lower(mix[m, OFF_L:].reshape(DIM, DIM)).T
    out = np.empty(pred32.shape)
    out[:, :, :L] = np.transpose(x[..., 0::2], (0, 1, 3, 2))
    out[:, :, L:] = np.transpose(x[..., 1::2], (0, 1, 3, 2))
    return out, comp


def best_of_k_ref(pred, targets, n_active, mix, seed, K, n_frames=None, ped_mask=None):
    """-> dict(per_ped, out, pairs, ade_k, fde_k) as tests/fullcov_ref.best_of_k_ref."""
    pred = np.asarray(pred, np.float64)
    S, F, _, N = pred.shape
    m = pair_mask(S, F, N, n_active, n_frames, ped_mask)
    ade_k = np.empty((K, S, F, N))
    fde_k = np.empty((K, S, F, N))
    for k in range(K):
        ade_k[k], fde_k[k] = draw_errors(sample(pred, mix, (int(seed) + k) & MASK64)[0], targets)
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
