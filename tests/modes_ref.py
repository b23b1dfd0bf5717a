"""float64 checker of the k-means reduction of a head's samples to M modes
(g2k_sample_modes_f32 and its full-covariance / mixture twins;
include/g2k_modes.h states the definition).  It takes the K draws as an array
[K, S, F, 24, N] (band layout), so the same code reduces the oracle's draws (on
the CPU) and the device's own (on the GPU).  Test helper, not a test module.

Columns of per_ped: cA, cF (the smallest ADE / FDE of the M centres), mA, mF
(the lowest centre attaining each), w_mA, w_mF (those centres' weights),
inertia (1/K sum_k d2(k, a(k)) of the final assignment), live (non-empty
clusters).  Columns of out: sum cA, sum cF, sum (1 - w_mA)^2, sum (1 - w_mF)^2,
the pairs with cF > miss_radius, sum inertia, sum live, the pair count.

``margin`` [S, F, N]: per pair the smallest (second - nearest) / (second +
nearest) over every (draw, iteration) assignment, the final assignment and the
A_m and F_m minima; a pair below FRAGILE is one whose result an arithmetic
difference of 1e-9 relative could change, and a value comparison leaves it
out.  An exact tie (0 / 0 included) has margin 0; M = 1 has no second: inf."""
import numpy as np

L = 12
M_MAX, K_MAX, ITERS_MAX = 32, 256, 64
COLS = ("cA", "cF", "mA", "mF", "w_mA", "w_mF", "inertia", "live")
# The GPU tests' gate, the project's metric tolerance: per pair
# |got - ref| <= TOL max(1, |ref|), and that times the pair count for a scene's
# sums.
TOL = 1e-4
FRAGILE = 1e-9
FRAGILE_SHARE = 0.01


def band_to_flat(x):
    """[..., 2L, N] (rows 0..L-1 x, L..2L-1 y) -> [..., N, 2L] with index j = 2t + c."""
    x = np.asarray(x)
    xy = np.stack([x[..., :L, :], x[..., L:, :]], axis=-1)          # [..., L, N, 2]
    xy = np.moveaxis(xy, -2, -3)                                    # [..., N, L, 2]
    return xy.reshape(xy.shape[:-2] + (2 * L,))


def flat_to_band(c):
    """[..., N, 2L] (j = 2t + c) -> [..., 2L, N] (band)."""
    c = np.asarray(c)
    xy = c.reshape(c.shape[:-1] + (L, 2))                           # [..., N, L, 2]
    return np.concatenate([np.moveaxis(xy[..., 0], -1, -2), np.moveaxis(xy[..., 1], -1, -2)], axis=-2)


def _margin2(v):
    """v [P, ..., M] -> the margin of the minimum over the last axis."""
    if v.shape[-1] < 2:
        return np.full(v.shape[:-1], np.inf)
    two = np.partition(v, 1, axis=-1)[..., :2]
    lo, hi = two[..., 0], two[..., 1]
    den = hi + lo
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, (hi - lo) / np.where(den > 0, den, 1.0), 0.0)


def _assign(x, c):
    """x [P, K, 24], c [P, M, 24] -> (a [P, K], d2 of the own centre [P, K],
    margin [P]); d2 summed with j ascending, the lowest m of the minimum."""
    P, K, _ = x.shape
    d2 = np.zeros((P, K, c.shape[1]))
    for j in range(2 * L):
        e = x[:, :, None, j] - c[:, None, :, j]
        d2 += e * e
    a = d2.argmin(axis=-1)                                          # the first (lowest) minimum
    mg = _margin2(d2).min(axis=-1) if P else np.zeros(0)
    return a, np.take_along_axis(d2, a[..., None], axis=-1)[..., 0], mg


def lloyd(x, M, iters):
    """x [P, K, 24] float64 -> dict(c [P, M, 24], a [P, K], n [P, M], d2 [P, K],
    margin [P], trace [iters + 1, P]: the inertia of every assignment)."""
    P, K, _ = x.shape
    c = x[:, :M].copy()
    margin = np.full(P, np.inf)
    trace = np.zeros((iters + 1, P))
    rows = np.arange(P)
    for it in range(iters + 1):
        a, d2, mg = _assign(x, c)
        margin = np.minimum(margin, mg)
        trace[it] = d2.sum(axis=1) / K
        if it == iters:
            break
        sums = np.zeros_like(c)
        n = np.zeros((P, M), np.int64)
        for k in range(K):                                          # k ascending
            sums[rows, a[:, k]] += x[:, k]
            n[rows, a[:, k]] += 1
        c = np.where(n[..., None] > 0, sums / np.maximum(n, 1)[..., None], c)
    n = np.zeros((P, M), np.int64)
    for k in range(K):
        n[rows, a[:, k]] += 1
    return dict(c=c, a=a, n=n, d2=d2, margin=margin, trace=trace)


def sample_modes_ref(draws, targets, pairs, M, iters, miss_radius=0.0):
    """draws [K, S, F, 2L, N], targets [S, F or 1, N, L, 2], pairs [S, F, N]
    bool -> dict(per_ped [S, F, N, 8], centres [S, F, M, 2L, N], weights [S, F,
    M, N], out [S, 8], margin [S, F, N] (inf for non-pairs), trace [iters + 1,
    S, F, N], pairs).  Non-pairs are zeros (their draws may be NaN: never
    looked at)."""
    pairs = np.asarray(pairs, bool)
    draws = np.asarray(draws)
    K, S, F, _, N = draws.shape
    assert 1 <= M <= M_MAX and M <= K <= K_MAX and 0 <= iters <= ITERS_MAX
    x_all = np.moveaxis(band_to_flat(draws), 0, -2)                 # [S, F, N, K, 24]
    x = x_all[pairs].astype(np.float64)                             # [P, K, 24]
    y = np.broadcast_to(np.asarray(targets).astype(np.float64), (S, F, N, L, 2))[pairs]   # [P, L, 2]
    r = lloyd(x, M, iters)
    c, n = r["c"], r["n"]
    P = x.shape[0]
    d = np.sqrt(((c.reshape(P, M, L, 2) - y[:, None]) ** 2).sum(axis=-1))         # [P, M, L]
    A = d.sum(axis=-1) / 12.0
    Fm = d[..., L - 1]
    mA, mF = A.argmin(axis=-1), Fm.argmin(axis=-1)
    rows = np.arange(P)
    w = n / float(K)
    per = np.zeros((P, 8))
    if P:
        per[:, 0], per[:, 1] = A[rows, mA], Fm[rows, mF]
        per[:, 2], per[:, 3] = mA, mF
        per[:, 4], per[:, 5] = w[rows, mA], w[rows, mF]
        per[:, 6] = r["d2"].sum(axis=1) / K
        per[:, 7] = (n > 0).sum(axis=-1)
    margin = np.minimum(r["margin"], np.minimum(_margin2(A), _margin2(Fm))) if P else np.zeros(0)
    per_ped = np.zeros((S, F, N, 8))
    per_ped[pairs] = per
    cen = np.zeros((S, F, N, M, 2 * L))
    cen[pairs] = c
    centres = flat_to_band(np.moveaxis(cen, 3, 2))                  # [S, F, M, N, 24] -> [S, F, M, 24, N]
    wt = np.zeros((S, F, N, M))
    wt[pairs] = w
    mg = np.full((S, F, N), np.inf)
    mg[pairs] = margin
    trace = np.zeros((iters + 1, S, F, N))
    trace[:, pairs] = r["trace"]
    rad = float(np.float32(miss_radius))
    out = np.zeros((S, 8))
    cols = np.stack([per_ped[..., 0], per_ped[..., 1], (1.0 - per_ped[..., 4]) ** 2,
                     (1.0 - per_ped[..., 5]) ** 2, (per_ped[..., 1] > rad).astype(np.float64),
                     per_ped[..., 6], per_ped[..., 7], np.ones((S, F, N))], axis=-1)
    out[:] = (cols * pairs[..., None]).sum(axis=(1, 2))
    return dict(per_ped=per_ped, centres=centres, weights=np.moveaxis(wt, 3, 2), out=out, margin=mg,
                trace=trace, pairs=pairs)


FIGURES = ("min_ade", "min_fde", "brier_ade", "brier_fde", "miss_rate", "inertia", "live")


def figures(out):
    """The host's figures from out [S, 8]: means over the pairs."""
    t = np.asarray(out, np.float64).reshape(-1, 8).sum(axis=0)
    n = t[7]
    if not n > 0:
        return {k: float("nan") for k in FIGURES}
    return dict(min_ade=t[0] / n, min_fde=t[1] / n, brier_ade=(t[0] + t[2]) / n,
                brier_fde=(t[1] + t[3]) / n, miss_rate=t[4] / n, inertia=t[5] / n, live=t[6] / n)
