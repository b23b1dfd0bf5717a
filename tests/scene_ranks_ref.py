"""The checker of the scene-level rank calibration (include/g2k_scene_ranks.h):
the definition restated in float64 NumPy on the float32 draws.  Per scored
scene-frame (P >= 2) the K + 1 pooled items (the K joint draws, then the
targets), each P x 24 (time-major, c = 2 t + x/y), their distance matrix from
differences, the three pre-rank features, the ranks and the energy-score
terms.  Both sides are double, so the floats differ by summation order alone;
a rank is an integer that a last-bit difference of two features can move, so
the checker also gives, per rank, the interval [#{g_k < g_K (1 - mu)}, #{g_k
<= g_K (1 + mu)}] that the device's must lie in, and how many intervals hold
more than one value.  ``scene_ranks_ref`` takes [K, S, F, 24, N] draws (the
device's own, or the restated samplers').  Test helper, not a test module."""
import numpy as np

L = 12
DIM = 24
K_MIN, K_MAX, B_MAX = 2, 64, 64
FEATURES = ("typ", "loc", "spr")
MU = 1e-12


def band_to_items(x):
    """[..., 2L, N] (rows 0..L-1 x, L..2L-1 y) -> [..., N, 24] time-major."""
    x = np.asarray(x)
    xy = np.stack([x[..., :L, :], x[..., L:, :]], axis=-1)          # [..., L, N, 2]
    xy = np.moveaxis(xy, -3, -2)                                    # [..., N, L, 2]
    return xy.reshape(xy.shape[:-2] + (DIM,))


def frame_features(Z, M):
    """Z [K + 1, P, 24] float64 items (the last the targets), M [P, 24] the
    means -> dict(D [K + 1, K + 1], typ, loc, spr [K + 1], m, p)."""
    NI, P, _ = Z.shape
    K = NI - 1
    diff = Z[:, None] - Z[None]                                      # [NI, NI, P, 24]
    D = np.sqrt((diff * diff).sum(axis=(2, 3)))
    typ = D.sum(axis=1)                                              # D(j, j) = 0
    r = Z - M[None]
    s = r.sum(axis=1)                                                # [NI, 24]
    q = (r * r).sum(axis=(1, 2))
    loc = (s * s).sum(axis=1) / P
    spr = q - loc
    m = D[:K, K].sum() / K
    p = 2.0 * np.triu(D[:K, :K], 1).sum() / (K * (K - 1))
    return dict(D=D, typ=typ, loc=loc, spr=spr, m=m, p=p)


def frame_loops(Z, M):
    """``frame_features`` and the ranks by plain Python loops, in the header's
    order -> [m, p, mean loc, loc_K, mean spr, spr_K, r_typ, r_loc, r_spr]."""
    NI, P = len(Z), len(Z[0])
    K = NI - 1
    D = [[0.0] * NI for _ in range(NI)]
    for j in range(NI):
        for l in range(j + 1, NI):
            acc = 0.0
            for i in range(P):
                for c in range(DIM):
                    d = float(Z[j][i][c]) - float(Z[l][i][c])
                    acc += d * d
            D[j][l] = D[l][j] = acc ** 0.5
    typ, loc, spr = [], [], []
    for j in range(NI):
        typ.append(sum(D[j][l] for l in range(NI) if l != j))
        s, q = [0.0] * DIM, 0.0
        for i in range(P):
            for c in range(DIM):
                r = float(Z[j][i][c]) - float(M[i][c])
                s[c] += r
                q += r * r
        lo = sum(v * v for v in s) / P
        loc.append(lo)
        spr.append(q - lo)
    m = sum(D[k][K] for k in range(K)) / K
    p = 2.0 * sum(D[k][l] for l in range(1, K) for k in range(l)) / (K * (K - 1))
    ranks = [sum(1 for k in range(K) if g[k] < g[K]) for g in (typ, loc, spr)]
    return [m, p, sum(loc[:K]) / K, loc[K], sum(spr[:K]) / K, spr[K]] + ranks


def rank_interval(g, mu=MU):
    """g [K + 1] -> (r, lo, hi): the strict rank of g[K] among g[:K] and the
    interval a device rank must lie in."""
    y = g[-1]
    e = mu * abs(y)
    return int((g[:-1] < y).sum()), int((g[:-1] < y - e).sum()), int((g[:-1] <= y + e).sum())


def scene_ranks_ref(draws, targets, pred, members, K, B, mu=MU):
    """draws [K, S, F, 24, N] float32, targets [S, F or 1, N, L, 2], pred [S, F,
    24, N], members [S, F, N] bool -> dict(per_frame_i [S, F, 4] int64,
    per_frame_d [S, F, 6] float64, sums [S, 6], hist [S, 3, B] int64, tot [S,
    4] int64, lo, hi [S, F, 3] the ranks' intervals, wide: the ranks whose
    interval holds more than one value, ranks: how many there are, ties)."""
    draws = np.asarray(draws)
    assert draws.dtype == np.float32 and draws.shape[0] == K
    S, F, N = members.shape
    x = band_to_items(draws)                                           # [K, S, F, N, 24]
    mu_ = band_to_items(np.asarray(pred, np.float32))
    y = np.broadcast_to(np.asarray(targets, np.float32), (S, F, N, L, 2)).reshape(S, F, N, DIM)
    pi = np.zeros((S, F, 4), np.int64)
    pd = np.zeros((S, F, 6), np.float64)
    lo, hi = np.zeros((S, F, 3), np.int64), np.zeros((S, F, 3), np.int64)
    hist = np.zeros((S, 3, B), np.int64)
    tot = np.zeros((S, 4), np.int64)
    wide = ties = ranks = 0
    for s in range(S):
        for f in range(F):
            idx = np.flatnonzero(members[s, f])
            P = len(idx)
            if P < 2:
                continue
            Z = np.concatenate([x[:, s, f, idx], y[None, s, f, idx]]).astype(np.float64)
            ft = frame_features(Z, mu_[s, f, idx].astype(np.float64))
            pi[s, f, 0] = P
            for gi, g in enumerate(FEATURES):
                r, a, b = rank_interval(ft[g], mu)
                pi[s, f, 1 + gi], lo[s, f, gi], hi[s, f, gi] = r, a, b
                wide += b > a
                ties += int((ft[g][:-1] == ft[g][-1]).sum())
                ranks += 1
                hist[s, gi, r * B // (K + 1)] += 1
            pd[s, f] = [ft["m"], ft["p"], ft["loc"][:K].mean(), ft["loc"][K], ft["spr"][:K].mean(),
                        ft["spr"][K]]
            tot[s] += [1, pi[s, f, 1], pi[s, f, 2], pi[s, f, 3]]
    return dict(per_frame_i=pi, per_frame_d=pd, sums=pd.sum(axis=1), hist=hist, tot=tot, lo=lo, hi=hi,
                wide=int(wide), ranks=ranks, ties=ties)


def recount(per_frame_i, K, B):
    """(hist [S, 3, B], tot [S, 4]) int64 that a per_frame_i implies."""
    pi = np.asarray(per_frame_i, np.int64)
    S = pi.shape[0]
    hist = np.zeros((S, 3, B), np.int64)
    tot = np.zeros((S, 4), np.int64)
    for s in range(S):
        sc = pi[s, :, 0] > 0
        tot[s] = [sc.sum(), pi[s, sc, 1].sum(), pi[s, sc, 2].sum(), pi[s, sc, 3].sum()]
        for g in range(3):
            hist[s, g] = np.bincount(pi[s, sc, 1 + g] * B // (K + 1), minlength=B)
    return hist, tot


def dev(counts):
    """Half the L1 distance of a histogram's shares from uniform."""
    c = np.asarray(counts, np.float64)
    n = c.sum()
    return float(0.5 * np.abs(c / n - 1.0 / len(c)).sum()) if n > 0 else float("nan")


def figures(sums, hist, tot, K):
    """dict(frames, es, feature -> dict(dev, pit[, draw, target])) from the
    outputs summed over the scenes, in float64."""
    s = np.asarray(sums, np.float64).sum(axis=0)
    t = np.asarray(tot, np.int64).sum(axis=0)
    h = np.asarray(hist, np.int64).sum(axis=0)
    n = int(t[0])
    nan = float("nan")
    out = {"frames": n, "es": (s[0] - 0.5 * s[1]) / n if n else nan}
    for g, name in enumerate(FEATURES):
        out[name] = dict(dev=dev(h[g]), pit=(int(t[1 + g]) + 0.5 * n) / ((K + 1) * n) if n else nan)
        if g:
            out[name].update(draw=s[2 * g] / n if n else nan, target=s[2 * g + 1] / n if n else nan)
    return out
