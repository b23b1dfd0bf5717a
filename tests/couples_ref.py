"""The checker of the couple-distance scores (include/g2k_couples.h): the
features restated in np.float32 operation for operation (two differences, two
products, one add per step, none fused; the minimum; one correctly rounded
square root), the ranks as comparisons of the float32 SQUARED values, the float
sums m, p, d, y in float64 over the float32 roots.  ``couple_scores_ref`` takes
[K, S, F, 24, N] draws (the device's own, or the restated samplers').  Test
helper, not a test module."""
import numpy as np

L = 12
K_MIN, K_MAX, B_MAX = 2, 64, 64
FEATURES = ("min", "fin")


def band_to_xy(x):
    """[..., 2L, N] (rows 0..L-1 x, L..2L-1 y) -> [..., N, L, 2]."""
    x = np.asarray(x)
    xy = np.stack([x[..., :L, :], x[..., L:, :]], axis=-1)          # [..., L, N, 2]
    return np.moveaxis(xy, -3, -2)


def features(za, zb):
    """za, zb [..., L, 2] float32 -> (qmin, qfin) float32: every operation one
    float32 operation, in the header's order."""
    za, zb = np.asarray(za, np.float32), np.asarray(zb, np.float32)
    dx = za[..., 0] - zb[..., 0]
    dy = za[..., 1] - zb[..., 1]
    xx = dx * dx
    yy = dy * dy
    q = xx + yy
    assert q.dtype == np.float32
    return q.min(axis=-1), q[..., L - 1]


def features_loops(za, zb):
    """One couple, step by step: [qmin, qfin] as Python floats of float32 values."""
    qmin, q = np.float32(np.inf), np.float32(0)
    for t in range(L):
        dx = np.float32(za[t][0]) - np.float32(zb[t][0])
        dy = np.float32(za[t][1]) - np.float32(zb[t][1])
        q = np.float32(np.float32(dx * dx) + np.float32(dy * dy))
        qmin = q if q < qmin else qmin
    return [float(qmin), float(q)]


def couple_loops(xa, xb, ya, yb):
    """One scored couple by plain loops: xa, xb [K, L, 2] the two members'
    draws, ya, yb [L, 2] their targets -> [r_min, r_fin, m_min, m_fin, p_min,
    p_fin, d_min, d_fin, y_min, y_fin]."""
    K = len(xa)
    qy = features_loops(ya, yb)
    qx = [features_loops(xa[k], xb[k]) for k in range(K)]
    out = []
    rs, ms, ps, ds, ys = [], [], [], [], []
    for g in range(2):
        sy = float(np.sqrt(np.float32(qy[g])))
        sx = [float(np.sqrt(np.float32(qx[k][g]))) for k in range(K)]
        rs.append(sum(1 for k in range(K) if qx[k][g] < qy[g]))
        ms.append(sum(abs(v - sy) for v in sx) / K)
        ps.append(2.0 * sum(abs(sx[k] - sx[l]) for k in range(K) for l in range(k + 1, K)) / (K * (K - 1)))
        ds.append(sum(sx) / K)
        ys.append(sy)
    out = rs + ms + ps + ds + ys
    return out


def scored_mask(qmin_mean, reach):
    """qmin(M) < reach * reach, one float32 product; +inf: every couple."""
    reach = np.float32(reach)
    if np.isinf(reach):
        return np.ones(np.shape(qmin_mean), bool)
    return np.asarray(qmin_mean, np.float32) < reach * reach


def couple_scores_ref(draws, targets, pred, members, K, B, reach=np.inf):
    """draws [K, S, F, 24, N] float32, targets [S, F or 1, N, L, 2], pred [S, F,
    24, N], members [S, F, N] bool -> dict(per_couple [S, F, N, N] int64,
    per_frame_f [S, F, 8] float64, per_frame_i [S, F, 4] int64, sums [S, 8]
    float64, hist [S, 2, B] int64, tot [S, 4] int64, n_scored, ties)."""
    draws = np.asarray(draws)
    assert draws.dtype == np.float32 and draws.shape[0] == K
    S, F, N = members.shape
    x = band_to_xy(draws)                                              # [K, S, F, N, L, 2]
    mu = band_to_xy(np.asarray(pred, np.float32))
    y = np.broadcast_to(np.asarray(targets, np.float32), (S, F, N, L, 2))
    pc = np.zeros((S, F, N, N), np.int64)
    pf = np.zeros((S, F, 8), np.float64)
    pi = np.zeros((S, F, 4), np.int64)
    hist = np.zeros((S, 2, B), np.int64)
    ties = 0
    for s in range(S):
        for f in range(F):
            idx = np.flatnonzero(members[s, f])
            P = len(idx)
            pi[s, f, 3] = P * (P - 1) // 2
            if P < 2:
                continue
            ia, ib = np.triu_indices(P, 1)
            a, b = idx[ia], idx[ib]
            qm = features(mu[s, f, a], mu[s, f, b])[0]
            sc = scored_mask(qm, reach)
            a, b = a[sc], b[sc]
            if not len(a):
                continue
            qy = np.stack(features(y[s, f, a], y[s, f, b]))              # [2, C]
            qx = np.stack(features(x[:, s, f, a], x[:, s, f, b]))        # [2, K, C]
            r = (qx < qy[:, None]).sum(axis=1)                           # [2, C]
            ties += int((qx == qy[:, None]).sum())
            sy = np.sqrt(qy).astype(np.float64)
            sx = np.sqrt(qx)
            assert sx.dtype == np.float32
            sx = sx.astype(np.float64)
            m = np.abs(sx - sy[:, None]).mean(axis=1)
            p = np.zeros_like(m)
            for k in range(K - 1):
                p += np.abs(sx[:, k:k + 1] - sx[:, k + 1:]).sum(axis=1)
            p *= 2.0 / (K * (K - 1))
            d = sx.mean(axis=1)
            pc[s, f, a, b] = 1 + r[0] + 256 * r[1]
            pf[s, f] = [m[0].sum(), m[1].sum(), p[0].sum(), p[1].sum(), d[0].sum(), d[1].sum(),
                        sy[0].sum(), sy[1].sum()]
            pi[s, f, :3] = [len(a), r[0].sum(), r[1].sum()]
            for g in range(2):
                hist[s, g] += np.bincount(r[g] * B // (K + 1), minlength=B)
    return dict(per_couple=pc, per_frame_f=pf, per_frame_i=pi, sums=pf.sum(axis=1), hist=hist,
                tot=pi.sum(axis=1), ties=ties)


def dev(counts):
    """Half the L1 distance of a histogram's shares from uniform."""
    c = np.asarray(counts, np.float64)
    n = c.sum()
    return float(0.5 * np.abs(c / n - 1.0 / len(c)).sum()) if n > 0 else float("nan")


def figures(sums, hist, tot, K):
    """feature -> dict(crps, pit_mean, dev, draw_mean, target_mean) and
    "couples", from the outputs summed over the scenes, in float64."""
    s = np.asarray(sums, np.float64).sum(axis=0)
    t = np.asarray(tot, np.int64).sum(axis=0)
    h = np.asarray(hist, np.int64).sum(axis=0)
    n = int(t[0])
    nan = float("nan")
    out = {"couples": n}
    for g, name in enumerate(FEATURES):
        out[name] = dict(crps=(s[g] - 0.5 * s[2 + g]) / n if n else nan,
                         pit_mean=(int(t[1 + g]) + 0.5 * n) / ((K + 1) * n) if n else nan,
                         dev=dev(h[g]), draw_mean=s[4 + g] / n if n else nan,
                         target_mean=s[6 + g] / n if n else nan)
    return out
