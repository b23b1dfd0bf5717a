"""Checker of the kinematic scores (g2k_sample_kin_f32 and its full-covariance /
mixture twins; include/g2k_kin.h states the definition).  It takes the K draws
as an array [K, S, F, 24, N] (band layout), so the same code scores the
oracle's draws (on the CPU) and the device's own (on the GPU).  Test helper,
not a test module.

The FEATURES are restated in np.float32, one IEEE operation after the other in
exactly the header's order, so they are the kernel's bit for bit and the ranks
(comparisons of fp32 values) are compared for EQUALITY, with no interval.  The
sums m, p, d, y over the features are taken in float64; the kernel's fp32 sums
are held to scores_ref.TOL."""
import numpy as np

L = 12
K_MIN, K_MAX, B_MAX, ROWS, COLS = 2, 255, 64, 32, 48
NS, NA = L - 1, L - 2
GROUPS = {"speed": slice(0, NS), "acc": slice(NS, NS + NA), "lacc": slice(NS + NA, NS + 2 * NA),
          "straight": slice(ROWS - 1, ROWS)}
NG = np.array([NS, NA, NA, 1], np.float64)
ROW_GROUP = np.array([0] * NS + [1] * NA + [2] * NA + [3])


def band_to_xy(x):
    """[..., 2L, N] (rows 0..L-1 x, L..2L-1 y) -> [..., N, L, 2]."""
    x = np.asarray(x)
    xy = np.stack([x[..., :L, :], x[..., L:, :]], axis=-1)          # [..., L, N, 2]
    return np.moveaxis(xy, -3, -2)


def _norm(dx, dy):
    """sqrt(dx dx + dy dy): two products, one add, one square root, each rounded to fp32."""
    xx = dx * dx
    yy = dy * dy
    return np.sqrt(xx + yy)


def features(z):
    """z [..., L, 2] -> the 32 features [..., 32], float32 throughout."""
    z = np.asarray(z)
    assert z.dtype == np.float32 and z.shape[-2:] == (L, 2)
    v = z[..., 1:, :] - z[..., :-1, :]                               # [..., 11, 2]
    s = _norm(v[..., 0], v[..., 1])
    w = v[..., 1:, :] - v[..., :-1, :]
    a = _norm(w[..., 0], w[..., 1])
    lacc = s[..., 1:] - s[..., :-1]
    length = s[..., 0]
    for t in range(1, NS):
        length = length + s[..., t]
    e = z[..., L - 1, :] - z[..., 0, :]
    net = _norm(e[..., 0], e[..., 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        st = np.where(length == 0, np.float32(1), net / length)
    out = np.concatenate([s, a, lacc, st[..., None]], axis=-1)
    assert out.dtype == np.float32 and out.shape[-1] == ROWS
    return out


def features_loops(z):
    """z [L, 2] float32 -> the 32 features by plain loops over np.float32 scalars."""
    f = np.float32
    z = [[f(z[t][0]), f(z[t][1])] for t in range(L)]
    v = [(f(z[t + 1][0] - z[t][0]), f(z[t + 1][1] - z[t][1])) for t in range(L - 1)]

    def norm(dx, dy):
        xx, yy = f(dx * dx), f(dy * dy)
        return f(np.sqrt(f(xx + yy)))
    s = [norm(*v[t]) for t in range(NS)]
    a = [norm(f(v[t + 1][0] - v[t][0]), f(v[t + 1][1] - v[t][1])) for t in range(NA)]
    lacc = [f(s[t + 1] - s[t]) for t in range(NA)]
    length = s[0]
    for t in range(1, NS):
        length = f(length + s[t])
    net = norm(f(z[L - 1][0] - z[0][0]), f(z[L - 1][1] - z[0][1]))
    st = f(1) if length == 0 else f(net / length)
    return s + a + lacc + [st]


def pair_loops(x, y):
    """x [K, L, 2], y [L, 2] float32 -> the pair's 48 columns by plain loops
    (float64 sums of the float32 features)."""
    K = len(x)
    fx = [features_loops(x[k]) for k in range(K)]
    fy = features_loops(y)
    r = [sum(1 for k in range(K) if fx[k][j] < fy[j]) for j in range(ROWS)]
    m, p, d, yg = [], [], [], []
    for name, sl in GROUPS.items():
        rows = range(sl.start, sl.stop)
        n = len(rows)
        m.append(sum(abs(float(fx[k][j]) - float(fy[j])) for k in range(K) for j in rows) / (K * n))
        p.append(2.0 * sum(abs(float(fx[k][j]) - float(fx[q][j])) for k in range(K) for q in range(k + 1, K)
                           for j in rows) / (K * (K - 1) * n))
        d.append(sum(float(fx[k][j]) for k in range(K) for j in rows) / (K * n))
        yg.append(sum(float(fy[j]) for j in rows) / n)
    return [float(v) for v in r] + m + p + d + yg


def _group_sums(v):
    """[..., 32] -> [..., 4] float64: the sums over each group's rows."""
    return np.stack([v[..., sl].sum(axis=-1) for sl in GROUPS.values()], axis=-1)


def sample_kin_ref(draws, targets, pairs):
    """draws [K, S, F, 24, N], targets [S, F or 1, N, L, 2] (float32), pairs [S,
    F, N] bool -> dict(per [S, F, N, 48] float64 (the header's per_ped), sums
    [S, 16] float64, fx [K, P, 32] and fy [P, 32] float32 of the P pairs)."""
    pairs = np.asarray(pairs, bool)
    draws = np.asarray(draws)
    assert draws.dtype == np.float32
    x = band_to_xy(draws)                                            # [K, S, F, N, L, 2]
    K, S, F, N = x.shape[:4]
    assert K_MIN <= K <= K_MAX
    y = np.broadcast_to(np.asarray(targets, np.float32), (S, F, N, L, 2))
    fx = features(np.ascontiguousarray(x[:, pairs]))                 # [K, P, 32]
    fy = features(np.ascontiguousarray(y[pairs]))                    # [P, 32]
    r = (fx < fy[None]).sum(axis=0)                                  # [P, 32]
    x64, y64 = fx.astype(np.float64), fy.astype(np.float64)
    m = _group_sums(np.abs(x64 - y64[None]).sum(axis=0)) / (K * NG)
    pp = np.zeros_like(y64)
    for k in range(K - 1):
        pp += np.abs(x64[k + 1:] - x64[k][None]).sum(axis=0)
    p = _group_sums(pp) * 2.0 / (K * (K - 1) * NG)
    d = _group_sums(x64.sum(axis=0)) / (K * NG)
    yg = _group_sums(y64) / NG
    per = np.zeros((S, F, N, COLS), np.float64)
    per[pairs] = np.concatenate([r.astype(np.float64), m, p, d, yg], axis=-1)
    return dict(per=per, sums=per[..., ROWS:].sum(axis=(1, 2)), fx=fx, fy=fy, pairs=pairs)


def hist_tot(per, pairs, k, bins):
    """hist [S, 32, B], tot [S, 8] as the sums of per_ped [S, F, N, 48]."""
    per = np.asarray(per)
    S = per.shape[0]
    r = np.rint(per[..., :ROWS]).astype(np.int64)
    hist = np.zeros((S, ROWS, bins), np.int64)
    tot = np.zeros((S, 8), np.int64)
    for s in range(S):
        rs = r[s][pairs[s]]                                          # [P, 32]
        for i in range(ROWS):
            hist[s, i] = np.bincount(rs[:, i] * bins // (k + 1), minlength=bins)
        tot[s, 0] = len(rs)
        for gi, sl in enumerate(GROUPS.values()):
            tot[s, 1 + gi] = int(rs[:, sl].sum())
    return hist, tot


def figures(sums, hist, tot, k):
    """The result class's figures from the counts, float64: dict group ->
    dict(crps, pit_mean, dev, draw_mean, target_mean)."""
    sums = np.asarray(sums, np.float64).sum(axis=0)
    h = np.asarray(hist, np.float64).sum(axis=0)
    t = np.asarray(tot, np.int64).sum(axis=0)
    n = float(t[0])
    out = {}
    for gi, (name, sl) in enumerate(GROUPS.items()):
        c = h[sl].sum(axis=0)
        rows = sl.stop - sl.start
        out[name] = dict(crps=(sums[gi] - 0.5 * sums[4 + gi]) / n, draw_mean=sums[8 + gi] / n,
                         target_mean=sums[12 + gi] / n,
                         pit_mean=(t[1 + gi] + 0.5 * rows * n) / ((k + 1) * rows * n),
                         dev=0.5 * np.abs(c / c.sum() - 1.0 / c.size).sum())
    return out
