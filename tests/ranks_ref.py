"""float64 checker of the rank-histogram calibration (g2k_sample_ranks_f32 and
its full-covariance / mixture twins; include/g2k_ranks.h states the
definition).  It takes the K draws as an array [K, S, F, 24, N] (band layout),
so the same code ranks the oracle's draws (on the CPU) and the device's own (on
the GPU).  Test helper, not a test module.

The kernel compares fp32 sums, so a rank is checked against an INTERVAL: with
rho the float64 pre-ranks,
  density rank     r_lo = #{k : rho(X_k) >  rho(Y) (1 + M) + A}
                   r_hi = #{k : rho(X_k) >= rho(Y) (1 - M) - A}
  trajectory rank  r_lo = #{k : rho(X_k) <  rho(Y) (1 - M) - A}
                   r_hi = #{k : rho(X_k) <= rho(Y) (1 + M) + A}
and the device's rank must lie in [r_lo, r_hi].  ``r`` is the float64 rank
itself (M = A = 0).  A step is degenerate when det H is not a positive finite
number; where |det H| <= M hxx hyy the fp32 moments may decide either way
(``deg_open``).

The margins.  A = 1e-30 covers the fp32 underflow of exp.  M is four times the
worst relative deviation of rho between ``restated=True`` — the same definition
with the kernel's precisions (the moments of fp32 differences centred as the
head's kernel centres them, summed in double; the bandwidth and the inverse of
its Cholesky factor in double, the scaled inverse rounded to fp32; fp32
quadratic forms as a sum of two squares, exp2 and running sums in k order) —
and float64,
over every case of tests/ranks_cases.py and the three heads on the oracle's
draws; the factor four is for the kernel's different summation order (a lane
starts at its own draw) and its 1-ulp exp2 and square root.  Measured by

  python -m tests.ranks_ref

which prints the deviation per case and head; the worst, 5.67e-6 (case k65,
mixture head), is MEASURED below, rounded up.  The deviation of a sum s32 from
s64 is taken as max(|s32 - s64| - A, 0) / s64.  (With the moments summed in
fp32 and the quadratic form written a ex^2 + b ex ey + c ey^2 the same
measurement gave 1.3e-4 — case n256, seven pooled points nearly collinear at one
step, det H = 0.01 hxx hyy, where the inverse magnifies the moments' rounding —
and with that M a quarter of the K = 255 intervals were wide: the kernel sums
the moments in double and takes the form as two squares for that reason.)"""
import numpy as np

L = 12
K_MIN, K_MAX, B_MAX, ROWS = 4, 255, 64, 13
A = 1e-30
MEASURED = 5.7e-6
M = 4 * MEASURED
WIDE_CAP = 0.05                 # the share of (pair, row) with r_hi > r_lo that a case may have
_S = -0.72134752044448170368    # -1/2 log2 e


def band_to_xy(x):
    """[..., 2L, N] (rows 0..L-1 x, L..2L-1 y) -> [..., N, L, 2]."""
    x = np.asarray(x)
    xy = np.stack([x[..., :L, :], x[..., L:, :]], axis=-1)          # [..., L, N, 2]
    return np.moveaxis(xy, -3, -2)


def _pooled(draws, targets, pairs):
    """-> z [K + 1, P, L, 2] float64 of the P pairs, the target LAST (the
    kernel's order: the K slots, then the target)."""
    pairs = np.asarray(pairs, bool)
    x = band_to_xy(np.asarray(draws))                                # [K, S, F, N, L, 2]
    K, S, F, N = x.shape[:4]
    assert K_MIN <= K <= K_MAX
    y = np.broadcast_to(np.asarray(targets), (S, F, N, L, 2))
    return np.concatenate([x[:, pairs], y[pairs][None]]).astype(np.float64)


def _rho64(z):
    """z [K + 1, P, L, 2] -> rho [K + 1, P, 13], det, hxx hyy [P, L] in float64."""
    n = z.shape[0]
    K = n - 1
    d = z - z.mean(axis=0)
    c = np.einsum("kpti,kptj->ptij", d, d) / K
    H = (K + 1) ** (-1.0 / 3.0) * c
    hxx, hyy, hxy = H[..., 0, 0], H[..., 1, 1], H[..., 0, 1]
    det = hxx * hyy - hxy * hxy
    ok = (det > 0) & np.isfinite(det)
    sdet = np.where(ok, det, 1.0)
    ixx, iyy, ixy = hyy / sdet, hxx / sdet, -hxy / sdet
    rho = np.zeros((n, z.shape[1], ROWS))
    for i in range(n):
        e = z[i][None] - z                                           # [K + 1, P, L, 2]
        q = ixx * e[..., 0] ** 2 + 2 * ixy * e[..., 0] * e[..., 1] + iyy * e[..., 1] ** 2
        t = np.exp(-0.5 * q)
        t[i] = 0.0
        rho[i, :, :L] = t.sum(axis=0)
        rho[i, :, L] = np.sqrt((e ** 2).sum(axis=(-1, -2))).sum(axis=0)
    return rho, det, hxx * hyy


def _rho32(z, mu, running_mean):
    """The same with the kernel's precisions; z float64 holding fp32 values,
    mu [P, L, 2] the means the plain sums are centred on."""
    f = np.float32
    n = z.shape[0]
    K = n - 1
    z = z.astype(f)
    if running_mean:
        m = np.zeros(z.shape[1:])
        cxx, cyy, cxy = (np.zeros(z.shape[1:3]) for _ in range(3))
        for k in range(n):
            u = z[k] - m
            m = m + u / (k + 1)
            v = z[k] - m
            cxx, cyy, cxy = cxx + u[..., 0] * v[..., 0], cyy + u[..., 1] * v[..., 1], cxy + u[..., 0] * v[..., 1]
    else:
        d = (z - mu.astype(f)).astype(f).astype(np.float64)          # fp32 differences, double sums
        sd = d.sum(axis=0)
        cxx = (d[..., 0] ** 2).sum(axis=0) - sd[..., 0] ** 2 / (K + 1)
        cyy = (d[..., 1] ** 2).sum(axis=0) - sd[..., 1] ** 2 / (K + 1)
        cxy = (d[..., 0] * d[..., 1]).sum(axis=0) - sd[..., 0] * sd[..., 1] / (K + 1)
    w = (K + 1) ** (-1.0 / 3.0) / K
    hxx, hyy, hxy = cxx * w, cyy * w, cxy * w
    det = hxx * hyy - hxy * hxy
    ok = (det > 0) & np.isfinite(det)
    l11 = np.sqrt(np.where(ok, hxx, 1.0))
    l21, l22 = hxy / l11, np.sqrt(np.where(ok, det, 1.0)) / l11
    sc = np.sqrt(-_S)
    a, b, c = (sc / l11).astype(f), (-sc * l21 / (l11 * l22)).astype(f), (sc / l22).astype(f)
    rho = np.zeros((n, z.shape[1], ROWS), f)
    for i in range(n):
        for j in list(range(i + 1, n)) + list(range(i)):             # the others, circularly
            e = (z[i] - z[j]).astype(f)
            u, v = (a * e[..., 0]).astype(f), (b * e[..., 0] + (c * e[..., 1]).astype(f)).astype(f)
            rho[i, :, :L] += np.exp2(-(u * u + (v * v).astype(f)).astype(f)).astype(f)
            rho[i, :, L] += np.sqrt((e * e).astype(f).sum(axis=(-1, -2), dtype=f))
    return rho.astype(np.float64), ~ok


def sample_ranks_ref(draws, targets, pairs, m=M, a=A):
    """draws [K, S, F, 2L, N], targets [S, F or 1, N, L, 2], pairs [S, F, N]
    bool -> dict(r, r_lo, r_hi [S, F, N, 13] int (zeros for non-pairs; the
    rows of degenerate steps hold -1), deg, deg_open [S, F, N, 12] bool, rho [K
    + 1, P, 13] (the target last), pairs).  Non-pairs' draws may be NaN: never
    looked at."""
    pairs = np.asarray(pairs, bool)
    z = _pooled(draws, targets, pairs)
    K = z.shape[0] - 1
    with np.errstate(invalid="ignore", over="ignore"):
        rho, det, scale = _rho64(z)
    deg = ~((det > 0) & np.isfinite(det))
    open_ = np.abs(det) <= m * scale
    rx, ry = rho[:K], rho[K]
    r = (rx > ry).sum(axis=0)
    lo = (rx > ry * (1 + m) + a).sum(axis=0)
    hi = (rx >= ry * (1 - m) - a).sum(axis=0)
    r[:, L] = (rx < ry)[..., L].sum(axis=0)
    lo[:, L] = (rx < ry * (1 - m) - a)[..., L].sum(axis=0)
    hi[:, L] = (rx <= ry * (1 + m) + a)[..., L].sum(axis=0)
    for v in (r, lo, hi):
        v[:, :L][deg] = -1
    out = {}
    for name, v, dt in (("r", r, np.int64), ("r_lo", lo, np.int64), ("r_hi", hi, np.int64)):
        full = np.zeros(pairs.shape + (ROWS,), dt)
        full[pairs] = v
        out[name] = full
    for name, v in (("deg", deg), ("deg_open", open_)):
        full = np.zeros(pairs.shape + (L,), bool)
        full[pairs] = v
        out[name] = full
    out.update(rho=rho, pairs=pairs, k=K)
    return out


def deviation(draws, targets, pairs, pred, running_mean, a=A):
    """The worst relative deviation of the restated fp32 sums from float64 over
    the pairs' K + 1 points and 13 rows (rows of degenerate steps left out)."""
    pairs = np.asarray(pairs, bool)
    z = _pooled(draws, targets, pairs)
    if z.shape[1] == 0:
        return 0.0
    S, F, N = pairs.shape
    mu = band_to_xy(np.asarray(pred))[pairs].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        r64, det, _ = _rho64(z)
        r32, deg32 = _rho32(z, mu, running_mean)
    keep = np.ones(r64.shape[1:], bool)
    keep[:, :L] = (det > 0) & np.isfinite(det) & ~deg32
    dev = np.maximum(np.abs(r32 - r64) - a, 0.0) / r64
    return float(dev[:, keep].max())


def hist_tot(per, pairs, k, bins):
    """hist [S, 13, B], tot [S, 4] as the sums of per_ped [S, F, N, 16]."""
    per = np.asarray(per)
    S = per.shape[0]
    r = np.rint(per[..., :ROWS]).astype(np.int64)
    hist = np.zeros((S, ROWS, bins), np.int64)
    tot = np.zeros((S, 4), np.int64)
    for s in range(S):
        rs = r[s][pairs[s]]                                          # [P, 13]
        for i in range(ROWS):
            v = rs[:, i][rs[:, i] >= 0]
            hist[s, i] = np.bincount(v * bins // (k + 1), minlength=bins)
        tot[s] = (len(rs), int((rs[:, :L] < 0).sum()), int(np.where(rs[:, :L] >= 0, rs[:, :L], 0).sum()),
                  int(rs[:, L].sum()))
    return hist, tot


def shares(hist):
    n = hist.sum(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, hist / n, np.nan)


def chi2(counts):
    """Pearson's statistic of counts [B] against uniform."""
    c = np.asarray(counts, np.float64)
    e = c.sum() / c.size
    return float(((c - e) ** 2 / e).sum())


def chi2_quantile(p, df):
    """scipy's when importable, else the Wilson-Hilferty approximation df (1 -
    2 / (9 df) + z_p sqrt(2 / (9 df)))^3."""
    try:
        from scipy import stats
        return float(stats.chi2.ppf(p, df))
    except ImportError:
        from statistics import NormalDist
        zp = NormalDist().inv_cdf(p)
        return df * (1 - 2 / (9 * df) + zp * (2 / (9 * df)) ** 0.5) ** 3


if __name__ == "__main__":
    from tests import ranks_cases as rc
    worst = 0.0
    for i, name in enumerate(rc.IDS):
        c = rc.inputs(i)
        for which in rc.HEADS:
            dv = deviation(rc.oracle_draws(i, which), c["targets"], c["pairs"], c["pred"], which == "mix")
            R = sample_ranks_ref(rc.oracle_draws(i, which), c["targets"], c["pairs"])
            wide = (R["r_hi"] > R["r_lo"])[c["pairs"]].mean() if c["pairs"].any() else 0.0
            print(f"{name:8s} {which:9s} deviation {dv:.3g}  wide intervals {wide:.4f}")
            worst = max(worst, dv)
    print(f"worst deviation {worst:.3g}: MEASURED = {MEASURED}, M = {M}")
