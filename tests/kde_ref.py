"""float64 checker of the KDE-NLL evaluation (g2k_kde_nll_f32 /
g2k_fullcov_kde_nll_f32; csrc/g2k_kde.hip states the definition).  It takes
the K draws as an array, so the same code scores the oracle's draws (on the
CPU) and the device's own (on the GPU).  ``restated=True`` repeats the
kernel's precision split instead: fp32 moments of d = x - mu, the bandwidth in
double, its three inverse entries and the constant rounded to fp32, fp32
distances and log-sum-exp.  Test helper, not a test module.

The definition is scipy.stats.gaussian_kde's (tests/test_kde_nll.py pins it):
covariance with divisor K - 1, Scott's factor K^(-1/(d + 4)), d = 2, squared,
and the normaliser 2 pi sqrt(det H)."""
import numpy as np

L = 12
LOG_2PI = float(np.log(2.0 * np.pi))
K_MIN, K_MAX = 4, 4096

# The GPU tests' gate on |kernel - float64 checker|, absolute, per clipped term
# and per pair's kde_nll: 8 x the worst |restated precision - float64| over the
# exact inputs of the GPU cases (tests/kde_cases.py) with the oracle's draws,
# both heads.  Measured worst (tests/test_kde_nll.py::test_gate_measurement
# prints it): 6.49e-5 (a term, case k4, per-step head), 4.49e-5 (a pair's
# kde_nll, the same case).  The factor 8 is for the device's expf / logf and a
# summation order that varies with KS.
MEASURED_WORST = 6.5e-5
GATE = 8 * MEASURED_WORST


def kde_logp(x, y, center=None, restated=False):
    """x [K, ..., 2] the K sampled positions, y [..., 2] -> (logp [...], ok
    [...]): the log density of y under the Gaussian KDE of the x_k with
    Scott's bandwidth; ok False where det H is not a positive finite number
    (logp is -inf there).  ``restated``: the kernel's precision split, with
    ``center`` [..., 2] the mean the moments are centred on."""
    x = np.asarray(x)
    K = x.shape[0]
    scott = float(K) ** (-1.0 / 3.0)
    with np.errstate(all="ignore"):
        if not restated:
            x = x.astype(np.float64)
            y = np.asarray(y, np.float64)
            d = x - x.mean(axis=0)
            cxx = (d[..., 0] ** 2).sum(axis=0) / (K - 1)
            cyy = (d[..., 1] ** 2).sum(axis=0) / (K - 1)
            cxy = (d[..., 0] * d[..., 1]).sum(axis=0) / (K - 1)
        else:
            x = x.astype(np.float32)
            y = np.asarray(y, np.float32)
            d = x - np.asarray(center, np.float32)
            s = np.zeros((5,) + d.shape[1:-1], np.float32)
            for k in range(K):                          # running fp32 sums
                dx, dy = d[k, ..., 0], d[k, ..., 1]
                s[0] += dx
                s[1] += dy
                s[2] += dx * dx
                s[3] += dy * dy
                s[4] += dx * dy
            s = s.astype(np.float64)
            cxx = (s[2] - s[0] * s[0] / K) / (K - 1)
            cyy = (s[3] - s[1] * s[1] / K) / (K - 1)
            cxy = (s[4] - s[0] * s[1] / K) / (K - 1)
        hxx, hyy, hxy = scott * cxx, scott * cyy, scott * cxy
        det = hxx * hyy - hxy * hxy
        ok = (det > 0) & np.isfinite(det)
        sdet = np.where(ok, det, 1.0)
        ixx, iyy, ixy = hyy / sdet, hxx / sdet, -hxy / sdet
        cst = -np.log(float(K)) - LOG_2PI - 0.5 * np.log(sdet)
        ft = np.float32 if restated else np.float64
        ixx, iyy, ixy, cst = (v.astype(ft) for v in (ixx, iyy, ixy, cst))
        ex, ey = y[..., 0] - x[..., 0], y[..., 1] - x[..., 1]          # [K, ...]
        a = ft(-0.5) * (ixx * ex * ex + ft(2) * ixy * ex * ey + iyy * ey * ey)
        m = a.max(axis=0)
        lse = m + np.log(np.exp(a - m).sum(axis=0, dtype=ft))
        logp = np.where(ok, cst + lse, -np.inf)
    return logp.astype(np.float64), ok


def band_to_xy(a):
    """[..., S, F, 2L, N] (band layout) -> [..., S, F, N, L, 2]."""
    a = np.asarray(a)
    xy = np.stack([a[..., :L, :], a[..., L:, :]], axis=-1)             # [..., S, F, L, N, 2]
    return np.swapaxes(xy, -3, -2)


def kde_nll_ref(draws, targets, pairs, log_floor=-20.0, pred=None, restated=False):
    """draws [K, S, F, 2L, N] (band layout: what the sampler writes for seeds
    seed + k), targets [S, F or 1, N, L, 2], pairs [S, F, N] bool ->
    dict(per_ped [S, F, N, 4] = {kde_nll, kde_nll_final, clipped steps, 0}
    (zeros for non-pairs), out [S, 8], logp [S, F, N, L] (-inf where singular),
    term [S, F, N, L], clip [S, F, N, L] bool).  ``restated`` needs ``pred``."""
    draws = np.asarray(draws)
    K, S, F, _, N = draws.shape
    if not K_MIN <= K <= K_MAX:
        raise ValueError(f"K = {K}: {K_MIN}..{K_MAX}")
    x = band_to_xy(draws)                                              # [K, S, F, N, L, 2]
    y = np.broadcast_to(np.asarray(targets), (S, F, N, L, 2))
    logp, ok = kde_logp(x, y, center=band_to_xy(pred) if restated else None, restated=restated)
    with np.errstate(invalid="ignore"):
        clip = ~ok | ~(logp >= log_floor)                              # a NaN clips
    term = np.where(clip, float(log_floor), logp)
    m = np.asarray(pairs, bool)
    per = np.zeros((S, F, N, 4))
    per[..., 0] = np.where(m, -term.mean(axis=-1), 0.0)
    per[..., 1] = np.where(m, -term[..., L - 1], 0.0)
    per[..., 2] = np.where(m, clip.sum(axis=-1), 0.0)
    out = np.zeros((S, 8))
    out[:, :2] = per[..., :2].sum(axis=(1, 2))
    out[:, 2] = m.sum(axis=(1, 2))
    out[:, 3] = per[..., 2].sum(axis=(1, 2))
    out[:, 4] = K
    out[:, 5] = np.float32(log_floor)
    return dict(per_ped=per, out=out, logp=logp, term=term, clip=clip)
