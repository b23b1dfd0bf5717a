"""float64 checker of the sample scores (g2k_sample_scores_f32 and its
full-covariance / mixture twins; include/g2k_scores.h states the definition).
It takes the K draws as an array [K, S, F, 24, N] (band layout), so the same
code scores the oracle's draws (on the CPU) and the device's own (on the GPU).
Test helper, not a test module.

Columns of per_ped: mA, mF, mR (the draws against the target: mean over the 12
steps' distances, the last step's, the 24-D norm), pA, pF, pR (the same among
the K (K - 1) / 2 couples of draws), vs (the variogram score of order 1/2 over
the 66 step pairs), 0."""
import numpy as np

L = 12
K_MIN, K_MAX = 2, 256
COLS = ("mA", "mF", "mR", "pA", "pF", "pR", "vs")
# The GPU tests' gate, the project's metric tolerance: per pair
# |got - ref| <= TOL max(1, |ref|), and that times the pair count for a scene's
# sums.
TOL = 1e-4


def band_to_xy(x):
    """[..., 2L, N] (rows 0..L-1 x, L..2L-1 y) -> [..., N, L, 2]."""
    x = np.asarray(x)
    xy = np.stack([x[..., :L, :], x[..., L:, :]], axis=-1)          # [..., L, N, 2]
    return np.moveaxis(xy, -3, -2)


def _afr(d):
    """d [..., L, 2] differences of two trajectories -> (a, f, r)."""
    n = np.sqrt((d ** 2).sum(axis=-1))
    return n.mean(axis=-1), n[..., L - 1], np.sqrt((d ** 2).sum(axis=(-1, -2)))


def _vario(x):
    """x [..., L, 2] -> [..., 66]: ||x(t) - x(u)||^(1/2), t < u, t-major."""
    t, u = np.triu_indices(L, 1)
    d = x[..., t, :] - x[..., u, :]
    return ((d ** 2).sum(axis=-1)) ** 0.25


def sample_scores_ref(draws, targets, pairs, restated=False):
    """draws [K, S, F, 2L, N], targets [S, F or 1, N, L, 2], pairs [S, F, N]
    bool -> dict(per_ped [S, F, N, 8], out [S, 8], pairs).  Non-pairs are
    zeros (their draws may be NaN: never looked at).  ``restated``: the same
    definition with every distance and sum carried in float32 (running sums in
    k, then l, order), for a measurement of what fp32 arithmetic alone costs."""
    f = np.float32 if restated else np.float64
    pairs = np.asarray(pairs, bool)
    x = band_to_xy(np.asarray(draws)).astype(f)                      # [K, S, F, N, L, 2]
    K, S, F, N = x.shape[:4]
    assert K_MIN <= K <= K_MAX
    y = np.broadcast_to(np.asarray(targets).astype(f), (S, F, N, L, 2))
    with np.errstate(invalid="ignore"):
        m = np.zeros((3, S, F, N), f)
        for k in range(K):
            for i, v in enumerate(_afr(x[k] - y)):
                m[i] += v.astype(f)
        p = np.zeros((3, S, F, N), f)
        for k in range(K):
            for l in range(k + 1, K):
                for i, v in enumerate(_afr(x[k] - x[l])):
                    p[i] += v.astype(f)
        vm = np.zeros((S, F, N, L * (L - 1) // 2), f)
        for k in range(K):
            vm += _vario(x[k]).astype(f)
        vs = ((_vario(y).astype(f) - vm / f(K)) ** 2).sum(axis=-1)
    per = np.zeros((S, F, N, 8), np.float64)
    per[..., 0:3] = np.moveaxis(m, 0, -1) / K
    per[..., 3:6] = np.moveaxis(p, 0, -1) * (2.0 / (K * (K - 1)))
    per[..., 6] = vs
    per[~pairs] = 0.0
    out = np.zeros((S, 8))
    out[:, :7] = per[..., :7].sum(axis=(1, 2))
    out[:, 7] = pairs.sum(axis=(1, 2))
    return dict(per_ped=per, out=out, pairs=pairs)


def figures(out):
    """The host's figures from out [S, 8] (or any [..., 8] rows summed over the
    leading axes): means over the pairs."""
    t = np.asarray(out, np.float64).reshape(-1, 8).sum(axis=0)
    n = t[7]
    if not n > 0:
        return {k: float("nan") for k in ("es_traj", "es_ade", "es_fde", "mean_ade", "mean_fde", "apd", "vs")}
    return dict(es_traj=(t[2] - 0.5 * t[5]) / n, es_ade=(t[0] - 0.5 * t[3]) / n,
                es_fde=(t[1] - 0.5 * t[4]) / n, mean_ade=t[0] / n, mean_fde=t[1] / n, apd=t[3] / n,
                vs=t[6] / n)


def es_columns(per):
    """per_ped [..., 8] -> (es_ade, es_fde, es_traj) per pair."""
    return per[..., 0] - 0.5 * per[..., 3], per[..., 1] - 0.5 * per[..., 4], per[..., 2] - 0.5 * per[..., 5]
