"""float64 checker of the joint best-of-K evaluation (g2k_joint_eval_f32;
csrc/g2k_joint.hip states the definition): the K draws of oracle.g2k_ref
.gauss_sample at seeds (seed + k) mod 2^64 taken as JOINT samples of a
scene-frame — the mean over its members of each draw's ADE / FDE
(tests/bestk_ref.py draw_errors), the independent minima over k with the
lowest index attaining each — and, per draw, for the mean prediction and for
the targets, the member couples i < j whose smallest distance over the 12
predicted steps is below the radius.  The threshold is discontinuous, so next
to every count come the counts at radius - eps and radius + eps (col_lo <=
col <= col_hi) and the number of couples within eps of the radius (ambiguous).
Test helper, not a test module."""
import numpy as np

from oracle import g2k_ref as ref
from tests.bestk_ref import L, MASK64, draw_errors, pair_mask

EPS = 1e-4


def _band_xy(x):
    """[S, F, 2L, N] (band layout) -> [S, F, L, N, 2]."""
    return np.stack([x[:, :, :L], x[:, :, L:]], axis=-1)


def min_dist(xy):
    """xy [S, F, L, N, 2] -> [S, F, N, N]: min over the L steps of |xy_i - xy_j|."""
    S, F, _, N, _ = xy.shape
    out = np.full((S, F, N, N), np.inf)
    for t in range(L):                                    # step by step: [S, F, N, N] at a time
        d = xy[:, :, t, :, None, :] - xy[:, :, t, None, :, :]
        np.minimum(out, np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2), out=out)
    return out


def count(dmin, couples, radius, eps=EPS):
    """-> (col, col_lo, col_hi, ambiguous) [S, F] over the couples."""
    c = lambda r: ((dmin < r) & couples).sum(axis=(2, 3))   # noqa: E731
    amb = ((np.abs(dmin - radius) <= eps) & couples).sum(axis=(2, 3))
    return c(radius), c(radius - eps), c(radius + eps), amb


def joint_eval_ref(pred, targets, n_active, head, seed, K, radius, n_frames=None, ped_mask=None,
                   eps=EPS):
    """-> dict(per_frame_f [S, F, 4] = {minJADE, minJFDE, kJA, kJF},
    per_frame_i [S, F, 6] = {P, PP, col_pred, col_gt, sum_k col_k, col_best},
    sums_f [S, 4], sums_i [S, 6], members [S, F, N] bool, jade_k / jfde_k /
    col_k / col_lo / col_hi / amb_k [K, S, F], pred_lo / pred_hi / amb_pred /
    gt_lo / gt_hi / amb_gt [S, F])."""
    pred = np.asarray(pred, np.float64)
    targets = np.asarray(targets, np.float64)
    S, F, _, N = pred.shape
    m = pair_mask(S, F, N, n_active, n_frames, ped_mask)
    P = m.sum(axis=2)
    couples = m[:, :, :, None] & m[:, :, None, :] & np.triu(np.ones((N, N), bool), 1)
    PP = couples.sum(axis=(2, 3))
    assert np.array_equal(PP, P * (P - 1) // 2)
    Pd = np.maximum(P, 1)
    jade_k, jfde_k = np.zeros((K, S, F)), np.zeros((K, S, F))
    col_k, col_lo, col_hi, amb_k = (np.zeros((K, S, F), np.int64) for _ in range(4))
    for k in range(K):
        x = ref.gauss_sample(pred, head, (int(seed) + k) & MASK64)
        a, f = draw_errors(x, targets)
        jade_k[k] = (a * m).sum(axis=2) / Pd
        jfde_k[k] = (f * m).sum(axis=2) / Pd
        col_k[k], col_lo[k], col_hi[k], amb_k[k] = count(min_dist(_band_xy(x)), couples, radius, eps)
    col_pred, pred_lo, pred_hi, amb_pred = count(min_dist(_band_xy(pred)), couples, radius, eps)
    tg = np.broadcast_to(targets, (S, F, N, L, 2)).transpose(0, 1, 3, 2, 4)
    col_gt, gt_lo, gt_hi, amb_gt = count(min_dist(tg), couples, radius, eps)
    on = P > 0
    kJA, kJF = jade_k.argmin(axis=0), jfde_k.argmin(axis=0)          # the first (lowest) minimum
    pf = np.stack([jade_k.min(axis=0), jfde_k.min(axis=0), kJA.astype(np.float64),
                   kJF.astype(np.float64)], axis=-1) * on[..., None]
    col_best = np.take_along_axis(col_k, kJA[None], axis=0)[0]
    pi = np.stack([P, PP, col_pred, col_gt, col_k.sum(axis=0), col_best], axis=-1).astype(np.int64)
    pi = pi * on[..., None]
    sums_f = np.zeros((S, 4))
    sums_f[:, 0] = (P * pf[..., 0]).sum(axis=1)
    sums_f[:, 1] = (P * pf[..., 1]).sum(axis=1)
    sums_f[:, 2] = K
    return dict(per_frame_f=pf, per_frame_i=pi, sums_f=sums_f, sums_i=pi.sum(axis=1), members=m,
                jade_k=jade_k, jfde_k=jfde_k, col_k=col_k, col_lo=col_lo, col_hi=col_hi, amb_k=amb_k,
                pred_lo=pred_lo, pred_hi=pred_hi, amb_pred=amb_pred, gt_lo=gt_lo, gt_hi=gt_hi,
                amb_gt=amb_gt)


def couples_case(rng_seed=0, S=3, F=2, N=20, sigma=1e-3):
    """The structured case with a hand-countable answer: pedestrians 2c and
    2c + 1 form couple c, 0.05 apart at every step; couples sit on a grid 1.5
    apart and all walk the same way, so members of different couples stay
    >= 1.0 apart; the head's sigma is 1e-3.  The mask breaks some couples (one
    partner masked) and removes others whole; n_active may cut a couple too.
    With radius 0.1 every draw, the mean and the targets collide in exactly the
    intact couples.  -> (inputs dict, intact [S, F] the hand count)."""
    rng = np.random.default_rng(rng_seed)
    c = np.arange(N) // 2
    x0 = 1.5 * (c % 4) + 0.05 * (np.arange(N) % 2)
    y0 = 1.5 * (c // 4).astype(np.float64)
    t = np.arange(L)
    pred = np.zeros((S, F, 2 * L, N))
    for s in range(S):
        for f in range(F):
            vx, vy = 0.1 * rng.standard_normal(2)
            pred[s, f, :L] = x0[None, :] + vx * t[:, None]
            pred[s, f, L:] = y0[None, :] + vy * t[:, None]
    pred = pred.astype(np.float32)
    tg = np.ascontiguousarray(_band_xy(pred).transpose(0, 1, 3, 2, 4)
                              + 1e-3 * rng.standard_normal((S, F, N, L, 2))).astype(np.float32)
    head = np.stack([np.full(L, np.log(sigma)), np.full(L, np.log(sigma)),
                     0.3 * rng.standard_normal(L)]).astype(np.float32)
    n_active = np.array([N, N - 3, N - 8], np.int32)[:S]          # N - 3 cuts a couple in two
    n_frames = np.array([F, F, max(F - 1, 0)], np.int32)[:S]
    pm = np.ones((S, N), np.uint8)
    pm[:, 2] = 0                                                   # couple 1 broken
    pm[0, 7] = 0                                                   # couple 3 broken in scene 0
    pm[1, 8:10] = 0                                                # couple 4 gone in scene 1
    m = pair_mask(S, F, N, n_active, n_frames, pm)
    intact = (m[:, :, 0::2] & m[:, :, 1::2]).sum(axis=2)
    return dict(pred=pred, targets=tg, head=head, n_active=n_active, n_frames=n_frames, ped_mask=pm,
                radius=0.1), intact
