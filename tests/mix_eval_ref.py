"""float64 checkers of the Gaussian-mixture head's fused joint best-of-K and
KDE-NLL evaluations (g2k_mix_joint_eval_f32, g2k_mix_kde_nll_f32;
include/g2k_mix.h, csrc/g2k_joint.hip and csrc/g2k_kde.hip state the
definitions): the full-covariance head's checkers (tests/fullcov_joint_ref.py,
tests/kde_ref.py) with tests/mixture_ref.sample as the draw, and the test
mixtures.  Dead slots, floats 1..7 and the entries above the diagonals of a
test block hold NaN: a finite result never read them.  Test helper, not a test
module.

The KDE kernel's moment scheme for this head differs from the other heads'
(kde_ref's ``restated=True``): the draws sit around mu + b_m, so the fp32
moments are a running mean and centred sums (Welford's update; the lanes'
partial results merged by Chan's formula).  ``kde_nll_ref(restated=True)``
restates THAT split: fp32 Welford moments of d = x - mu in draw order, the
bandwidth in double, its inverse and the constant rounded to fp32, fp32
distances and log-sum-exp."""
import functools

import numpy as np

from tests import fullcov_joint_ref as fj
from tests import kde_cases as kc
from tests import kde_ref as kr
from tests import mixture_ref as mr
from tests.bestk_ref import L, MASK64, draw_errors, pair_mask
from tests.joint_ref import EPS, count, min_dist

SLOTS3 = (0, 2, 5)
ALL8 = tuple(range(mr.SLOTS))

# The GPU tests' gate on |kernel - float64 checker| of the KDE-NLL, absolute,
# per term and per pair's kde_nll: 8 x the worst |restated precision - float64|
# over the eight tests/kde_cases.py inputs with the checker's mixture draws,
# near (b = 1.5 N(0, 1)) and far (b = 10 N(0, 1)) blocks.  Measured worst
# (tests/test_mix_eval.py::test_kde_gate_measurement prints it): 1.88e-4 (a
# term, case shared, far block; near block 9.3e-5, case k4), 9.3e-5 (a pair's
# kde_nll, near block, case k4).  With the other heads' moments (plain sums of
# x - mu, kde_ref's restatement) the same inputs give 6.1e-4 far and 8.4e-4
# near; with the sums centred on the pair's draw 0, 2.9e-4 and 5.8e-4.  What is
# left at the far block is the fp32 distance y - x_k at coordinates of 10..30,
# which no centring removes.  The factor 8 is tests/kde_ref.py's: the device's
# expf / logf and a summation order that varies with KS.
MEASURED_WORST = 1.9e-4
GATE = 8 * MEASURED_WORST
KDE_SCALES = {"near": 1.5, "far": 10.0}
# a step is "near det H = 0" when det H <= NEAR_SINGULAR hxx hyy (1 - rho^2 of
# the draws): fp32 centred sums of up to 200 terms carry a relative error of
# the order 200 x 2^-24 = 1.2e-5, which decides the sign of a determinant only
# below that; ten times the margin
NEAR_SINGULAR = 1e-4


def make_block(weights, bs, chols, slots):
    """[8, 608] f32: slot slots[q] = (weights[q], bs[q], tril(chols[q])); NaN
    in dead slots (their w is 0), in floats 1..7 and above the diagonals."""
    p = np.full((mr.SLOTS, mr.PITCH), np.nan, np.float32)
    p[:, 0] = 0.0
    for q, m in enumerate(slots):
        p[m, 0] = weights[q]
        p[m, mr.OFF_B:mr.OFF_L] = bs[q]
        p[m, mr.OFF_L:] = fj.nan_above(chols[q]).reshape(-1)
    return p


def mix_block(sigma, rs, slots=SLOTS3):
    """The joint tests' mixture: weights U(0.2, 1) and b = 1.5 sigma N(0, 1)
    from default_rng(rs + 2000) (the weights first), slot m's factor
    walk_factor(sigma, default_rng(rs + 1000 + m))."""
    rng = np.random.default_rng(rs + 2000)
    w = rng.uniform(0.2, 1.0, len(slots))
    bs = 1.5 * sigma * rng.standard_normal((len(slots), mr.DIM))
    return make_block(w, bs, [fj.walk_factor(sigma, np.random.default_rng(rs + 1000 + m)) for m in slots],
                      slots)


def one_slot_block(chol):
    """What MixtureHead.from_fullcov builds, with the NaN of a test block."""
    return make_block([1.0], [np.zeros(mr.DIM)], [chol], (0,))


@functools.lru_cache(maxsize=None)
def kde_block(i, which):
    """The KDE tests' mixture of tests/kde_cases.py case i: slots {0, 2, 5},
    weights U(0.2, 1), the case's chol as every factor, b = scale N(0, 1)
    (KDE_SCALES[which]) from default_rng(7000 + 100 * (which == "far") + i)."""
    rng = np.random.default_rng(7000 + (100 if which == "far" else 0) + i)
    w = rng.uniform(0.2, 1.0, 3)
    bs = KDE_SCALES[which] * rng.standard_normal((3, mr.DIM))
    return make_block(w, bs, [kc.inputs(i)["chol"]] * 3, SLOTS3)


@functools.lru_cache(maxsize=None)
def kde_draws(i, which):
    """[K, S, F, 24, N] float32: the checker's draws of case i's mixture for
    seeds seed + k, rounded to the sampler's fp32."""
    c = kc.inputs(i)
    mix = kde_block(i, which)
    with np.errstate(invalid="ignore"):
        d = [mr.sample(c["pred"], mix, (c["seed"] + k) & MASK64)[0] for k in range(c["K"])]
    return np.stack(d).astype(np.float32)


def joint_eval_ref(pred, targets, n_active, mix, seed, K, radius, n_frames=None, ped_mask=None,
                   eps=EPS):
    """tests/fullcov_joint_ref.joint_eval_ref with mixture_ref.sample(...)[0]
    as joint sample k -> the same dictionary, brackets included."""
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
        x = mr.sample(pred, mix, (int(seed) + k) & MASK64)[0]
        a, f = draw_errors(x, targets)
        jade_k[k] = (a * m).sum(axis=2) / Pd
        jfde_k[k] = (f * m).sum(axis=2) / Pd
        col_k[k], col_lo[k], col_hi[k], amb_k[k] = count(min_dist(fj._band_xy(x)), couples, radius, eps)
    col_pred, pred_lo, pred_hi, amb_pred = count(min_dist(fj._band_xy(pred)), couples, radius, eps)
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


def welford_logp(x, y, center):
    """kde_ref.kde_logp's restated branch with this head's moments: x [K, ...,
    2] f32, y, center [..., 2] -> (logp, ok)."""
    x = np.asarray(x, np.float32)
    y = np.asarray(y, np.float32)
    K = x.shape[0]
    scott = float(K) ** (-1.0 / 3.0)
    f32 = np.float32
    with np.errstate(all="ignore"):
        d = x - np.asarray(center, np.float32)
        mx, my, sxx, syy, sxy = (np.zeros(d.shape[1:-1], np.float32) for _ in range(5))
        for k in range(K):                                  # running mean, centred sums: fp32
            rc = f32(1.0) / f32(k + 1)
            ux, uy = d[k, ..., 0] - mx, d[k, ..., 1] - my
            mx = mx + ux * rc
            my = my + uy * rc
            vx, vy = d[k, ..., 0] - mx, d[k, ..., 1] - my
            sxx = sxx + ux * vx
            syy = syy + uy * vy
            sxy = sxy + ux * vy
        for a in (mx, sxx, syy, sxy):
            assert a.dtype == np.float32
        hxx, hyy, hxy = (scott * s.astype(np.float64) / (K - 1) for s in (sxx, syy, sxy))
        det = hxx * hyy - hxy * hxy
        ok = (det > 0) & np.isfinite(det)
        sdet = np.where(ok, det, 1.0)
        ixx, iyy, ixy = hyy / sdet, hxx / sdet, -hxy / sdet
        cst = -np.log(float(K)) - kr.LOG_2PI - 0.5 * np.log(sdet)
        ixx, iyy, ixy, cst = (v.astype(f32) for v in (ixx, iyy, ixy, cst))
        ex, ey = y[..., 0] - x[..., 0], y[..., 1] - x[..., 1]
        a = f32(-0.5) * (ixx * ex * ex + f32(2) * ixy * ex * ey + iyy * ey * ey)
        m = a.max(axis=0)
        lse = m + np.log(np.exp(a - m).sum(axis=0, dtype=f32))
        logp = np.where(ok, cst + lse, -np.inf)
    return logp.astype(np.float64), ok


def kde_nll_ref(draws, targets, pairs, log_floor=-20.0, pred=None, restated=False):
    """tests/kde_ref.kde_nll_ref on mixture draws [K, S, F, 2L, N] -> the same
    dictionary plus near_singular [S, F, N, L] (det H <= NEAR_SINGULAR hxx hyy
    in float64).  ``restated`` (needs ``pred``): this head's precision split."""
    R = kr.kde_nll_ref(draws, targets, pairs, log_floor)
    draws = np.asarray(draws)
    K, S, F, _, N = draws.shape
    x = kr.band_to_xy(draws)
    with np.errstate(all="ignore"):
        d = x.astype(np.float64) - x.astype(np.float64).mean(axis=0)
        cxx, cyy = (d[..., 0] ** 2).sum(axis=0), (d[..., 1] ** 2).sum(axis=0)
        cxy = (d[..., 0] * d[..., 1]).sum(axis=0)
        R["near_singular"] = ~(cxx * cyy - cxy * cxy > NEAR_SINGULAR * cxx * cyy)
    if not restated:
        return R
    y = np.broadcast_to(np.asarray(targets), (S, F, N, L, 2))
    logp, ok = welford_logp(x, y, kr.band_to_xy(pred))
    with np.errstate(invalid="ignore"):
        clip = ~ok | ~(logp >= log_floor)
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
    return dict(per_ped=per, out=out, logp=logp, term=term, clip=clip, near_singular=R["near_singular"])


# ---------------------------------------------------------------------------
# the joint tests' runs: tests/test_fullcov_joint_gpu.py's cases with a mixture
# ---------------------------------------------------------------------------
def joint_runs():
    """(RUNS, RUN_IDS): that file's (case, radius) runs with slots {0, 2, 5},
    then the n256 case with all 8 slots live; a run is (case, radius, slots)."""
    from tests import test_fullcov_joint_gpu as tj
    runs = [(i, r, SLOTS3) for i, r in tj.RUNS] + [(tj.IDS.index("n256"), 0.3, ALL8)]
    return runs, list(tj.RUN_IDS) + ["n256-r0.3-slots8"]


@functools.lru_cache(maxsize=None)
def joint_inputs(i, slots=SLOTS3):
    """Case i of tests/test_fullcov_joint_gpu.py (its pred / targets / mask
    construction, K and seed) with ``mix`` = mix_block(sigma, rs, slots); the
    structured couples case takes sigma 1e-3 and rs -1 (its factor's rng is
    default_rng(999))."""
    from tests import test_fullcov_joint_gpu as tj
    c = dict(tj._inputs(i))
    sigma, rs = (1e-3, -1) if i == tj.COUPLES else (tj.CASES[i][4], tj.CASES[i][10])
    c["mix"] = mix_block(sigma, rs, slots)
    return c


@functools.lru_cache(maxsize=None)
def joint_reference(i, radius, slots=SLOTS3):
    c = joint_inputs(i, slots)
    return joint_eval_ref(c["pred"], c["targets"], c["n_active"], c["mix"], c["seed"], c["K"], radius,
                          c["n_frames"], c["ped_mask"])
