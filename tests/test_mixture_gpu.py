"""GPU: the Gaussian-mixture trajectory head (csrc/g2k_mix.hip, the MixHead
policy of csrc/g2k_head_draw.h; mixture.MixtureHead; evaluate.py
--mixture_head) against the float64 checker tests/mixture_ref.py.  PARITY
UNPINNED: the reference has no probabilistic head.

EM.  The kernels deal the S F Nmax slots to workgroups of at least 512 slots,
so S 2 x F 3 x Nmax 5 (30 slots; a mask, a scene with n_active = 0, one with
n_frames < F, shared targets in one variant) is one workgroup and S 4 x F 8 x
Nmax 33 (1056 slots) three, whose ranges end inside a scene-frame
(test_em_cases_cover_both_reductions).  Blocks of 1, 3 and 8 live slots; the
3-slot block has dead slots between the live ones; every block holds NaN in
floats 1..7, above the diagonals and all over its dead slots, and every
non-pair of pred and targets is NaN: finite outputs prove none was read.
Bounds: pairs and hard counts exact (no two gamma of a pair within 1e-9 of
each other, asserted on the checker); moments, resp and total within EM_TOL
max(1, |ref|); new w and b 1e-6 relative (the f32 rounding); new factors by the
backward error |L L^T - C| <= 1e-4 max|C|.

Three more cases reach what well-conditioned inputs never do, at the same
bounds (em_branch_preconditions holds, on the checker alone, the conditions
under which they do): "outliers" (a tenth of the pairs 40 sigma out: every
exp(l_m) is 0 in double, so only the max-shifted logsumexp of
g2k_mix_resp_kernel is finite), "starved" (a twin slot with 0 < N_m < 0.5 and
a far slot with N_m = 0 exactly: the "too little mass" branch of
g2k_mix_finish_kernel keeps b and the lower triangle bit for bit, zeroes what
held NaN, and w = N_m / n = 0 kills the far slot for the second step, which is
run and checked too) and "cap" (132600 slots: 256 workgroups of 518 slots,
three rounds each, the last workgroup 510).  test_em_without_a_pair is the
n = 0 arm of that branch through the raw ABI.

fit(iters=5) is five em_step calls bit for bit.  Its trace is compared with
the checker twice: each iteration's log-likelihood against the checker's on
the SAME block (the device's), and against the checker's own five
free-running steps, both within EM_TOL (the second holds because on this data
the device's float32 blocks are the checker's bit for bit at every step).

Sampler and best-of-K: the four properties tests/test_fullcov_gpu.py checks
(values within 1e-4 max(1, |ref|) of the checker, the indices attain the
checker's minimum, ``best`` is the unfused draw bit for bit, repeated calls
are bit-identical), ``comp`` equal to the checker's, and the one-slot b = 0
mixture equal to FullCovHead bit for bit.

Measured on an MI355X: moments within 1.4e-15, resp within 1.9e-16 and total
within 6.4e-16 of max(1, |ref|) (EM_TOL stays at the 1e-12 the full-covariance
stats are held to), every hard count equal, new w and b equal to the checker's
float32 bits, |L L^T - C| <= 8.1e-8 max|C|; the fit's trace within 2.5e-16 of
the checker's on the same blocks and of its own five steps; the sampler within
1.9e-6 and best-of-K's per_ped within 8.5e-7, sums within 2.9e-7 of the
checker, every index attaining the checker's minimum exactly.
The new cases (moments / resp / total of max(1, |ref|), against EM_TOL 1e-12):
outliers 7.6e-15 / 1.7e-16 / 0; starved 2.8e-14 / 1.5e-16 / 1.1e-16 and its
second step 3.6e-14 / 1.7e-16 / 2.8e-14; cap 2.2e-15 / 6.6e-16 / 5.9e-16 (67091
pairs; its em_step, the copy of the inputs included, took 73 ms as the first
launch of a process, the whole test 0.2 s); new w and b
the checker's float32 bits and |L L^T - C| <= 6.8e-8 max|C| in all of them; the
kept slots bit for bit.  On the CPU, the two float64 formulations of the E-step
(the checker's solve / the explicit forward-substituted inverse the kernel
forms) disagree by 0 on "outliers" (the outliers' max l_m in [-3.5e4, -4.9e3],
their two best l_m at least 1109 apart: every gamma saturates), by 1.7e-18 on
"starved" and by at most 5e-15 (total) on its second step: 200 times below
EM_TOL at the least.  The selector's edges: comp equal to the checker's in all
three blocks ({2, 6} only with cw[4] == cw[2]: 524 + 532 and 548 + 508 of 1056;
all 1056 in slot 1, in slot 7), draws within 1.1e-6."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib
from tests import fullcov_ref as fr
from tests import mixture_ref as mr
from tests.abi_arena import Arena, all_written
from tests.bestk_ref import MASK64, pair_mask
from tests.conftest import close

pytestmark = pytest.mark.gpu
TOL = 1e-4
EM_TOL = 1e-12                 # moments, resp, total: of max(1, |ref|)
OUT_SIGMA = 40.0               # how far out the outliers of the "outliers" / "starved" cases lie
SEED = (7 << 32) + 99


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _mix(block, dev):
    from multimodaltraj_2_amd.mixture import MixtureHead
    return MixtureHead.from_block(np.asarray(block, np.float32), device=dev)


def _factor(rng, scale=0.05):
    Lm = np.zeros((24, 24))
    for i in range(24):
        for j in range(i + 1):
            Lm[i, j] = scale * (1.0 if i == j else 0.6 ** ((i - j + 1) // 2)) * (0.5 + rng.random())
    return Lm


def _block(rng, slots, scale=0.05):
    """Live ``slots`` with random weights, offsets and factors; NaN wherever
    the definition says nothing is read."""
    p = np.full((8, 608), np.nan, np.float32)
    p[:, 0] = 0
    for m in slots:
        p[m, 0] = rng.uniform(0.2, 1.0)                   # need not sum to 1
        p[m, 8:32] = scale * rng.standard_normal(24)
        Lm = _factor(rng, scale)
        Lm[np.triu_indices(24, 1)] = np.nan
        p[m, 32:] = Lm.reshape(-1)
    return p


# ---------------------------------------------------------------------------
# EM
# ---------------------------------------------------------------------------
#            S  F  Nmax n_active        n_frames      shared  live slots
EM_CASES = [(2, 3, 5, [5, 0], [2, 3], False, (0,)),
            (2, 3, 5, [5, 0], [2, 3], False, (0, 2, 5)),
            (2, 3, 5, [4, 5], [3, 1], True, tuple(range(8))),
            (4, 8, 33, [33, 0, 17, 30], [8, 8, 5, 7], False, (3,)),
            (4, 8, 33, [33, 0, 17, 30], [8, 8, 5, 7], False, (0, 2, 5)),
            (4, 8, 33, [33, 20, 17, 30], [8, 8, 5, 7], False, tuple(range(8)))]
EM_IDS = ["one-1", "one-3gap", "one-shared-8", "rows-1", "rows-3gap", "rows-8"]
# the branches the cases above never reach (test_em_new_cases_reach_their_branches
# holds the conditions, on the checker alone):
#  outliers  a tenth of the pairs tens of sigma from every component: exp(l_m)
#            is 0 in double for every m, only the max-shifted logsumexp is finite
#  starved   slots 0, 2, 5 as in "outliers"; slot 3 is slot 2's twin (its b and L,
#            1e-4 of its w: 0 < N_m < 0.5), slot 6 is far from every pair (N_m is
#            exactly 0): the finish kernel's "too little mass" branch
#  cap       132600 slots: mix_geom's 256-workgroup cap, 518 slots a workgroup
#            (three rounds, the last of 6), the last workgroup 510
OUTLIERS, STARVED, CAP = 6, 7, 8
TWIN, TWIN_OF, FAR = 3, 2, 6
ORDINARY = (0, 2, 5)
EM_CASES += [(4, 8, 33, [33, 0, 17, 30], [8, 8, 5, 7], False, ORDINARY),
             (4, 8, 33, [33, 0, 17, 30], [8, 8, 5, 7], False, (0, 2, TWIN, 5, FAR)),
             (26, 20, 255, [255, 0] + [255 - 9 * s for s in range(2, 26)], [20, 20, 20, 13] + [20] * 22, False,
              (1, 6))]
EM_IDS += ["outliers", "starved", "cap"]
SMALL = [i for i in range(len(EM_CASES)) if i != CAP]


@functools.lru_cache(maxsize=None)
def _em_inputs(i):
    S, F, N, nact, nfr, shared, slots = EM_CASES[i]
    rng = np.random.default_rng(900 + i)
    nact, nfr = np.asarray(nact, np.int32), np.asarray(nfr, np.int32)
    pm = np.ones((S, N), np.uint8)
    pm[:, 1] = 0
    drawn = ORDINARY if i == STARVED else slots            # the slots the residuals are drawn from
    mix = _block(rng, drawn)
    # residuals from a mixture near the block's: every component gets pairs
    Ft = 1 if shared else F
    k = rng.choice(np.asarray(drawn), size=(S, Ft, N))
    r = np.empty((S, Ft, N, 24))
    for m in drawn:
        Lm = np.tril(np.nan_to_num(mix[m, 32:].reshape(24, 24).astype(np.float64)))
        r[k == m] = 1.3 * mix[m, 8:32] + rng.standard_normal((int((k == m).sum()), 24)) @ (1.2 * Lm).T
    far_out = np.zeros((S, Ft, N), bool)
    if i in (OUTLIERS, STARVED):
        # a tenth of the pairs far out, each along its own component's shape
        # (OUT_SIGMA sigma of it), so that the other components are farther
        # still: gamma saturates to exactly 1 / 0 and the E-step's sums do not
        # depend on how a formulation rounds q (test_em_new_cases_reach_their_branches)
        far_out = rng.random((S, Ft, N)) < 0.1
        for m in drawn:
            sel = far_out & (k == m)
            Lm = np.tril(np.nan_to_num(mix[m, 32:].reshape(24, 24).astype(np.float64)))
            r[sel] = mix[m, 8:32] + OUT_SIGMA * rng.standard_normal((int(sel.sum()), 24)) @ Lm.T
    if i == STARVED:
        mix[TWIN] = mix[TWIN_OF]
        mix[TWIN, 0] = np.float32(1e-4) * mix[TWIN_OF, 0]
        mix[FAR, 0] = 0.5
        mix[FAR, 8:32] = 1000.0 + rng.standard_normal(24)
        Lf = _factor(rng)
        Lf[np.triu_indices(24, 1)] = np.nan
        mix[FAR, 32:] = Lf.reshape(-1)
    pred = rng.standard_normal((S, F, 24, N)).astype(np.float32)
    if shared:
        # one prediction for every frame, so that the residuals against the one
        # target set stay of the components' scale: a component that holds a
        # single pair has C = r r^T - r r^T + ridge, which any two float64
        # evaluations agree on only to eps |r|^2 / 1e-12 of max|C| — below the
        # factor's 1e-4 for |r| ~ 0.1, not for |r| ~ 1
        pred[:] = pred[:, :1]
    tg = np.empty((S, Ft, N, 12, 2))
    tg[..., 0] = np.transpose(pred[:, :Ft, :12], (0, 1, 3, 2)) + r[..., 0::2]
    tg[..., 1] = np.transpose(pred[:, :Ft, 12:], (0, 1, 3, 2)) + r[..., 1::2]
    tg = np.ascontiguousarray(tg.astype(np.float32))
    m = pair_mask(S, F, N, nact, nfr, pm)
    np.transpose(pred, (0, 1, 3, 2))[~m] = np.nan         # a view: pred itself
    if shared:
        tg[:, 0][~m.any(axis=1)] = np.nan
    else:
        tg[~m] = np.nan
    return dict(pred=pred, targets=tg, mix=mix, n_active=nact, n_frames=nfr, ped_mask=pm,
                shared=shared, pairs=int(m.sum()),
                outlier=np.broadcast_to(far_out, (S, F, N))[m])          # per pair, in the checker's order


@functools.lru_cache(maxsize=None)
def _em_reference(i):
    c = _em_inputs(i)
    return mr.em_ref(c["pred"], c["targets"], c["n_active"], c["mix"], c["n_frames"], c["ped_mask"])


def _em_run(i, dev, update=True):
    c = _em_inputs(i)
    h = _mix(c["mix"], dev)
    st = h.em_step(_t(c["pred"], dev), _t(c["targets"], dev), _t(c["n_active"], dev),
                   n_frames=_t(c["n_frames"], dev), ped_mask=_t(c["ped_mask"], dev),
                   targets_shared=c["shared"], update=update)
    torch.cuda.synchronize()
    return h, st


_EM = {}


def _em_result(i, dev):
    if i not in _EM:
        _EM[i] = _em_run(i, dev)
    return _EM[i]


def _ws_bytes(S, F, N):
    d = _lib.G2KDims(S, F, 8, 12, 16, 64, N, 8, 0)
    from multimodaltraj_2_amd import mixture
    return int(mixture.load().g2k_mix_em_workspace_bytes(ctypes.byref(d)))


def test_em_cases_cover_both_reductions():
    """By the launch's own workspace (gamma [8][slots], then a row [10] and 8
    rows [448] per workgroup): the small shape is one workgroup, the large one
    three whose ranges end inside a scene-frame; every live component of every
    case gets pairs, and no two gamma of a pair are within 1e-9."""
    per_wg = 8 * (10 + 8 * 448)
    assert _ws_bytes(2, 3, 5) == 8 * 8 * 30 + per_wg
    assert _ws_bytes(4, 8, 33) == 8 * 8 * 1056 + 3 * per_wg
    assert -(-1056 // 3) % 33 != 0
    for i in range(len(EM_CASES)):
        R, c = _em_reference(i), _em_inputs(i)
        assert R["total"][0] == c["pairs"] > 0
        g = np.sort(R["gamma"], axis=1)
        if len(EM_CASES[i][6]) > 1:
            assert (g[:, -1] - g[:, -2]).min() > 1e-9, EM_IDS[i]
        assert np.all(R["resp"][[m for m in EM_CASES[i][6] if (i, m) != (STARVED, FAR)], 0] > 0)
    assert _em_inputs(0)["pairs"] < 24 and _em_inputs(4)["pairs"] > 300


def _forward_inverse(Lm):
    """L^-1 a column at a time by forward substitution, as g2k_mix_resp_kernel
    forms it (float64)."""
    W = np.zeros_like(Lm)
    for c in range(24):
        for i in range(24):
            acc = (1.0 if i == c else 0.0) - Lm[i, :i] @ W[:i, c]
            W[i, c] = acc / Lm[i, i]
    return W


def _e_step_by_explicit_inverse(r, mix):
    """The checker's E-step sums with q_m = ||W_m (r - b_m)||^2, W_m the explicit
    inverse, where tests/mixture_ref.py solves L_m z = r - b_m: a second
    float64 formulation, for the sensitivity of the sums to how q is rounded."""
    w, b, Lm = mr.unpack(mix)
    lv = np.flatnonzero(mr.live(mix))
    lm = np.full((r.shape[0], 8), -np.inf)
    for m in lv:
        z = (r - b[m]) @ _forward_inverse(Lm[m]).T
        lm[:, m] = (np.log(w[m] / w.sum()) - 12.0 * mr.LOG_2PI - np.log(np.diag(Lm[m])).sum()
                    - 0.5 * (z * z).sum(axis=1))
    lmax = lm.max(axis=1)
    l = lmax + np.log(np.exp(lm - lmax[:, None]).sum(axis=1))
    g = np.exp(lm - l[:, None])
    mo, rs = np.zeros((8, 25, 24)), np.zeros((8, 2))
    for m in lv:
        mo[m, :24], mo[m, 24] = (r * g[:, m, None]).T @ r, g[:, m] @ r
        rs[m] = g[:, m].sum(), (g.argmax(axis=1) == m).sum()
    return mo, rs, np.array([r.shape[0], l.sum(), 0.0, 0.0])


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def _residuals(c):
    return fr.residuals(c["pred"], c["targets"], c["n_active"], c["n_frames"], c["ped_mask"])


def em_branch_preconditions(log=print):
    """What makes the cases "outliers", "starved" and "cap" reach the branches
    they are for: conditions on the inputs, on tests/mixture_ref.py alone (no
    GPU).  tests/test_mixture.py runs this in the CPU suite too.

    MEASURED (CPU): the outliers' max_m l_m lies in [-3.5e4, -4.9e3], their two
    best l_m 1109 apart at the least ("outliers"; in "starved" the twin is
    log 1e4 = 9.21 below its original by construction); the disagreement of the
    two float64 E-step formulations (solve / explicit forward-substituted
    inverse), of max(1, |ref|): "outliers" 0 (moments, resp and total alike:
    every gamma the same double), "starved" 1.7e-18 / 0 / 0 and its second step
    2.3e-16 / 0 / 5.0e-15 (3.0e-15 with another BLAS): 200 times below EM_TOL at
    the least, where 10 are asked."""
    for i in (OUTLIERS, STARVED):
        c, R = _em_inputs(i), _em_reference(i)
        r, o = _residuals(c), c["outlier"]
        d = mr.log_density(r, c["mix"])
        best = d["lm"].max(axis=1)
        assert 0.05 * c["pairs"] < o.sum() < 0.2 * c["pairs"]
        # every exp(l_m) of an outlier is 0 in double: the unshifted logsumexp of
        # the checker's own l_m is -inf, the shifted one is what the checker has
        assert best[o].max() < -745.0 and best[~o].min() > -100.0
        with np.errstate(divide="ignore"):
            naive = np.log(np.exp(d["lm"]).sum(axis=1))
        assert np.all(np.isneginf(naive[o])) and np.all(np.isfinite(naive[~o]))
        assert np.all(np.isfinite(d["l"])) and np.array_equal(d["l"], R["l"])
        for k in ("moments", "resp", "total", "mix_out"):
            assert np.all(np.isfinite(R[k])), (EM_IDS[i], k)
        g = np.sort(R["gamma"], axis=1)
        assert (g[:, -1] - g[:, -2]).min() > 1e-9, EM_IDS[i]
        mo, rs, tt = _e_step_by_explicit_inverse(r, c["mix"])
        sens = (_rel(mo, R["moments"]), _rel(rs, R["resp"]), _rel(tt, R["total"]))
        top = np.sort(d["lm"][o], axis=1)
        log(f"case {EM_IDS[i]}: {int(o.sum())} outliers of {c['pairs']} pairs, their max l_m in "
            f"[{best[o].min():.3g}, {best[o].max():.3g}], two best l_m apart by >= "
            f"{(top[:, -1] - top[:, -2]).min():.4g}; two float64 E-steps disagree by "
            f"{sens[0]:.3g} / {sens[1]:.3g} / {sens[2]:.3g} (moments / resp / total)")
        assert max(sens) <= EM_TOL / 10
    N = _em_reference(OUTLIERS)["resp"][:, 0]
    assert np.all(N[list(ORDINARY)] > 2.0)
    # starved: the twin gets a little mass, the far slot exactly none, and no
    # live slot sits where N >= 1 hangs on the last bit; the same after the step
    c, R = _em_inputs(STARVED), _em_reference(STARVED)
    assert np.array_equal(c["mix"][TWIN, 8:].view(np.int32), c["mix"][TWIN_OF, 8:].view(np.int32))
    r = _residuals(c)
    for step, E in (("first", R), ("second", mr.em_step(r, R["mix_out"]))):
        N = E["resp"][:, 0]
        live = np.flatnonzero(mr.live(c["mix"] if step == "first" else R["mix_out"]))
        log(f"case starved, {step} step: live {list(live)}, N_m {N[live]}")
        assert np.all(N[list(ORDINARY)] > 2.0) and not np.any((N[live] >= 0.5) & (N[live] <= 2.0))
        g = np.sort(E["gamma"], axis=1)
        assert (g[:, -1] - g[:, -2]).min() > 1e-9
        if step == "first":
            assert list(live) == sorted(EM_CASES[STARVED][6]) and N[FAR] == 0.0 and 0.0 < N[TWIN] < 0.5
            assert E["C"][TWIN] is None and E["C"][FAR] is None
            assert E["mix_out"][FAR, 0] == 0.0 and E["mix_out"][TWIN, 0] > 0.0
        else:
            # the far slot died; the twin, still where slot TWIN_OF was, now takes
            # that slot's inliers (the slot itself widened over its outliers)
            assert list(live) == sorted(ORDINARY + (TWIN,))
            mo, rs, tt = _e_step_by_explicit_inverse(r, R["mix_out"])
            sens = (_rel(mo, E["moments"]), _rel(rs, E["resp"]), _rel(tt, E["total"]))
            log(f"case starved, second step: two float64 E-steps disagree by {sens[0]:.3g} / {sens[1]:.3g} "
                f"/ {sens[2]:.3g}")
            assert max(sens) <= EM_TOL / 10
    # cap: more than 131072 slots, so 256 workgroups of U slots, three rounds
    # each, the last one partial, the ranges ending inside a scene-frame
    S, F, Nm = EM_CASES[CAP][:3]
    slots, per_wg = S * F * Nm, 8 * (10 + 8 * 448)
    assert slots > 131072 and _ws_bytes(S, F, Nm) == 8 * 8 * slots + 256 * per_wg
    U = -(-slots // 256)
    assert U > 512 and U % Nm != 0 and U % 256 != 0 and 0 < slots - 255 * U < U
    c, R = _em_inputs(CAP), _em_reference(CAP)
    assert c["n_frames"].min() < F and c["n_active"].min() == 0 and not c["ped_mask"].all()
    assert np.all(R["resp"][list(EM_CASES[CAP][6]), 0] > 2.0)
    g = np.sort(R["gamma"], axis=1)
    assert (g[:, -1] - g[:, -2]).min() > 1e-9
    log(f"case cap: {slots} slots, U {U} (last workgroup {slots - 255 * U}), {c['pairs']} pairs")


def test_em_new_cases_reach_their_branches():
    em_branch_preconditions()


def _check_em_step(name, mo, rs, tt, out, R, slots):
    """One step's outputs (host arrays) against the checker's R at the bounds
    of the module docstring; ``slots`` are the live slots of the step's block.
    -> {quantity: its worst error over its bound}."""
    dead = [m for m in range(8) if m not in slots]
    assert mo.dtype == rs.dtype == tt.dtype == np.float64
    assert np.all(np.isfinite(mo)) and np.all(np.isfinite(rs)) and np.all(np.isfinite(tt))
    assert tt[0] == R["total"][0] and tt[2] == tt[3] == 0
    np.testing.assert_array_equal(rs[:, 1], R["resp"][:, 1])              # hard counts: exact
    assert np.all(mo[dead] == 0) and np.all(rs[dead] == 0)
    np.testing.assert_array_equal(mo[:, :24], np.transpose(mo[:, :24], (0, 2, 1)))
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
    em, er, et = rel(mo, R["moments"]), rel(rs, R["resp"]), rel(tt, R["total"])
    print(f"case {name}: {int(tt[0])} pairs, moments err {em:.3g}, resp err {er:.3g}, "
          f"total err {et:.3g}")
    assert em <= EM_TOL and er <= EM_TOL and et <= EM_TOL
    # the M-step
    want = R["mix_out"]
    assert out.dtype == np.float32 and np.all(np.isfinite(out))
    assert np.all(out[dead] == 0) and np.all(out[:, 1:8] == 0)
    Ls = out[:, 32:].reshape(8, 24, 24)
    assert np.all(Ls[:, np.triu_indices(24, 1)[0], np.triu_indices(24, 1)[1]] == 0)
    def rel32(got, ref):                                  # relative; a zero is met exactly
        nz = ref != 0
        assert np.all(got[~nz] == 0)
        return float((np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])).max()) if nz.any() else 0.0
    ew, eb = rel32(out[slots, 0], want[slots, 0]), rel32(out[slots, 8:32], want[slots, 8:32])
    print(f"case {name}: new w err {ew:.3g}, new b err {eb:.3g}")
    assert ew <= 1e-6 and eb <= 1e-6
    ratios = {"moments": em / EM_TOL, "resp": er / EM_TOL, "total": et / EM_TOL, "new w": ew / 1e-6,
              "new b": eb / 1e-6, "factor": 0.0}
    for m in slots:
        f64 = Ls[m].astype(np.float64)
        assert np.all(np.diag(f64) > 0)
        if R["C"][m] is None:                             # N_m < 1: the component stays
            np.testing.assert_array_equal(out[m, 8:], want[m, 8:])
            continue
        e = np.abs(f64 @ f64.T - R["C"][m]).max() / np.abs(R["C"][m]).max()
        print(f"case {name} slot {m}: N {rs[m, 0]:.4g}, |L L^T - C| / max|C| {e:.3g}")
        assert e <= 1e-4
        ratios["factor"] = max(ratios["factor"], e / 1e-4)
    return ratios


def _kept(name, out, blk, m):
    """Slot m of ``out`` is what the "too little mass" branch writes for slot m
    of the input block ``blk``: b and the lower triangle bit for bit, zeros in
    floats 1..7 and above the diagonal, where the input holds NaN."""
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)
    lo, up = np.tril_indices(24), np.triu_indices(24, 1)
    Li, Lo = blk[m, 32:].reshape(24, 24), out[m, 32:].reshape(24, 24)
    assert np.all(np.isnan(blk[m, 1:8])) and np.all(np.isnan(Li[up])), (name, m, "the input's NaN")
    assert np.array_equal(bits(out[m, 8:32]), bits(blk[m, 8:32])), (name, m, "b")
    assert np.array_equal(bits(Lo[lo]), bits(Li[lo])), (name, m, "lower triangle")
    assert np.all(bits(Lo[up]) == 0) and np.all(bits(out[m, 1:8]) == 0), (name, m, "zeros")


@pytest.mark.parametrize("i", range(len(EM_CASES)), ids=EM_IDS)
def test_em_step_matches_checker(gpu, i):
    import time
    t0 = time.perf_counter()
    h, st = _em_result(i, gpu)
    if i == CAP:
        print(f"case cap: em_step took {1e3 * (time.perf_counter() - t0):.1f} ms (inputs to the device included)")
    out = h.params.cpu().numpy()
    _check_em_step(EM_IDS[i], st.moments.cpu().numpy(), st.resp.cpu().numpy(), st.total.cpu().numpy(), out,
                   _em_reference(i), list(EM_CASES[i][6]))
    if i != STARVED:
        return
    # the "too little mass" branch: the twin (0 < N < 0.5) and the far slot (N = 0)
    c, R = _em_inputs(i), _em_reference(i)
    rs = st.resp.cpu().numpy()
    assert 0.0 < rs[TWIN, 0] < 0.5 and rs[FAR, 0] == 0.0 and np.all(st.moments.cpu().numpy()[FAR] == 0)
    for m in (TWIN, FAR):
        _kept("starved", out, c["mix"], m)
    assert out[TWIN, 0].view(np.int32) == R["mix_out"][TWIN, 0].view(np.int32) and out[TWIN, 0] > 0
    assert out[FAR, 0].view(np.int32) == 0                  # + 0.0: dead from now on
    # a second step from the device's block (a head of its own: the cached one
    # stays at the first step's block): the far slot is dead
    c_dev = {k: _t(c[k], gpu) for k in ("pred", "targets", "n_active", "n_frames", "ped_mask")}
    h2 = _mix(out, gpu)
    assert torch.equal(h2.params, h.params)
    st2 = h2.em_step(c_dev["pred"], c_dev["targets"], c_dev["n_active"], n_frames=c_dev["n_frames"],
                    ped_mask=c_dev["ped_mask"])
    torch.cuda.synchronize()
    R2 = mr.em_step(_residuals(c), out)
    N2 = R2["resp"][:, 0]
    live2 = sorted(ORDINARY + (TWIN,))
    assert not np.any((N2[live2] >= 0.5) & (N2[live2] <= 2.0))
    out2, mo2, rs2 = h2.params.cpu().numpy(), st2.moments.cpu().numpy(), st2.resp.cpu().numpy()
    _check_em_step("starved, second step", mo2, rs2, st2.total.cpu().numpy(), out2, R2, live2)
    assert np.all(out2[FAR].view(np.int32) == 0) and np.all(mo2[FAR] == 0) and np.all(rs2[FAR] == 0)


@pytest.mark.parametrize("i", [1, 4], ids=[EM_IDS[1], EM_IDS[4]])
def test_e_step_alone_and_repeats_are_bit_identical(gpu, i):
    h, st = _em_result(i, gpu)
    c = _em_inputs(i)
    h2, st2 = _em_run(i, gpu)
    h0, st0 = _em_run(i, gpu, update=False)
    for a in (st2, st0):
        assert torch.equal(a.moments.view(torch.int64), st.moments.view(torch.int64))
        assert torch.equal(a.resp.view(torch.int64), st.resp.view(torch.int64))
        assert torch.equal(a.total.view(torch.int64), st.total.view(torch.int64))
    assert torch.equal(h2.params, h.params)
    assert torch.equal(h0.params.view(torch.int32), _t(c["mix"], gpu).view(torch.int32))
    R = _em_reference(i)
    n = R["total"][0]
    assert abs(st0.nll + R["total"][1] / n) <= EM_TOL * max(1.0, abs(st0.nll)) * 10
    np.testing.assert_array_equal(st0.usage, R["resp"][:, 1] / n)
    np.testing.assert_allclose(st0.resp_mass, R["resp"][:, 0] / n, rtol=0, atol=1e-12)
    assert st0.pairs == n


@pytest.mark.parametrize("i", [1, 4, 5, OUTLIERS, STARVED], ids=[EM_IDS[k] for k in (1, 4, 5, OUTLIERS, STARVED)])
def test_em_write_footprint(gpu, i):
    """The raw ABI call into guarded, poisoned outputs: every element written,
    no store outside; mix_out = NULL leaves no footprint and the same bits."""
    from multimodaltraj_2_amd import mixture
    lib = mixture.load()
    c = _em_inputs(i)
    S, F, N = EM_CASES[i][:3]
    d = _lib.G2KDims(S, F, 8, 12, 16, 64, N, 8, _lib.STEP_TARGETS_SHARED if c["shared"] else 0)
    need = int(lib.g2k_mix_em_workspace_bytes(ctypes.byref(d)))
    keep = [_t(c[k], gpu) for k in ("pred", "targets", "n_active", "n_frames", "ped_mask", "mix")]
    p = lambda t: None if t is None else t.data_ptr()

    def run(with_out):
        ar = Arena(gpu)
        mo = ar.alloc((8, 25, 24), torch.float64, "moments")
        rs = ar.alloc((8, 2), torch.float64, "resp")
        tt = ar.alloc(4, torch.float64, "total")
        out = ar.alloc((8, 608), torch.float32, "mix_out")
        ws = ar.alloc(need, torch.uint8, "workspace")
        rc = lib.g2k_mix_em_f32(ctypes.byref(d), *(p(t) for t in keep), p(mo), p(rs), p(tt),
                                p(out) if with_out else None, p(ws), need, None)
        torch.cuda.synchronize()
        assert rc == 0, lib.g2k_last_error()
        ar.check_guards()
        return mo, rs, tt, out
    mo, rs, tt, out = run(True)
    for t in (mo, rs, tt, out):
        assert all_written(t)
    h, st = _em_result(i, gpu)
    assert torch.equal(mo.view(torch.int64), st.moments.view(torch.int64))
    assert torch.equal(rs.view(torch.int64), st.resp.view(torch.int64))
    assert torch.equal(tt.view(torch.int64), st.total.view(torch.int64))
    assert torch.equal(out, h.params)
    mo0, rs0, tt0, out0 = run(False)
    assert not all_written(out0) and bool((out0.view(torch.int32) == 0x7FC0BEEF).all())
    assert torch.equal(mo0.view(torch.int64), mo.view(torch.int64))
    assert torch.equal(rs0.view(torch.int64), rs.view(torch.int64))
    assert torch.equal(tt0.view(torch.int64), tt.view(torch.int64))


@pytest.mark.parametrize("with_out", [True, False], ids=["mix_out", "e-step-only"])
def test_em_without_a_pair(gpu, with_out):
    """n_active all 0 (MixtureHead.fit raises before it launches, so through
    the raw ABI), pred and targets all NaN: total = {0, 0, 0, 0}, moments and
    resp zeros with every element written; in mix_out every live slot keeps
    its w bits, b and lower triangle (zeros in floats 1..7 and above the
    diagonal, where the input holds NaN) and the dead slots are zeros."""
    from multimodaltraj_2_amd import mixture
    lib = mixture.load()
    S, F, N = 2, 3, 5
    mix = _block(np.random.default_rng(950), ORDINARY)
    d = _lib.G2KDims(S, F, 8, 12, 16, 64, N, 8, 0)
    need = int(lib.g2k_mix_em_workspace_bytes(ctypes.byref(d)))
    ar = Arena(gpu)
    pred = ar.put(np.full((S, F, 24, N), np.nan, np.float32), "pred")
    tg = ar.put(np.full((S, F, N, 12, 2), np.nan, np.float32), "targets")
    nact, nfr = ar.put(np.zeros(S, np.int32), "n_active"), ar.put(np.full(S, F, np.int32), "n_frames")
    pm, blk = ar.put(np.ones((S, N), np.uint8), "ped_mask"), ar.put(mix, "mix_in")
    mo = ar.alloc((8, 25, 24), torch.float64, "moments")
    rs = ar.alloc((8, 2), torch.float64, "resp")
    tt = ar.alloc(4, torch.float64, "total")
    out = ar.alloc((8, 608), torch.float32, "mix_out")
    ws = ar.alloc(need, torch.uint8, "workspace")
    p = lambda t: t.data_ptr()
    rc = lib.g2k_mix_em_f32(ctypes.byref(d), p(pred), p(tg), p(nact), p(nfr), p(pm), p(blk), p(mo), p(rs),
                            p(tt), p(out) if with_out else None, p(ws), need, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.g2k_last_error()
    ar.check_guards()
    assert np.array_equal(blk.cpu().numpy().view(np.int32), mix.view(np.int32))       # the input block: read only
    for t in (mo, rs, tt):
        assert all_written(t) and bool((t.view(torch.int64) == 0).all())               # + 0.0, every element
    if not with_out:
        assert bool((out.view(torch.int32) == 0x7FC0BEEF).all())
        return
    assert all_written(out)
    o = out.cpu().numpy()
    R = mr.em_step(np.zeros((0, 24)), mix)
    dead = [m for m in range(8) if m not in ORDINARY]
    assert np.all(o[dead].view(np.int32) == 0)
    for m in ORDINARY:
        assert o[m, 0].view(np.int32) == mix[m, 0].view(np.int32)
        _kept("no-pairs", o, mix, m)
    assert np.array_equal(o.view(np.int32), R["mix_out"].view(np.int32))               # the checker's block, too


@pytest.mark.parametrize("i", [4], ids=[EM_IDS[4]])
def test_fit_is_em_steps_and_its_trace_the_checkers(gpu, i):
    c = _em_inputs(i)
    args = (_t(c["pred"], gpu), _t(c["targets"], gpu), _t(c["n_active"], gpu))
    kw = dict(n_frames=_t(c["n_frames"], gpu), ped_mask=_t(c["ped_mask"], gpu), targets_shared=c["shared"])
    a = _mix(c["mix"], gpu)
    f = a.fit(*args, iters=5, init=a, **kw)
    b = _mix(c["mix"], gpu)
    r = fr.residuals(c["pred"], c["targets"], c["n_active"], c["n_frames"], c["ped_mask"])
    trace, same_block, st = [], [], None
    for _ in range(5):
        blk = b.params.cpu().numpy()
        st = b.em_step(*args, **kw)
        trace.append(st.loglik)
        e = mr.em_step(r, blk)                            # the checker on the device's block
        same_block.append(e["total"][1] / e["total"][0])
    assert torch.equal(a.params, b.params)
    np.testing.assert_array_equal(f.loglik, np.array(trace))
    assert torch.equal(f.resp.view(torch.int64), st.resp.view(torch.int64)) and f.pairs == c["pairs"]
    assert f.gain == trace[-1] - trace[0]
    free, blk = [], c["mix"]
    for _ in range(5):
        e = mr.em_step(r, blk)
        free.append(e["total"][1] / e["total"][0])
        blk = e["mix_out"]
    rel = lambda x, y: float(np.max(np.abs(np.array(x) - np.array(y)) / np.maximum(1.0, np.abs(y))))
    print(f"fit trace {np.array(trace)}; vs the checker on the same blocks {rel(trace, same_block):.3g}, "
          f"vs the checker's own five steps {rel(trace, free):.3g}; smallest step "
          f"{np.diff(trace).min():.3g}")
    assert rel(trace, same_block) <= EM_TOL
    assert rel(trace, free) <= EM_TOL
    assert np.diff(trace).min() >= -1e-4
    # init=None: the deterministic start of a no-head full-covariance launch
    from multimodaltraj_2_amd.fullcov import FullCovHead
    from multimodaltraj_2_amd.mixture import MixtureHead
    g = MixtureHead(components=2, device=gpu)
    fg = g.fit(*args, iters=3, **kw)
    st0 = FullCovHead(device=gpu).stats(*args, (), use_head=False, **kw)
    start = MixtureHead.init_from(st0, 2)
    np.testing.assert_array_equal(start.params.cpu().numpy()[:, 0], mr.init_from(st0.cov, st0.fit_chol.cpu().numpy(), 2)[:, 0])
    g2 = MixtureHead(components=2, device=gpu)
    fg2 = g2.fit(*args, iters=3, init=start, **kw)
    assert torch.equal(g.params, g2.params) and np.array_equal(fg.loglik, fg2.loglik)
    assert g.components == 2 and np.diff(fg.loglik).min() >= -1e-4
    with pytest.raises(ValueError, match="no .* pair"):
        g.fit(args[0], args[1], torch.zeros(4, dtype=torch.int32, device=gpu), iters=2, **kw)


# ---------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------
def _sampler_block():
    rng = np.random.default_rng(77)
    p = _block(rng, (0, 1, 2), scale=0.3)
    p[:3, 0] = (0.5, 0.3, 0.2)
    return p


@pytest.mark.parametrize("seed", [SEED, (1 << 64) - 1], ids=["seed", "wrap"])
def test_sample_matches_checker_and_meets_the_weights(gpu, seed):
    """S 4 x F 8 x Nmax 33 = 1056 trajectories, weights (0.5, 0.3, 0.2): each
    count within 5 sqrt(n w (1 - w)) of n w (a binomial bound)."""
    mix = _sampler_block()
    pred = np.random.default_rng(5).standard_normal((4, 8, 24, 33)).astype(np.float32)
    x, comp = _mix(mix, gpu).sample(_t(pred, gpu), seed=seed, want_components=True)
    ref, rcomp = mr.sample(pred, mix, seed)
    assert comp.dtype == torch.int32 and tuple(comp.shape) == (4, 8, 33)
    np.testing.assert_array_equal(comp.cpu().numpy(), rcomp)
    err = close(x.cpu().numpy(), ref)
    cnt = np.bincount(rcomp.reshape(-1), minlength=8)
    print(f"sample err {err:.3g}; component counts {cnt[:3]} of 1056")
    assert err <= TOL and cnt[3:].sum() == 0
    for m, w in enumerate((0.5, 0.3, 0.2)):
        assert abs(cnt[m] - 1056 * w) <= 5 * np.sqrt(1056 * w * (1 - w))
    again = _mix(mix, gpu).sample(_t(pred, gpu), seed=seed)
    assert torch.equal(again, x)


# the selector's edges: (live slots, their weights)
SELECTOR_EDGES = {"equal-cw": ((2, 4, 6), (1.0, 1e-9, 1.0)),      # slot 4's f32 cw equals slot 2's
                  "first-live-not-0": ((1, 5), (1.0, 1e-9)),      # the last live slot's cw is forced to 1
                  "one-at-7": ((7,), (0.7,))}
SELECTOR_SHAPE = (4, 8, 24, 33)


def _selector_block(name):
    slots, w = SELECTOR_EDGES[name]
    p = _block(np.random.default_rng(80 + len(slots)), slots, scale=0.3)
    p[list(slots), 0] = w
    return p


def selector_edge_preconditions():
    """On tests/mixture_ref.py alone: what each block of SELECTOR_EDGES is for.
    {name: the components the checker selects at SEED and at the wrapping seed}."""
    found = {}
    for name, (slots, w) in SELECTOR_EDGES.items():
        mix = _selector_block(name)
        cw = mr.cum_weights(mix)
        assert cw.dtype == np.float32 and cw[slots[-1]] == 1.0
        found[name] = set()
        for seed in (SEED, (1 << 64) - 1):
            found[name] |= set(np.unique(mr.components(SELECTOR_SHAPE, mix, seed)).tolist())
    cw = mr.cum_weights(_selector_block("equal-cw"))
    assert cw[4] == cw[2] == np.float32(0.5) and cw[3] == cw[2]      # 0.5 + 5e-10 rounds to 0.5 in f32
    assert found["equal-cw"] == {2, 6}                               # slot 4 is live and never selected
    # slots {1, 5}: cw[1] = f32(1 / (1 + 1e-9)) = 1 exactly, and u <= 1 - 2^-25
    # < 1 for every h (u = 1 only as the rounding of h = 2^24 - 1, which 1056
    # trajectories do not draw), so by the definition slot 5 is selected
    # exactly where u >= cw[1]: nowhere at this size.  The checker says so.
    cw = mr.cum_weights(_selector_block("first-live-not-0"))
    assert cw[0] == 0.0 and cw[1] == 1.0 and cw[5] == 1.0
    u = np.stack([mr.selector_u(SELECTOR_SHAPE, seed) for seed in (SEED, (1 << 64) - 1)])
    assert u.max() < cw[1] and found["first-live-not-0"] == {1}
    assert found["one-at-7"] == {7}
    return found


@pytest.mark.parametrize("name", list(SELECTOR_EDGES))
def test_sample_selector_edges(gpu, name):
    """S 4 x F 8 x Nmax 33 with the blocks of SELECTOR_EDGES: ``comp`` is the
    checker's exactly (mr.components restates the f32 casts of u and cw), the
    draws within TOL; every block holds NaN wherever nothing is read, so finite
    draws prove that no dead slot was touched.  In "first-live-not-0" the
    definition selects slot 5 exactly where u >= cw[1] = 1, which happens for
    no trajectory here (selector_edge_preconditions): every comp is 1."""
    found = selector_edge_preconditions()[name]
    mix = _selector_block(name)
    pred = np.random.default_rng(6).standard_normal(SELECTOR_SHAPE).astype(np.float32)
    for seed in (SEED, (1 << 64) - 1):
        x, comp = _mix(mix, gpu).sample(_t(pred, gpu), seed=seed, want_components=True)
        ref, rcomp = mr.sample(pred, mix, seed)
        got = comp.cpu().numpy()
        np.testing.assert_array_equal(got, rcomp)
        assert set(np.unique(got).tolist()) <= found
        xs = x.cpu().numpy()
        err = close(xs, ref)
        print(f"selector {name} seed {seed:#x}: components {np.bincount(got.reshape(-1), minlength=8)}, "
              f"sample err {err:.3g}")
        assert np.all(np.isfinite(xs)) and err <= TOL


def test_one_slot_mixture_is_the_full_covariance_head(gpu):
    """b = 0, one live slot: the sampler's and best-of-K's bits are FullCovHead's."""
    from multimodaltraj_2_amd.fullcov import FullCovHead
    from multimodaltraj_2_amd.mixture import MixtureHead
    c = _bk_inputs(0)
    rng = np.random.default_rng(3)
    fc = FullCovHead(device=gpu)
    fc.chol = _t(np.tril(_factor(rng, 0.3)).astype(np.float32), gpu)
    mx = MixtureHead.from_fullcov(fc)
    assert mx.components == 1 and mx.params.device == fc.chol.device
    pred = _t(c["pred"], gpu)
    for seed in (0, SEED, (1 << 64) - 1):
        a, comp = mx.sample(pred, seed=seed, want_components=True)
        assert np.array_equal(a.cpu().numpy(), fc.sample(pred, seed=seed).cpu().numpy())
        assert not bool(comp.any())
    args = (pred, _t(c["targets"], gpu), _t(c["n_active"], gpu), c["K"])
    kw = dict(seed=c["seed"], n_frames=_t(c["n_frames"], gpu), ped_mask=_t(c["ped_mask"], gpu),
              want_best=True)
    ra, rb = mx.best_of_k(*args, **kw), fc.best_of_k(*args, **kw)
    assert torch.equal(ra.sums, rb.sums) and torch.equal(ra.per_ped, rb.per_ped)
    assert torch.equal(ra.best, rb.best) and ra.pairs > 0


# ---------------------------------------------------------------------------
# best-of-K
# ---------------------------------------------------------------------------
#           S  F   Nmax K   n_active              n_frames          mask   shared seed   geometry (ks, fc, c)
BK_CASES = [(2, 20, 32, 20, [32, 21], [20, 13], True, False, SEED, (16, 1, 20)),
            (5, 3, 20, 20, [0, 1, 13, 20, 7], [3, 0, 2, 3, 1], True, False, SEED, None),
            (2, 2, 256, 1, [256, 37], None, False, True, (1 << 64) - 2, (1, 1, 2))]
BK_IDS = ["ks16-c20", "mask-empty", "n256-k1-shared"]


@functools.lru_cache(maxsize=None)
def _bk_inputs(i):
    S, F, N, K, nact, nfr, masked, shared, seed, _ = BK_CASES[i]
    rng = np.random.default_rng(300 + i)
    pred = rng.standard_normal((S, F, 24, N)).astype(np.float32)
    Ft = 1 if shared else F
    base = pred[:, :Ft].reshape(S, Ft, 2, 12, N).transpose(0, 1, 4, 3, 2)
    tg = (base + 0.9 * rng.standard_normal((S, Ft, N, 12, 2))).astype(np.float32)
    pm = (rng.random((S, N)) > 0.2).astype(np.uint8) if masked else None
    mix = _block(rng, (0, 3, 4), scale=0.3)
    mix[(0, 3, 4), 0] = (0.4, 0.35, 0.25)
    return dict(pred=pred, targets=np.ascontiguousarray(tg), mix=mix, n_active=np.array(nact, np.int32),
                n_frames=None if nfr is None else np.array(nfr, np.int32), ped_mask=pm, K=K,
                seed=seed, shared=shared)


@functools.lru_cache(maxsize=None)
def _bk_reference(i):
    c = _bk_inputs(i)
    return mr.best_of_k_ref(c["pred"], c["targets"], c["n_active"], c["mix"], c["seed"], c["K"],
                            c["n_frames"], c["ped_mask"])


def _bk_run(i, dev):
    c = _bk_inputs(i)
    h = _mix(c["mix"], dev)
    pred = _t(c["pred"], dev)
    r = h.best_of_k(pred, _t(c["targets"], dev), _t(c["n_active"], dev), c["K"], seed=c["seed"],
                    n_frames=_t(c["n_frames"], dev), ped_mask=_t(c["ped_mask"], dev),
                    targets_shared=c["shared"], want_best=True)
    torch.cuda.synchronize()
    return h, pred, r


_BK = {}


def _bk_result(i, dev):
    if i not in _BK:
        _BK[i] = _bk_run(i, dev)
    return _BK[i]


def test_best_of_k_cases_reach_the_geometries():
    """By g2k_best_of_k_geometry: a case with a pair's draws on KS >= 4 lanes
    and C > 1 workgroups per scene, one with KS = 1 (adjacent lanes are
    adjacent pedestrians); a mask and an empty scene; and adjacent lanes hold
    different components (the checker's ``comp``: of adjacent draws k of a
    pair when KS > 1, of adjacent pedestrians when KS = 1)."""
    from multimodaltraj_2_amd.nll import best_of_k_geometry
    geo = [best_of_k_geometry(*c[:4]) for c in BK_CASES]
    print("best-of-K geometries:", geo)
    assert (geo[0]["ks"], geo[0]["fc"], geo[0]["c"]) == BK_CASES[0][9]
    assert geo[0]["ks"] >= 4 and geo[0]["c"] > 1
    assert (geo[2]["ks"], geo[2]["fc"], geo[2]["c"]) == BK_CASES[2][9]
    assert BK_CASES[1][4][0] == 0 and _bk_inputs(1)["ped_mask"] is not None
    for i, g in enumerate(geo):
        c = _bk_inputs(i)
        m = _bk_reference(i)["pairs"]
        c0 = mr.components(c["pred"].shape, c["mix"], c["seed"])
        assert set(np.unique(c0)) == {0, 3, 4}
        if g["ks"] > 1:
            c1 = mr.components(c["pred"].shape, c["mix"], (c["seed"] + 1) & MASK64)
            differ = (c0 != c1)[m].mean()
        else:
            both = m[..., 1:] & m[..., :-1]
            differ = (c0[..., 1:] != c0[..., :-1])[both].mean()
        assert differ > 0.5, (BK_IDS[i], differ)


@pytest.mark.parametrize("i", range(len(BK_CASES)), ids=BK_IDS)
def test_best_of_k_values_match_checker(gpu, i):
    _, pred, r = _bk_result(i, gpu)
    R = _bk_reference(i)
    per, out = r.per_ped.cpu().numpy(), r.sums.cpu().numpy()
    m = R["pairs"]
    print(f"case {BK_IDS[i]}: pairs {int(m.sum())}, per_ped err {close(per[..., :2], R['per_ped'][..., :2]):.3g}, "
          f"sums err {close(out[:, :5], R['out'][:, :5]):.3g}")
    assert np.all(np.isfinite(per)) and np.all(np.isfinite(out))       # the block's NaN: not read
    assert close(per[..., :2], R["per_ped"][..., :2]) <= TOL
    assert close(out[:, :5], R["out"][:, :5]) <= TOL
    np.testing.assert_array_equal(out[:, 2], R["out"][:, 2])
    np.testing.assert_array_equal(out[:, 5], R["out"][:, 5])
    assert np.all(out[:, 6:] == 0)
    assert np.all(per[~m] == 0)
    off = ~torch.from_numpy(m).to(gpu)[:, :, None, :].expand_as(pred)
    assert torch.equal(r.best[off], pred[off])


@pytest.mark.parametrize("i", range(len(BK_CASES)), ids=BK_IDS)
def test_best_of_k_indices_attain_the_minimum(gpu, i):
    _, _, r = _bk_result(i, gpu)
    R = _bk_reference(i)
    K = BK_CASES[i][3]
    per = r.per_ped.cpu().numpy().astype(np.float64)
    m = R["pairs"]
    for col, errs in ((2, R["ade_k"]), (3, R["fde_k"])):
        k = per[..., col][m]
        assert np.all(k == np.round(k)) and np.all((k >= 0) & (k < K))
        at = np.take_along_axis(errs, per[..., col].astype(np.int64)[None], axis=0)[0][m]
        best = errs.min(axis=0)[m]
        worst = float((np.abs(at - best) / np.maximum(1.0, np.abs(best))).max()) if at.size else 0.0
        print(f"case {BK_IDS[i]} col {col}: {at.size} pairs, checker error at the kernel's index vs "
              f"checker minimum: {worst:.3g}")
        assert worst <= TOL


@pytest.mark.parametrize("i", range(len(BK_CASES)), ids=BK_IDS)
def test_best_is_the_unfused_draw_exactly(gpu, i):
    h, pred, r = _bk_result(i, gpu)
    c = _bk_inputs(i)
    pairs = torch.from_numpy(_bk_reference(i)["pairs"]).to(gpu)
    kA = r.per_ped[..., 2]
    want = pred.clone()
    for k in range(c["K"]):
        sel = pairs & (kA == k)
        if bool(sel.any()):
            xk = h.sample(pred, seed=(c["seed"] + k) & MASK64)
            want = torch.where(sel[:, :, None, :], xk, want)
    assert torch.equal(r.best, want)
    assert not torch.equal(r.best, pred)


@pytest.mark.parametrize("i", [0, 1], ids=[BK_IDS[0], BK_IDS[1]])
def test_best_of_k_repeated_calls_are_bit_identical(gpu, i):
    a, b = _bk_result(i, gpu)[2], _bk_run(i, gpu)[2]
    assert torch.equal(a.sums, b.sums) and torch.equal(a.per_ped, b.per_ped)
    assert torch.equal(a.best, b.best)


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def test_evaluation_end_to_end(gpu, tmp_path, data_root):
    """The recipe of tests/test_fullcov_gpu.py::test_evaluation_end_to_end with
    --fit_head eval --fullcov_head eval --mixture_head eval (in-sample).  One
    component: a centred Gaussian is at least as likely in-sample as the
    uncentred one, so mix_nll <= fullcov_nll + 1e-3 (that test's ridge
    allowance).  Three components: EM loses no more than 1e-4 over the fit and
    ends no worse than one component (+ 1e-3).  With the flag off the result
    has no mix_* key."""
    from multimodaltraj_2_amd import checkpoint, evaluate
    from multimodaltraj_2_amd import train as tr
    from multimodaltraj_2_amd.argParser import ArgsParser
    argv = ["--data_root", data_root, "--leaveDataset", "2", "--n_max", "32", "--train_scenes", "64",
            "--train_batch", "32", "--num_epochs", "2", "--loss", "l2", "--num_samples", "4",
            "--mode", "train", "--save_dir", str(tmp_path), "--log_dir", str(tmp_path),
            "--device", "cuda:0"]
    args = ArgsParser().parser.parse_args(argv)
    assert (args.mixture_head, args.mixture_components, args.mixture_iters) == ("off", 3, 30)
    tr.run_train_mode(args, gpu, log=lambda s: None)
    prm = checkpoint.load_params(checkpoint.read_state(str(tmp_path)), device=gpu)
    args.fit_head, args.fullcov_head = "eval", "eval"
    logs0, keep0 = [], {}
    res0 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs0.append, keep=keep0)
    assert not any(k.startswith("mix_") for k in res0) and "mixture" not in keep0
    assert not any("mixture head" in s for s in logs0)

    args.mixture_head, args.mixture_components = "eval", 1
    logs1, keep1 = [], {}
    res1 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs1.append, keep=keep1)
    assert list(res1) == list(res0) + list(evaluate.MIX_FIGURES)
    assert {k: res1[k] for k in res0} == res0
    assert logs1[:len(logs0)] == logs0 and len(logs1) == len(logs0) + 1
    assert logs1[-1].startswith("mixture head on dataset 2") and "in-sample" in logs1[-1]
    assert sorted(set(keep1) - set(keep0)) == ["mixture"]
    for k in evaluate.MIX_FIGURES:
        print(f"evaluation M = 1 {k}: {res1[k]:.8g}")
        assert np.isfinite(res1[k]), k
    assert res1["mix_components"] == 1 and res1["mix_weight_max"] == 1.0
    print(f"in-sample NLL per pair ({res1['pairs']} pairs): mixture of one {res1['mix_nll']:.8g}, "
          f"full covariance {res1['fullcov_nll']:.8g}")
    assert res1["mix_nll"] <= res1["fullcov_nll"] + 1e-3
    # the figures are a direct call's on keep's tensors
    mx = keep1["mixture"]["head"]
    t = keep1["plan"].to_device(gpu, F=1)
    one = torch.ones(keep1["plan"].S, dtype=torch.int32, device=gpu)
    st = mx.stats(keep1["pred"], t["targets"], t["n_active"], n_frames=one, ped_mask=t["ped_mask"])
    bk = mx.best_of_k(keep1["pred"], t["targets"], t["n_active"], 4, seed=args.sample_seed,
                      n_frames=one, ped_mask=t["ped_mask"], want_per_ped=False)
    assert (st.nll, bk.min_ade, bk.min_fde) == (res1["mix_nll"], res1["mix_min_ade"], res1["mix_min_fde"])
    assert bk.pairs == st.pairs == res1["pairs"]

    args.mixture_components = 3
    res3 = evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
    for k in evaluate.MIX_FIGURES:
        print(f"evaluation M = 3 {k}: {res3[k]:.8g}")
        assert np.isfinite(res3[k]), k
    assert 1 <= res3["mix_components"] <= 3 and 0 < res3["mix_weight_max"] <= 1.0
    assert res3["mix_loglik_gain"] >= -1e-4
    assert res3["mix_nll"] <= res1["mix_nll"] + 1e-3
    cli = evaluate.main(argv + ["--fit_head", "eval", "--fullcov_head", "eval", "--mixture_head", "eval"],
                        log=lambda s: None)
    assert [cli[k] for k in evaluate.MIX_FIGURES] == [res3[k] for k in evaluate.MIX_FIGURES]
