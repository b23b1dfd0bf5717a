"""GPU: the Gaussian-mixture head's fused joint best-of-K and KDE-NLL
(g2k_mix_joint_eval_f32, g2k_mix_kde_nll_f32: joint_kernel<MixHead>,
joint_wave_kernel<MixHead>, kde_nll_kernel<MixHead>; MixtureHead.joint_eval /
kde_nll; evaluate.py --mixture_head with --collision_radius / --kde_nll)
against the float64 checkers of tests/mix_eval_ref.py and the device's own
draws.  PARITY UNPINNED: the reference has no probabilistic head.

Joint: the runs, rules and tolerances of tests/test_fullcov_joint_gpu.py (its
eight shapes and the structured couples case, the same pred / targets / mask
construction, seeds and radii) with the mixture mix_block(sigma, rs) of three
live slots {0, 2, 5}, plus the n256 case with all 8 slots live (every component
in one wave of the four-wave kernel, which holds 69.7 KB of static LDS: these
runs are what shows that it launches).  Floats close(got, ref) <= 1e-4; the
checker's value at the kernel's index within tolerance of the checker's
minimum; counts inside the checker's bracket at radius -/+ 1e-4 (the cap on the
bracket is asserted on the checker alone, tests/test_mix_eval.py too); the
device's own MixtureHead.sample draws recounted in float64 at radius (1 -/+
1e-6) bracket the kernel's counts.

KDE: the eight tests/kde_cases.py inputs, each with a "near" (b = 1.5 N(0, 1))
and a "far" (b = 10 N(0, 1)) mixture, against the float64 checker fed with the
device's own draws.  Gate mix_eval_ref.GATE, absolute: 8 x the worst
|restated - float64| of this head's moment scheme (running mean and centred
sums) over these inputs, measured on the CPU (tests/test_mix_eval.py::
test_kde_gate_measurement).  That scheme is not the other heads', so the
one-slot b = 0 block agrees with FullCovHead.kde_nll within the gate
(mix_eval_ref.GATE), not bit for bit; the joint evaluation of that block IS
FullCovHead.joint_eval's bit for bit (the draws are).

Measured on an MI355X: joint per_frame within 1.8e-7 and sums within 5.5e-7 of
the checker, every index attaining the checker's minimum exactly; KDE worst
|kernel - float64| of a pair 9.3e-5 (case k4, near block; far block 5.4e-5)
against the gate 1.52e-3, every clip count exact; the one-slot block within
1.3e-5 of FullCovHead.kde_nll."""
import functools

import numpy as np
import pytest
import torch

from tests import kde_cases as kc
from tests import mix_eval_ref as me
from tests import test_fullcov_joint_gpu as tj
from tests.bestk_ref import MASK64, draw_errors
from tests.conftest import close

pytestmark = pytest.mark.gpu
TOL, REL = tj.TOL, tj.REL
FLOOR = -20.0
RUNS, RUN_IDS = me.joint_runs()
POSITIVE = [(r, n) for r, n in zip(RUNS, RUN_IDS) if r[1] > 0]
N256 = tj.IDS.index("n256")
_t, _between, _host = tj._t, tj._between, tj._host


def _mx(block, dev):
    from multimodaltraj_2_amd.mixture import MixtureHead
    return MixtureHead.from_block(block, device=dev)


@functools.lru_cache(maxsize=None)
def _reference(i, radius, slots):
    R, c = me.joint_reference(i, radius, slots), me.joint_inputs(i, slots)
    tj.assert_cap(int(R["amb_k"].sum()), c["K"] * int(R["per_frame_i"][..., 1].sum()),
                  int(R["col_k"].sum()), f"checker, case {i} radius {radius} slots {slots}")
    return R


def _run(i, radius, dev, slots=me.SLOTS3, K=None, head=None, **over):
    c = me.joint_inputs(i, slots)
    a, kw = tj._args(c, dev)
    kw.update(over)
    r = (head or _mx(c["mix"], dev)).joint_eval(*a, K or c["K"], radius, seed=c["seed"], **kw)
    torch.cuda.synchronize()
    return r


_CACHE = {}


def _gpu_result(i, radius, dev, slots=me.SLOTS3):
    if (i, radius, slots) not in _CACHE:
        _CACHE[i, radius, slots] = _run(i, radius, dev, slots)
    return _CACHE[i, radius, slots]


# ---------------------------------------------------------------------------
# joint
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("i,radius,slots", RUNS, ids=RUN_IDS)
def test_joint_values_match_checker(gpu, i, radius, slots):
    R = _reference(i, radius, slots)
    pf, pi, sf, si = _host(_gpu_result(i, radius, gpu, slots))
    K = me.joint_inputs(i, slots)["K"]
    print(f"members {int(R['per_frame_i'][..., 0].sum())}, per_frame err "
          f"{close(pf[..., :2], R['per_frame_f'][..., :2]):.3g}, sums err "
          f"{close(sf[:, :2], R['sums_f'][:, :2]):.3g}")
    assert close(pf[..., :2], R["per_frame_f"][..., :2]) <= TOL
    assert close(sf[:, :2], R["sums_f"][:, :2]) <= TOL
    assert np.all(sf[:, 2] == K) and np.all(sf[:, 3] == 0)
    assert si.dtype == np.int64
    np.testing.assert_array_equal(pi[..., :2], R["per_frame_i"][..., :2])       # P, PP
    np.testing.assert_array_equal(si[:, :2], R["sums_i"][:, :2])
    off = R["per_frame_i"][..., 0] == 0                    # no member: exactly zero, every column
    assert np.all(pf[off] == 0) and np.all(pi[off] == 0)
    np.testing.assert_array_equal(si, pi.sum(axis=1))      # the scene sums are the frames'
    if radius == 0:
        assert np.all(pi[..., 2:] == 0)
    # the checker's value at the kernel's index attains the checker's minimum
    on = R["per_frame_i"][..., 0] > 0
    for col, errs in ((2, R["jade_k"]), (3, R["jfde_k"])):
        k = pf[..., col][on]
        assert np.all(k == np.round(k)) and np.all((k >= 0) & (k < K))
        at = np.take_along_axis(errs, pf[..., col].astype(np.int64)[None], axis=0)[0][on]
        best = errs.min(axis=0)[on]
        worst = float((np.abs(at - best) / np.maximum(1.0, np.abs(best))).max()) if at.size else 0.0
        print(f"col {col}: checker error at the kernel's index vs checker minimum: {worst:.3g}")
        assert worst <= TOL


@pytest.mark.parametrize("i,radius,slots", RUNS, ids=RUN_IDS)
def test_joint_collision_counts_within_the_checkers_bracket(gpu, i, radius, slots):
    R = _reference(i, radius, slots)
    pf, pi, _, si = _host(_gpu_result(i, radius, gpu, slots))
    lo_k, hi_k = R["col_lo"].sum(axis=0), R["col_hi"].sum(axis=0)
    print(f"col_pred {pi[..., 2].sum()} in [{R['pred_lo'].sum()}, {R['pred_hi'].sum()}], col_gt "
          f"{pi[..., 3].sum()} in [{R['gt_lo'].sum()}, {R['gt_hi'].sum()}], sum col_k {pi[..., 4].sum()} "
          f"in [{lo_k.sum()}, {hi_k.sum()}], col_best {pi[..., 5].sum()}")
    for col, lo, hi in ((2, R["pred_lo"], R["pred_hi"]), (3, R["gt_lo"], R["gt_hi"]), (4, lo_k, hi_k)):
        assert _between(lo, pi[..., col], hi), col                     # per scene-frame
        assert _between(lo.sum(axis=1), si[:, col], hi.sum(axis=1)), col   # per scene
    kJA = pf[..., 2].astype(np.int64)                      # the KERNEL's index
    blo = np.take_along_axis(R["col_lo"], kJA[None], axis=0)[0]
    bhi = np.take_along_axis(R["col_hi"], kJA[None], axis=0)[0]
    on = R["per_frame_i"][..., 0] > 0
    assert _between(blo[on], pi[..., 5][on], bhi[on])
    assert _between((blo * on).sum(axis=1), si[:, 5], (bhi * on).sum(axis=1))
    if radius > 0 and i != tj.COUPLES:
        assert pi[..., 4].sum() > 0                        # there is something to count


@functools.lru_cache(maxsize=None)
def _device_draws(i, slots, dev):
    """[K, S, F, 24, N] f32: MixtureHead.sample at the seeds (seed + k) mod 2^64."""
    c = me.joint_inputs(i, slots)
    mx, pred = _mx(c["mix"], dev), _t(c["pred"], dev)
    return np.stack([mx.sample(pred, seed=(c["seed"] + k) & MASK64).cpu().numpy() for k in range(c["K"])])


@pytest.mark.parametrize("i,radius,slots", [r for r, _ in POSITIVE], ids=[n for _, n in POSITIVE])
def test_joint_counts_against_the_devices_own_draws(gpu, i, radius, slots):
    """The draws are the sampler's, bit for bit: the counts recounted in
    float64 from MixtureHead.sample's f32 coordinates at radius (1 -/+ 1e-6)
    bracket the kernel's, and JADE_k recomputed from them gives its minimum."""
    c = me.joint_inputs(i, slots)
    R = _reference(i, radius, slots)
    pf, pi, _, si = _host(_gpu_result(i, radius, gpu, slots))
    xs = _device_draws(i, slots, gpu)
    m = R["members"]
    lo, hi, amb = tj.fj.recount(xs, m, radius, REL)
    tj.assert_cap(int(amb.sum()), c["K"] * int(pi[..., 1].sum()), int(lo.sum()),
                  f"device draws, case {i} radius {radius}")
    print(f"sum col_k {pi[..., 4].sum()} in [{lo.sum()}, {hi.sum()}]")
    assert _between(lo.sum(axis=0), pi[..., 4], hi.sum(axis=0))
    assert _between(lo.sum(axis=(0, 2)), si[:, 4], hi.sum(axis=(0, 2)))
    kJA = pf[..., 2].astype(np.int64)
    on = pi[..., 0] > 0
    blo = np.take_along_axis(lo, kJA[None], axis=0)[0]
    bhi = np.take_along_axis(hi, kJA[None], axis=0)[0]
    assert _between(blo[on], pi[..., 5][on], bhi[on])
    Pd = np.maximum(m.sum(axis=2), 1)
    jade, jfde = np.empty(lo.shape), np.empty(lo.shape)
    for k in range(c["K"]):
        a, f = draw_errors(xs[k].astype(np.float64), c["targets"])
        jade[k], jfde[k] = (a * m).sum(axis=2) / Pd, (f * m).sum(axis=2) / Pd
    err = close(pf[..., 0], jade.min(axis=0) * on), close(pf[..., 1], jfde.min(axis=0) * on)
    print(f"minJADE / minJFDE vs the float64 recomputation from the device's draws: "
          f"{err[0]:.3g} / {err[1]:.3g}")
    assert max(err) <= TOL
    at = np.take_along_axis(jade, kJA[None], axis=0)[0]
    assert close(at * on, jade.min(axis=0) * on) <= TOL


@pytest.mark.parametrize("radius", [0.1, 0.3])
def test_joint_structured_couples_exactly(gpu, radius):
    _, intact = tj.couples_case()
    _, pi, _, si = _host(_gpu_result(tj.COUPLES, radius, gpu))
    np.testing.assert_array_equal(pi[..., 2], intact)
    np.testing.assert_array_equal(pi[..., 3], intact)
    np.testing.assert_array_equal(pi[..., 4], tj.K_COUPLES * intact)
    np.testing.assert_array_equal(pi[..., 5], intact)


@pytest.mark.parametrize("i", [0, 1, 5, tj.COUPLES], ids=[tj.IDS[0], tj.IDS[1], tj.IDS[5], "couples"])
def test_joint_head_independent_columns_are_the_per_step_kernels(gpu, i):
    a = _gpu_result(i, 0.3, gpu)
    b = tj._run(i, 0.3, gpu, head=tj._gh(tj._inputs(i), gpu))
    assert torch.equal(a.per_frame_i[..., :4], b.per_frame_i[..., :4])
    assert torch.equal(a.sums_i[:, :4], b.sums_i[:, :4])
    assert int(a.sums_i[:, 1].sum()) > 0


def _marginal(i, dev):
    c = me.joint_inputs(i)
    a, kw = tj._args(c, dev)
    r = _mx(c["mix"], dev).best_of_k(*a, c["K"], seed=c["seed"], **kw)
    torch.cuda.synchronize()
    return r.per_ped.cpu().numpy().astype(np.float64)


def test_joint_one_draw_is_the_marginal_kernels_sum(gpu):
    i = tj.IDS.index("k1")
    pf, pi, _, _ = _host(_gpu_result(i, 0.3, gpu))
    per = _marginal(i, gpu)
    for c in (0, 1):
        assert close(pi[..., 0] * pf[..., c], per[..., c].sum(axis=2)) <= TOL
    assert pi[..., 0].sum() > 0


def test_joint_is_not_below_marginal(gpu):
    pf, pi, _, _ = _host(_gpu_result(0, 0.3, gpu))
    per = _marginal(0, gpu)
    for c in (0, 1):
        marg = per[..., c].sum(axis=2)
        assert np.all(pi[..., 0] * pf[..., c] >= marg - TOL * np.maximum(1.0, marg))
    assert np.any(pi[..., 0] * pf[..., 0] > per[..., 0].sum(axis=2) + 1e-3)


def test_joint_nested_draws(gpu):
    """K' = 10 are the first ten draws of K = 20, dealt differently."""
    R = _reference(0, 0.3, me.SLOTS3)
    a, b = _run(0, 0.3, gpu, K=10), _gpu_result(0, 0.3, gpu)
    pf, pi, _, _ = _host(a)
    on = R["per_frame_i"][..., 0] > 0
    assert close(pf[..., 0], R["jade_k"][:10].min(axis=0) * on) <= TOL
    assert close(pf[..., 1], R["jfde_k"][:10].min(axis=0) * on) <= TOL
    assert _between(R["col_lo"][:10].sum(axis=0), pi[..., 4], R["col_hi"][:10].sum(axis=0))
    assert bool((b.per_frame_f[..., :2] <= a.per_frame_f[..., :2]).all())
    assert bool((b.per_frame_f[..., 0] < a.per_frame_f[..., 0]).any())
    assert bool((b.per_frame_i[..., 4] >= a.per_frame_i[..., 4]).all())
    assert torch.equal(b.per_frame_i[..., :4], a.per_frame_i[..., :4])


@pytest.mark.parametrize("i", [0, 1], ids=[tj.IDS[0], tj.IDS[1]])        # one wave per unit; four
def test_joint_repeated_calls_are_bit_identical(gpu, i):
    a, b = _gpu_result(i, 0.3, gpu), _run(i, 0.3, gpu)
    assert torch.equal(a.sums_f, b.sums_f) and torch.equal(a.sums_i, b.sums_i)
    assert torch.equal(a.per_frame_f, b.per_frame_f) and torch.equal(a.per_frame_i, b.per_frame_i)


def test_joint_outputs_may_be_omitted(gpu):
    r = _run(0, 0.3, gpu, want_per_frame=False)
    full = _gpu_result(0, 0.3, gpu)
    assert r.per_frame_f is None and r.per_frame_i is None
    assert torch.equal(r.sums_f, full.sums_f) and torch.equal(r.sums_i, full.sums_i)
    R = _reference(0, 0.3, me.SLOTS3)
    assert r.pairs == int(R["sums_i"][:, 0].sum()) and r.ped_pairs == int(R["sums_i"][:, 1].sum())
    assert abs(r.jade - R["sums_f"][:, 0].sum() / r.pairs) <= TOL


@pytest.mark.parametrize("i", [0, 1], ids=[tj.IDS[0], tj.IDS[1]])
def test_joint_one_slot_block_is_the_full_covariance_head(gpu, i):
    """One live slot, b = 0: FullCovHead.joint_eval bit for bit, from
    MixtureHead.from_fullcov and from the NaN test block of the same factor."""
    from multimodaltraj_2_amd.mixture import MixtureHead
    c = tj._inputs(i)
    fc = tj._fc(c, gpu)
    want = tj._run(i, 0.3, gpu, head=fc)
    clean = tj._fc(dict(chol=np.tril(np.nan_to_num(c["chol"]))), gpu)
    for mx in (MixtureHead.from_fullcov(clean), _mx(me.one_slot_block(c["chol"]), gpu)):
        got = tj._run(i, 0.3, gpu, head=mx)
        assert torch.equal(got.sums_f, want.sums_f) and torch.equal(got.sums_i, want.sums_i)
        assert torch.equal(got.per_frame_f, want.per_frame_f)
        assert torch.equal(got.per_frame_i, want.per_frame_i)
    assert int(want.sums_i[:, 4].sum()) > 0


# ---------------------------------------------------------------------------
# KDE-NLL
# ---------------------------------------------------------------------------
KDE = [(i, w) for i in range(len(kc.CASES)) for w in me.KDE_SCALES]
KDE_IDS = [f"{kc.IDS[i]}-{w}" for i, w in KDE]
_KDEV, _KRES, _KREF = {}, {}, {}


def _kde_inputs(i, which, dev):
    if (i, which) not in _KDEV:
        c = kc.inputs(i)
        t = {k: _t(c[k], dev) for k in ("pred", "targets", "n_active", "n_frames", "ped_mask")}
        _KDEV[i, which] = (_mx(me.kde_block(i, which), dev), t)
    return _KDEV[i, which]


def _kde_run(i, which, dev, head=None, want_per_ped=True, log_floor=FLOOR):
    c = kc.inputs(i)
    h, t = _kde_inputs(i, which, dev)
    r = (head or h).kde_nll(t["pred"], t["targets"], t["n_active"], c["K"], seed=c["seed"],
                            log_floor=log_floor, n_frames=t["n_frames"], ped_mask=t["ped_mask"],
                            want_per_ped=want_per_ped, targets_shared=c["shared"])
    torch.cuda.synchronize()
    return r


def _kde_result(i, which, dev):
    if (i, which) not in _KRES:
        _KRES[i, which] = _kde_run(i, which, dev)
    return _KRES[i, which]


def _kde_recount(i, which, dev):
    """The float64 checker over the device's own K draws (computed once)."""
    if (i, which) not in _KREF:
        c = kc.inputs(i)
        h, t = _kde_inputs(i, which, dev)
        draws = np.stack([h.sample(t["pred"], seed=(c["seed"] + k) & MASK64).cpu().numpy()
                          for k in range(c["K"])])
        _KREF[i, which] = me.kde_nll_ref(draws, c["targets"], c["pairs"], FLOOR)
    return _KREF[i, which]


@pytest.mark.parametrize("i,which", KDE, ids=KDE_IDS)
def test_kde_recount_from_the_devices_own_draws(gpu, i, which):
    c = kc.inputs(i)
    r, R = _kde_result(i, which, gpu), _kde_recount(i, which, gpu)
    m = c["pairs"]
    per, out = r.per_ped.cpu().numpy().astype(np.float64), r.out.cpu().numpy().astype(np.float64)
    assert np.isfinite(per).all() and np.isfinite(out).all()
    d_pair = float(np.abs(per[..., :2] - R["per_ped"][..., :2]).max())
    npairs = R["out"][:, 2]
    d_out = np.abs(out[:, :2] - R["out"][:, :2]).max(axis=1)
    print(f"case {kc.IDS[i]} {which}: {int(m.sum())} pairs, worst |kernel - float64| per pair "
          f"{d_pair:.3g} (gate {me.GATE:.3g}), per scene {d_out.max():.3g} (gate x pairs "
          f"{(me.GATE * npairs).max():.3g})")
    assert d_pair <= me.GATE
    assert np.all(d_out <= me.GATE * npairs)
    np.testing.assert_array_equal(out[:, 2], npairs)
    assert np.all(out[:, 4] == c["K"]) and np.all(out[:, 5] == FLOOR) and np.all(out[:, 6:] == 0)
    assert np.all(per[~m] == 0) and np.all(per[..., 3] == 0)               # non-pairs: exactly zero
    assert np.all(per[..., 0][m] <= -FLOOR) and np.all(per[..., 1][m] <= -FLOOR)
    # the clip counts: exact, but for steps within the gate of the floor or next to det H = 0
    near = m[..., None] & ((np.abs(R["logp"] - FLOOR) <= me.GATE) | R["near_singular"])
    sure = (R["clip"] & ~near & m[..., None]).sum(axis=-1)
    extra = per[..., 2] - sure
    print(f"   clipped steps {int(per[..., 2].sum())} of {12 * int(m.sum())}, {int(near.sum())} "
          f"within the gate of the floor or next to det H = 0")
    assert near.sum() <= 0.01 * 12 * max(1, int(m.sum()))
    assert np.all(extra >= 0) and np.all(extra <= near.sum(axis=-1))
    assert np.all(np.abs(out[:, 3] - sure.sum(axis=(1, 2))) <= near.sum(axis=(1, 2, 3)))
    assert per[..., 2].sum() < 12 * m.sum()                                # not everything on the floor
    if kc.IDS[i] == "far":                                                 # the clip path is exercised
        assert 0.05 <= r.clipped_share <= 0.95
    if m.any():
        assert abs(r.kde_nll - R["out"][:, 0].sum() / m.sum()) <= me.GATE
        assert r.pairs == int(m.sum())


@pytest.mark.parametrize("i,which", [(0, "near"), (1, "far")], ids=["k5-near", "chunks-far"])
def test_kde_repeated_calls_and_null_per_ped(gpu, i, which):
    """A second call's bits; per_ped NULL leaves out's bits alone; the
    poisoned columns of pred / targets and of the block were never read."""
    a, b = _kde_result(i, which, gpu), _kde_run(i, which, gpu)
    assert torch.equal(a.per_ped, b.per_ped) and torch.equal(a.out, b.out)
    c = _kde_run(i, which, gpu, want_per_ped=False)
    assert c.per_ped is None and torch.equal(c.out, a.out)
    assert not bool(torch.isnan(a.per_ped).any())
    assert bool((a.per_ped[~_t(kc.inputs(i)["pairs"], gpu)] == 0).all())


@pytest.mark.parametrize("i", [0, 6], ids=[kc.IDS[0], kc.IDS[6]])
def test_kde_one_slot_block_is_the_full_covariance_head_within_the_gate(gpu, i):
    """One live slot, b = 0: the draws are FullCovHead's bit for bit, the
    moments are taken by this head's scheme, so a pair's figures agree with
    FullCovHead.kde_nll within mix_eval_ref.GATE, not bit for bit.  Pairs with
    a step whose float64 log density (the checker on the device's own draws)
    lies within that gate of the floor may clip in one kernel and not in the
    other: they are left out of both comparisons, and such steps are at most
    1 % of the case's steps."""
    from multimodaltraj_2_amd.fullcov import FullCovHead
    c = kc.inputs(i)
    _, t = _kde_inputs(i, "near", gpu)
    fc = FullCovHead(device=gpu)
    fc.chol = _t(c["chol"], gpu)
    want = fc.kde_nll(t["pred"], t["targets"], t["n_active"], c["K"], seed=c["seed"], log_floor=FLOOR,
                      n_frames=t["n_frames"], ped_mask=t["ped_mask"], want_per_ped=True,
                      targets_shared=c["shared"])
    mx = _mx(me.one_slot_block(c["chol"]), gpu)
    got = _kde_run(i, "near", gpu, head=mx)
    draws = [mx.sample(t["pred"], seed=(c["seed"] + k) & MASK64) for k in range(c["K"])]
    assert torch.equal(draws[1].nan_to_num(), fc.sample(t["pred"], seed=(c["seed"] + 1) & MASK64).nan_to_num())
    R = me.kde_nll_ref(np.stack([x.cpu().numpy() for x in draws]), c["targets"], c["pairs"], FLOOR)
    bound = me.GATE
    near_steps = c["pairs"][..., None] & (np.abs(R["logp"] - FLOOR) <= bound)
    near = near_steps.any(axis=-1)
    a, b = got.per_ped.cpu().numpy().astype(np.float64), want.per_ped.cpu().numpy().astype(np.float64)
    d = float(np.abs(a[..., :2] - b[..., :2])[~near].max())
    print(f"case {kc.IDS[i]}: one-slot mixture vs FullCovHead.kde_nll, worst pair {d:.3g} (gate "
          f"{bound:.3g}); {int(near_steps.sum())} steps next to the floor in {int(near.sum())} pairs")
    assert d <= bound
    np.testing.assert_array_equal(a[..., 2][~near], b[..., 2][~near])
    assert near_steps.sum() <= 0.01 * 12 * max(1, int(c["pairs"].sum()))
    assert torch.equal(got.out[:, 2], want.out[:, 2]) and int(want.out[:, 2].sum()) > 0


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def test_evaluation_end_to_end(gpu, tmp_path, data_root):
    """The recipe of tests/test_mixture_gpu.py::test_evaluation_end_to_end with
    --collision_radius 0.2 --kde_nll 1: MIX_JOINT_FIGURES and MIX_KDE_FIGURES
    after the existing keys, which do not change; two more log lines; every new
    figure finite and equal to a direct call on ``keep``'s tensors; with either
    flag at its default or --mixture_head off, nothing new."""
    from multimodaltraj_2_amd import checkpoint, evaluate
    from multimodaltraj_2_amd import train as tr
    from multimodaltraj_2_amd.argParser import ArgsParser
    argv = ["--data_root", data_root, "--leaveDataset", "2", "--n_max", "32", "--train_scenes", "64",
            "--train_batch", "32", "--num_epochs", "2", "--loss", "l2", "--num_samples", "4",
            "--mode", "train", "--save_dir", str(tmp_path), "--log_dir", str(tmp_path),
            "--device", "cuda:0"]
    args = ArgsParser().parser.parse_args(argv)
    tr.run_train_mode(args, gpu, log=lambda s: None)
    prm = checkpoint.load_params(checkpoint.read_state(str(tmp_path)), device=gpu)
    new = evaluate.MIX_JOINT_FIGURES + evaluate.MIX_KDE_FIGURES
    args.fit_head, args.mixture_head = "eval", "eval"
    logs0, keep0 = [], {}
    res0 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs0.append, keep=keep0)
    assert list(res0)[-len(evaluate.MIX_FIGURES):] == list(evaluate.MIX_FIGURES)
    assert not set(new) & set(res0) and sorted(keep0["mixture"]) == ["fit", "head", "out", "stats"]

    args.collision_radius, args.kde_nll = 0.2, 1
    args.mixture_head = "off"
    logs_off = []
    res_off = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs_off.append)
    assert not any(k.startswith("mix_") for k in res_off)
    args.mixture_head = "eval"
    logs, keep = [], {}
    res = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs.append, keep=keep)
    assert list(res) == list(res_off) + list(evaluate.MIX_FIGURES) + list(new)
    assert {k: res[k] for k in res_off} == res_off and {k: res[k] for k in res0} == res0
    assert len(logs) == len(logs_off) + 3 and logs[:len(logs_off)] == logs_off
    assert logs[-3].startswith("mixture head on dataset 2")
    assert logs[-2].startswith("mixture joint best-of-K on dataset 2: radius 0.2, K 4,")
    assert logs[-1].startswith("mixture KDE-NLL of the 4 draws on dataset 2:")
    assert sorted(keep["mixture"]) == ["fit", "head", "joint", "kde", "out", "stats"]
    # each flag alone adds its own figures only
    args.kde_nll = 0
    res_j = evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
    assert list(res_j)[-4:] == list(evaluate.MIX_JOINT_FIGURES) and "mix_kde_nll" not in res_j
    args.collision_radius, args.kde_nll = 0.0, 1
    res_k = evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
    assert list(res_k)[-3:] == list(evaluate.MIX_KDE_FIGURES) and "mix_jade" not in res_k
    # a direct call on keep's tensors
    mx = keep["mixture"]["head"]
    t = keep["plan"].to_device(gpu, F=1)
    one = torch.ones(keep["plan"].S, dtype=torch.int32, device=gpu)
    je = mx.joint_eval(keep["pred"], t["targets"], t["n_active"], 4, 0.2, seed=args.sample_seed,
                       n_frames=one, ped_mask=t["ped_mask"])
    kd = mx.kde_nll(keep["pred"], t["targets"], t["n_active"], 4, seed=args.sample_seed,
                    log_floor=args.kde_floor, n_frames=one, ped_mask=t["ped_mask"])
    direct = dict(evaluate.mixture_joint_figures(je), **evaluate.kde_figures(kd, "mix_"))
    assert tuple(direct) == new
    for k in new:
        print(f"evaluation {k}: {res[k]:.8g}")
        assert np.isfinite(res[k]) and res[k] == direct[k], k
    assert torch.equal(keep["mixture"]["joint"].sums_i, je.sums_i)
    assert torch.equal(keep["mixture"]["joint"].per_frame_f, je.per_frame_f)
    assert torch.equal(keep["mixture"]["kde"].out, kd.out)
    assert je.pairs == kd.pairs == res["pairs"] and je.ped_pairs == res["ped_pairs"]
    assert torch.equal(je.sums_i[:, :4], keep["joint"].sums_i[:, :4])      # head-independent columns
    assert res["mix_jade"] >= res["mix_min_ade"] - TOL and res["mix_jfde"] >= res["mix_min_fde"] - TOL
    assert f"JADE_4 {res['mix_jade']:.6g}" in logs[-2] and f"{res['mix_kde_nll']:.6g}" in logs[-1]
    assert 0.0 <= res["mix_kde_clipped"] <= 1.0 and res["mix_kde_nll"] <= -args.kde_floor
