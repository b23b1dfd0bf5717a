"""GPU: the fused joint best-of-K evaluation of the full-covariance head
(g2k_fullcov_joint_eval_f32, csrc/g2k_joint.hip; FullCovHead.joint_eval;
evaluate.py --fullcov_head with --collision_radius) against the float64 checker
tests/fullcov_joint_ref.py and against the device's own draws.  PARITY
UNPINNED: the reference has no probabilistic head.

Against the checker the rules are those of tests/test_joint_eval_gpu.py: floats
close(got, ref) <= 1e-4; indices are not compared for equality (the checker's
value AT the kernel's index must be within tolerance of the checker's minimum);
collision counts are bracketed between the checker's counts at radius -/+ 1e-4,
after the cap on the checker alone (the couple-draws within 1e-4 of the radius
are at most 1e-3 of all couple-draws and at most 1 % of the collisions).

The sharp test exists because the draw is bit-defined: draw k of every member
is FullCovHead.sample(pred, seed + k).  Those f32 coordinates are fetched and
the couples recounted in float64 at radius (1 -/+ 1e-6); the kernel's counts
must lie in that bracket.  The margin is derived: the kernel's comparison
fmaf(dx, dx, dy * dy) < radius * radius in f32 has a relative error of about
2e-7 of the radius (one rounding each in dx and dy, three in the fmaf form, one
in radius^2); the bracket gives five times that.

Shapes: the eight of tests/test_joint_eval_gpu.py restated (the smallest that
reach every branch: P = 0, 1, 2 and a full 256, P across wave boundaries, lane
groups of 16 / 32 / 64 with item lists that do and do not fill them, K = 1,
K = 7 dealt to 4 units, F = 40, shared targets, NULL mask and n_frames, a seed
that wraps 2^64) and the structured couples case; the same pred / targets /
mask construction and seeds, each case's sigma, and the factor walk_factor(
sigma, default_rng(rs + 1000)) with NaN above the diagonal."""
import functools

import numpy as np
import pytest
import torch

from tests import fullcov_joint_ref as fj
from tests.bestk_ref import MASK64, draw_errors
from tests.conftest import close
from tests.joint_ref import couples_case

pytestmark = pytest.mark.gpu
TOL = 1e-4
REL = 1e-6                                                 # the recount's bracket: radius (1 -/+ REL)
SEED = (7 << 32) + 99

#        S  F   Nmax K   sigma n_active              n_frames          mask   shared seed             rng
CASES = [(5, 3, 20, 20, 0.05, [0, 1, 13, 20, 7], [3, 0, 2, 3, 1], True, False, SEED, 100),
         (2, 2, 256, 3, 1.0, [256, 37], None, False, False, SEED, 101),     # four waves, NULLs
         (2, 1, 256, 2, 0.3, [129, 65], None, True, False, SEED, 106),      # P across wave boundaries
         (3, 4, 17, 1, 0.3, [17, 1, 0], [4, 2, 4], True, False, SEED, 102),   # K = 1
         (2, 40, 32, 7, 0.3, [32, 21], [40, 33], True, False, SEED, 103),   # many frames, K = 7 on 4 units
         (3, 4, 20, 20, 0.05, [20, 0, 13], [4, 4, 0], True, True, SEED, 104),   # shared targets
         (2, 2, 9, 5, 0.3, [9, 4], [2, 1], True, False, (1 << 64) - 2, 105),    # the seed wraps
         (3, 2, 64, 5, 0.3, [64, 40, 2], [2, 1, 2], False, False, SEED, 107)]   # one group of 64; P = 2
IDS = ["s5f3n20k20", "n256", "n256waves", "k1", "f40k7", "shared", "wrap", "n64"]
COUPLES = len(CASES)                                       # the structured case's index
K_COUPLES = 6
#       (case, radius)
RUNS = [(i, 0.3) for i in range(len(CASES))] + [(0, 0.1), (0, 0.0), (COUPLES, 0.1), (COUPLES, 0.3)]
RUN_IDS = [f"{(IDS + ['couples'])[i]}-r{r}" for i, r in RUNS]
POSITIVE = [(r, n) for r, n in zip(RUNS, RUN_IDS) if r[1] > 0]


@functools.lru_cache(maxsize=None)
def _inputs(i):
    if i == COUPLES:
        c, _ = couples_case()
        chol = fj.nan_above(fj.walk_factor(1e-3, np.random.default_rng(999)))
        return dict(c, chol=chol, K=K_COUPLES, seed=SEED, shared=False)
    S, F, N, K, sigma, nact, nfr, masked, shared, seed, rs = CASES[i]
    rng = np.random.default_rng(rs)
    pred = rng.standard_normal((S, F, 24, N)).astype(np.float32)
    Ft = 1 if shared else F
    base = pred[:, :Ft].reshape(S, Ft, 2, 12, N).transpose(0, 1, 4, 3, 2)
    tg = (base + sigma * rng.standard_normal((S, Ft, N, 12, 2))).astype(np.float32)
    head = np.stack([np.log(sigma) + 0.2 * rng.standard_normal(12),
                     np.log(sigma) + 0.2 * rng.standard_normal(12),
                     0.5 * rng.standard_normal(12)]).astype(np.float32)
    pm = (rng.random((S, N)) > 0.2).astype(np.uint8) if masked else None
    chol = fj.nan_above(fj.walk_factor(sigma, np.random.default_rng(rs + 1000)))
    return dict(pred=pred, targets=np.ascontiguousarray(tg), head=head, chol=chol,
                n_active=np.array(nact, np.int32),
                n_frames=None if nfr is None else np.array(nfr, np.int32), ped_mask=pm,
                K=K, seed=seed, shared=shared)


def assert_cap(amb, couple_draws, collisions, label):
    """The ambiguous couple-draws are at most 1e-3 of all couple-draws and at
    most 1 % of the collisions: the bracket cannot hide a failure."""
    print(f"{label}: {couple_draws} couple-draws, {collisions} collisions, {amb} ambiguous")
    assert amb <= 1e-3 * couple_draws and amb <= 0.01 * collisions


@functools.lru_cache(maxsize=None)
def _reference(i, radius):
    c = _inputs(i)
    R = fj.joint_eval_ref(c["pred"], c["targets"], c["n_active"], c["chol"], c["seed"], c["K"], radius,
                          c["n_frames"], c["ped_mask"])
    assert_cap(int(R["amb_k"].sum()), c["K"] * int(R["per_frame_i"][..., 1].sum()),
               int(R["col_k"].sum()), f"checker, case {i} radius {radius}")
    return R


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _fc(c, dev):
    from multimodaltraj_2_amd.fullcov import FullCovHead
    fc = FullCovHead(device=dev)
    fc.chol = _t(c["chol"], dev)
    return fc


def _gh(c, dev):
    from multimodaltraj_2_amd.nll import GaussianHead
    gh = GaussianHead(device=dev)
    gh.head = _t(c["head"], dev)
    return gh


def _args(c, dev):
    return (_t(c["pred"], dev), _t(c["targets"], dev), _t(c["n_active"], dev)), \
        dict(n_frames=_t(c["n_frames"], dev), ped_mask=_t(c["ped_mask"], dev), targets_shared=c["shared"])


def _run(i, radius, dev, K=None, head=None, **over):
    c = _inputs(i)
    a, kw = _args(c, dev)
    kw.update(over)
    r = (head or _fc(c, dev)).joint_eval(*a, K or c["K"], radius, seed=c["seed"], **kw)
    torch.cuda.synchronize()
    return r


_CACHE = {}


def _gpu_result(i, radius, dev):
    if (i, radius) not in _CACHE:
        _CACHE[i, radius] = _run(i, radius, dev)
    return _CACHE[i, radius]


def _host(r):
    return (r.per_frame_f.cpu().numpy().astype(np.float64), r.per_frame_i.cpu().numpy().astype(np.int64),
            r.sums_f.cpu().numpy().astype(np.float64), r.sums_i.cpu().numpy())


@pytest.mark.parametrize("i,radius", RUNS, ids=RUN_IDS)
def test_values_match_checker(gpu, i, radius):
    R = _reference(i, radius)
    pf, pi, sf, si = _host(_gpu_result(i, radius, gpu))
    K = _inputs(i)["K"]
    print(f"{RUN_IDS[RUNS.index((i, radius))]}: members {int(R['per_frame_i'][..., 0].sum())}, per_frame err "
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


@pytest.mark.parametrize("i,radius", RUNS[:len(CASES)] + RUNS[-2:-1],
                         ids=RUN_IDS[:len(CASES)] + RUN_IDS[-2:-1])
def test_indices_attain_the_minimum(gpu, i, radius):
    R = _reference(i, radius)
    pf = _host(_gpu_result(i, radius, gpu))[0]
    K = _inputs(i)["K"]
    on = R["per_frame_i"][..., 0] > 0
    for col, errs in ((2, R["jade_k"]), (3, R["jfde_k"])):
        k = pf[..., col][on]
        assert np.all(k == np.round(k)) and np.all((k >= 0) & (k < K))
        at = np.take_along_axis(errs, pf[..., col].astype(np.int64)[None], axis=0)[0][on]
        best = errs.min(axis=0)[on]
        worst = float((np.abs(at - best) / np.maximum(1.0, np.abs(best))).max()) if at.size else 0.0
        print(f"case {i} col {col}: {at.size} scene-frames, checker error at the kernel's index vs "
              f"checker minimum: {worst:.3g}")
        assert worst <= TOL


def _between(lo, x, hi):
    return bool(np.all(lo <= x) and np.all(x <= hi))


@pytest.mark.parametrize("i,radius", RUNS, ids=RUN_IDS)
def test_collision_counts_within_the_checkers_bracket(gpu, i, radius):
    R = _reference(i, radius)
    pf, pi, _, si = _host(_gpu_result(i, radius, gpu))
    lo_k, hi_k = R["col_lo"].sum(axis=0), R["col_hi"].sum(axis=0)
    print(f"case {i} radius {radius}: col_pred {pi[..., 2].sum()} in [{R['pred_lo'].sum()}, "
          f"{R['pred_hi'].sum()}], col_gt {pi[..., 3].sum()} in [{R['gt_lo'].sum()}, {R['gt_hi'].sum()}], "
          f"sum col_k {pi[..., 4].sum()} in [{lo_k.sum()}, {hi_k.sum()}], col_best {pi[..., 5].sum()}")
    for col, lo, hi in ((2, R["pred_lo"], R["pred_hi"]), (3, R["gt_lo"], R["gt_hi"]), (4, lo_k, hi_k)):
        assert _between(lo, pi[..., col], hi), col                     # per scene-frame
        assert _between(lo.sum(axis=1), si[:, col], hi.sum(axis=1)), col   # per scene
    kJA = pf[..., 2].astype(np.int64)                      # the KERNEL's index
    blo = np.take_along_axis(R["col_lo"], kJA[None], axis=0)[0]
    bhi = np.take_along_axis(R["col_hi"], kJA[None], axis=0)[0]
    on = R["per_frame_i"][..., 0] > 0
    assert _between(blo[on], pi[..., 5][on], bhi[on])
    assert _between((blo * on).sum(axis=1), si[:, 5], (bhi * on).sum(axis=1))
    if radius > 0 and i != COUPLES:
        assert pi[..., 4].sum() > 0                        # there is something to count


@functools.lru_cache(maxsize=None)
def _device_draws(i, dev):
    """[K, S, F, 24, N] f32: FullCovHead.sample at the seeds (seed + k) mod 2^64."""
    c = _inputs(i)
    fc, pred = _fc(c, dev), _t(c["pred"], dev)
    xs = [fc.sample(pred, seed=(c["seed"] + k) & MASK64).cpu().numpy() for k in range(c["K"])]
    return np.stack(xs)


@pytest.mark.parametrize("i,radius", [r for r, _ in POSITIVE], ids=[n for _, n in POSITIVE])
def test_counts_against_the_devices_own_draws(gpu, i, radius):
    """The sharp test: the draws are the sampler's, bit for bit, so the counts
    recounted in float64 from the sampler's f32 coordinates at radius (1 -/+
    1e-6) bracket the kernel's, and JADE_k recomputed from them gives the
    kernel's minimum."""
    c = _inputs(i)
    R = _reference(i, radius)
    pf, pi, _, si = _host(_gpu_result(i, radius, gpu))
    xs = _device_draws(i, gpu)
    m = R["members"]
    lo, hi, amb = fj.recount(xs, m, radius, REL)
    assert_cap(int(amb.sum()), c["K"] * int(pi[..., 1].sum()), int(lo.sum()),
               f"device draws, case {i} radius {radius}")
    print(f"case {i} radius {radius}: sum col_k {pi[..., 4].sum()} in [{lo.sum()}, {hi.sum()}]")
    assert _between(lo.sum(axis=0), pi[..., 4], hi.sum(axis=0))
    assert _between(lo.sum(axis=(0, 2)), si[:, 4], hi.sum(axis=(0, 2)))
    kJA = pf[..., 2].astype(np.int64)
    on = pi[..., 0] > 0
    blo = np.take_along_axis(lo, kJA[None], axis=0)[0]
    bhi = np.take_along_axis(hi, kJA[None], axis=0)[0]
    assert _between(blo[on], pi[..., 5][on], bhi[on])
    # JADE_k / JFDE_k in float64 from the device's draws
    Pd = np.maximum(m.sum(axis=2), 1)
    jade, jfde = np.empty(lo.shape), np.empty(lo.shape)
    for k in range(c["K"]):
        a, f = draw_errors(xs[k].astype(np.float64), c["targets"])     # every element is finite
        jade[k], jfde[k] = (a * m).sum(axis=2) / Pd, (f * m).sum(axis=2) / Pd
    err = close(pf[..., 0], jade.min(axis=0) * on), close(pf[..., 1], jfde.min(axis=0) * on)
    print(f"case {i}: minJADE / minJFDE vs the float64 recomputation from the device's draws: "
          f"{err[0]:.3g} / {err[1]:.3g}")
    assert max(err) <= TOL
    # the kernel's index attains that minimum
    at = np.take_along_axis(jade, kJA[None], axis=0)[0]
    assert close(at * on, jade.min(axis=0) * on) <= TOL


@pytest.mark.parametrize("radius", [0.1, 0.3])
def test_structured_couples_exactly(gpu, radius):
    """Every collision column is exactly the hand count."""
    _, intact = couples_case()
    _reference(COUPLES, radius)
    _, pi, _, si = _host(_gpu_result(COUPLES, radius, gpu))
    assert intact.tolist() == [[8, 8], [6, 6], [5, 0]]
    np.testing.assert_array_equal(pi[..., 2], intact)
    np.testing.assert_array_equal(pi[..., 3], intact)
    np.testing.assert_array_equal(pi[..., 4], K_COUPLES * intact)
    np.testing.assert_array_equal(pi[..., 5], intact)
    np.testing.assert_array_equal(si[:, 2:], np.stack([intact.sum(axis=1)] * 2 + [K_COUPLES * intact.sum(
        axis=1), intact.sum(axis=1)], axis=1))


@pytest.mark.parametrize("i", [0, 1, 5, COUPLES], ids=[IDS[0], IDS[1], IDS[5], "couples"])
def test_head_independent_columns_are_the_per_step_kernels(gpu, i):
    """P, PP, col_pred and col_gt do not depend on the head: bit for bit those
    of g2k_joint_eval_f32 on the same inputs."""
    a = _gpu_result(i, 0.3, gpu)
    b = _run(i, 0.3, gpu, head=_gh(_inputs(i), gpu))
    assert torch.equal(a.per_frame_i[..., :4], b.per_frame_i[..., :4])
    assert torch.equal(a.sums_i[:, :4], b.sums_i[:, :4])
    assert int(a.sums_i[:, 1].sum()) > 0


def _marginal(i, dev, K=None):
    c = _inputs(i)
    a, kw = _args(c, dev)
    r = _fc(c, dev).best_of_k(*a, K or c["K"], seed=c["seed"], **kw)
    torch.cuda.synchronize()
    return r.per_ped.cpu().numpy().astype(np.float64)


def test_one_draw_is_the_marginal_kernels_sum(gpu):
    """K = 1: P * minJADE == the per-scene-frame sum of g2k_fullcov_best_of_k_f32's
    minADE (the same draws through the shipped marginal kernel)."""
    i = IDS.index("k1")
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


def test_nested_draws(gpu):
    """The draws of K' = 10 are the first ten of K = 20 (dealt differently):
    the K' run gives the prefix minima of the checker's jade_k / jfde_k and the
    prefix's collisions; K = 20 does not rise above it; the mean's and the
    targets' columns do not change."""
    R = _reference(0, 0.3)
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


@pytest.mark.parametrize("i", [0, 1], ids=[IDS[0], IDS[1]])
def test_block_factor_agrees_with_the_per_step_head(gpu, i):
    """FullCovHead.from_gaussian_head(head): the same distribution through the
    other kernel; JADE / JFDE agree within the tolerance."""
    from multimodaltraj_2_amd.fullcov import FullCovHead
    c = _inputs(i)
    gh = _gh(c, gpu)
    a = _run(i, 0.3, gpu, head=FullCovHead.from_gaussian_head(gh.head))
    b = _run(i, 0.3, gpu, head=gh)
    err = close(a.per_frame_f[..., :2].cpu().numpy(), b.per_frame_f[..., :2].cpu().numpy())
    print(f"case {i}: block factor vs per-step head, minJADE / minJFDE: {err:.3g}")
    assert err <= TOL
    assert close(a.sums_f[:, :2].cpu().numpy(), b.sums_f[:, :2].cpu().numpy()) <= TOL
    assert torch.equal(a.per_frame_i[..., :4], b.per_frame_i[..., :4])


@pytest.mark.parametrize("i", [0, 1], ids=[IDS[0], IDS[1]])        # one wave per unit; four
def test_repeated_calls_are_bit_identical(gpu, i):
    a, b = _gpu_result(i, 0.3, gpu), _run(i, 0.3, gpu)
    assert torch.equal(a.sums_f, b.sums_f) and torch.equal(a.sums_i, b.sums_i)
    assert torch.equal(a.per_frame_f, b.per_frame_f) and torch.equal(a.per_frame_i, b.per_frame_i)


def test_outputs_may_be_omitted(gpu):
    r = _run(0, 0.3, gpu, want_per_frame=False)
    full = _gpu_result(0, 0.3, gpu)
    assert r.per_frame_f is None and r.per_frame_i is None
    assert torch.equal(r.sums_f, full.sums_f) and torch.equal(r.sums_i, full.sums_i)
    R = _reference(0, 0.3)
    assert r.pairs == int(R["sums_i"][:, 0].sum()) and r.ped_pairs == int(R["sums_i"][:, 1].sum())
    assert abs(r.jade - R["sums_f"][:, 0].sum() / r.pairs) <= TOL
    assert r.collision_rate_gt == int(full.sums_i[:, 3].sum()) / r.ped_pairs


def test_null_mask_and_frames(gpu):
    """NULL n_frames / ped_mask: every frame, every column below n_active."""
    c = _inputs(0)
    r = _run(0, 0.3, gpu, n_frames=None, ped_mask=None)
    P = np.broadcast_to(np.clip(c["n_active"], 0, 20)[:, None], (5, 3))
    np.testing.assert_array_equal(r.per_frame_i[..., 0].cpu().numpy(), P)
    np.testing.assert_array_equal(r.per_frame_i[..., 1].cpu().numpy(), P * (P - 1) // 2)
    assert bool(torch.isfinite(r.per_frame_f).all())


def test_evaluation_end_to_end(gpu, tmp_path, data_root):
    """The recipe of tests/test_fullcov_gpu.py::test_evaluation_end_to_end with
    --fullcov_head train --collision_radius 0.2 --num_samples 4: exactly
    FULLCOV_JOINT_FIGURES after FULLCOV_FIGURES, each finite and equal to a
    direct FullCovHead.joint_eval call on ``keep``'s tensors and factor; one
    more log line; nothing new with either flag at its default."""
    from multimodaltraj_2_amd import checkpoint, evaluate
    from multimodaltraj_2_amd import train as tr
    from multimodaltraj_2_amd.argParser import ArgsParser
    from multimodaltraj_2_amd.fullcov import FullCovHead
    argv = ["--data_root", data_root, "--leaveDataset", "2", "--n_max", "32", "--train_scenes", "64",
            "--train_batch", "32", "--num_epochs", "2", "--loss", "l2", "--num_samples", "4",
            "--mode", "train", "--save_dir", str(tmp_path), "--log_dir", str(tmp_path),
            "--device", "cuda:0"]
    args = ArgsParser().parser.parse_args(argv)
    tr.run_train_mode(args, gpu, log=lambda s: None)
    prm = checkpoint.load_params(checkpoint.read_state(str(tmp_path)), device=gpu)
    new, prefix = evaluate.FULLCOV_JOINT_FIGURES, "full-covariance joint best-of-K on dataset"
    logs0, keep0 = [], {}
    res0 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs0.append, keep=keep0)

    # each flag alone: no new key, no new line
    args.collision_radius = 0.2
    logs1, keep1 = [], {}
    res1 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs1.append, keep=keep1)
    assert list(res1) == list(res0) + list(evaluate.JOINT_FIGURES)
    args.collision_radius, args.fullcov_head = 0.0, "train"
    logs2, keep2 = [], {}
    res2 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs2.append, keep=keep2)
    assert list(res2) == list(res0) + list(evaluate.FULLCOV_FIGURES)
    assert "joint" not in keep2["fullcov"]
    for r, lg in ((res0, logs0), (res1, logs1), (res2, logs2)):
        assert not any(k in r for k in new) and not any(s.startswith(prefix) for s in lg)

    # both
    args.collision_radius = 0.2
    logs, keep = [], {}
    res = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs.append, keep=keep)
    assert list(res) == list(res1) + list(evaluate.FULLCOV_FIGURES) + list(new)
    assert {k: res[k] for k in res1} == res1 and {k: res[k] for k in res2} == res2
    assert sorted(keep) == sorted(keep2) and sorted(keep["fullcov"]) == sorted(list(keep2["fullcov"]) + ["joint"])
    line = [s for s in logs if s.startswith(prefix)]
    assert len(line) == 1 and logs[-1] == line[0] and len(logs) == len(logs1) + 2
    assert line[0].startswith(prefix + " 2:")
    fc = FullCovHead(device=gpu)
    fc.chol = keep["fullcov_chol"]
    t = keep["plan"].to_device(gpu, F=1)
    one = torch.ones(keep["plan"].S, dtype=torch.int32, device=gpu)
    je = fc.joint_eval(keep["pred"], t["targets"], t["n_active"], 4, 0.2, seed=args.sample_seed,
                       n_frames=one, ped_mask=t["ped_mask"])
    direct = evaluate.fullcov_joint_figures(je)
    assert tuple(direct) == new
    for k in new:
        print(f"evaluation {k}: {res[k]:.8g} (per-step head: "
              f"{res[k.replace('fullcov_', '')]:.8g})")
        assert np.isfinite(res[k]) and res[k] == direct[k], k
    assert torch.equal(keep["fullcov"]["joint"].sums_i, je.sums_i)
    assert torch.equal(keep["fullcov"]["joint"].per_frame_f, je.per_frame_f)
    assert je.pairs == res["pairs"] and je.ped_pairs == res["ped_pairs"]
    # the head-independent columns are the per-step launch's
    assert torch.equal(je.sums_i[:, :4], keep["joint"].sums_i[:, :4])
    assert res["fullcov_jade"] >= res["fullcov_min_ade"] - TOL
    assert res["fullcov_jfde"] >= res["fullcov_min_fde"] - TOL
    assert f"JADE_4 {res['fullcov_jade']:.6g}" in line[0] and f"{res['jade']:.6g}" in line[0]
    cli = evaluate.main(argv + ["--fullcov_head", "train", "--collision_radius", "0.2"],
                        log=lambda s: None)
    assert list(cli) == list(res) and [cli[k] for k in new] == [res[k] for k in new]
