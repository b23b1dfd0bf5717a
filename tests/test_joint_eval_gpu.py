"""GPU: the fused joint best-of-K evaluation (g2k_joint_eval_f32,
csrc/g2k_joint.hip; GaussianHead.joint_eval; evaluate.py --collision_radius)
against the float64 checker tests/joint_ref.py.  PARITY UNPINNED: the
reference has no probabilistic head.

Float outputs: the project's rule close(got, ref) <= 1e-4.  Indices are not
compared for equality (the checker's best and second-best JADE can be 1e-5
apart): the checker's JADE AT the kernel's index must be within tolerance of
the checker's minimum.  Collision counts are BRACKETED, not compared: the
threshold is discontinuous and the kernel's draws are f32 against the
checker's f64, so each count must lie between the checker's counts at
radius - 1e-4 and radius + 1e-4.  So that the bracket cannot hide a failure,
every reference first asserts on the checker alone that the couple-draws
within 1e-4 of the radius are at most 1e-3 of all couple-draws and at most 1 %
of the collisions.  The structured couples case (tests/joint_ref.py
couples_case) has nothing near the threshold: its counts are compared exactly
with the hand count.

Shapes: the smallest that reach every branch — P = 0, 1, 2 and a full 256, P
crossing wave boundaries (37, 65, 129; one wave per unit up to Nmax 64, four
above), the one-wave kernel's groups of 16, 32 and 64 lanes (P <= 16, <= 32,
40 and 64) with item lists that do and do not fill the groups, K = 1, K not a multiple of the units the draws are dealt to, many
frames per scene, shared targets, NULL mask and n_frames, a seed that wraps."""
import functools

import numpy as np
import pytest
import torch

from tests.conftest import close
from tests.joint_ref import couples_case, joint_eval_ref

pytestmark = pytest.mark.gpu
TOL = 1e-4
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


@functools.lru_cache(maxsize=None)
def _inputs(i):
    if i == COUPLES:
        c, _ = couples_case()
        return dict(c, K=K_COUPLES, seed=SEED, shared=False)
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
    return dict(pred=pred, targets=np.ascontiguousarray(tg), head=head,
                n_active=np.array(nact, np.int32),
                n_frames=None if nfr is None else np.array(nfr, np.int32), ped_mask=pm,
                K=K, seed=seed, shared=shared)


def assert_bracket_is_tight(R, K, label):
    """On the checker alone: the couple-draws within eps of the radius are at
    most 1e-3 of all couple-draws and at most 1 % of the collisions."""
    amb, cd, col = int(R["amb_k"].sum()), K * int(R["per_frame_i"][..., 1].sum()), int(R["col_k"].sum())
    print(f"{label}: {cd} couple-draws, {col} collisions, {amb} ambiguous "
          f"({amb / max(cd, 1):.3g} of the couple-draws)")
    assert amb <= 1e-3 * cd and amb <= 0.01 * col


@functools.lru_cache(maxsize=None)
def _reference(i, radius, K=None):
    c = _inputs(i)
    K = K or c["K"]
    R = joint_eval_ref(c["pred"], c["targets"], c["n_active"], c["head"], c["seed"], K, radius,
                       c["n_frames"], c["ped_mask"])
    assert_bracket_is_tight(R, K, f"case {i} radius {radius} K {K}")
    return R


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _head(c, dev):
    from multimodaltraj_2_amd.nll import GaussianHead
    gh = GaussianHead(device=dev)
    gh.head = _t(c["head"], dev)
    return gh


def _run(i, radius, dev, K=None):
    c = _inputs(i)
    r = _head(c, dev).joint_eval(_t(c["pred"], dev), _t(c["targets"], dev), _t(c["n_active"], dev),
                                 K or c["K"], radius, seed=c["seed"], n_frames=_t(c["n_frames"], dev),
                                 ped_mask=_t(c["ped_mask"], dev), targets_shared=c["shared"])
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
def test_collision_counts_within_the_bracket(gpu, i, radius):
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


def _marginal(i, dev, K=None):
    c = _inputs(i)
    r = _head(c, dev).best_of_k(_t(c["pred"], dev), _t(c["targets"], dev), _t(c["n_active"], dev),
                                K or c["K"], seed=c["seed"], n_frames=_t(c["n_frames"], dev),
                                ped_mask=_t(c["ped_mask"], dev), targets_shared=c["shared"])
    torch.cuda.synchronize()
    return r.per_ped.cpu().numpy().astype(np.float64)


def test_one_draw_is_the_marginal_kernels_sum(gpu):
    """K = 1: P * minJADE == the per-scene-frame sum of best_of_k's minADE
    (the same draws, bit for bit, through the shipped marginal kernel)."""
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
    """The draws of K = 10 are the first ten of K = 20 (dealt differently):
    minJADE does not rise, the collisions of the draws do not fall, the mean's
    and the targets' do not change."""
    a, b = _run(0, 0.3, gpu, K=10), _gpu_result(0, 0.3, gpu)
    assert bool((b.per_frame_f[..., :2] <= a.per_frame_f[..., :2]).all())
    assert bool((b.per_frame_f[..., 0] < a.per_frame_f[..., 0]).any())
    assert bool((b.per_frame_i[..., 4] >= a.per_frame_i[..., 4]).all())
    assert torch.equal(b.per_frame_i[..., :4], a.per_frame_i[..., :4])


@pytest.mark.parametrize("i", [0, 4], ids=[IDS[0], IDS[4]])
def test_repeated_calls_are_bit_identical(gpu, i):
    a, b = _gpu_result(i, 0.3, gpu), _run(i, 0.3, gpu)
    assert torch.equal(a.sums_f, b.sums_f) and torch.equal(a.sums_i, b.sums_i)
    assert torch.equal(a.per_frame_f, b.per_frame_f) and torch.equal(a.per_frame_i, b.per_frame_i)


def test_outputs_may_be_omitted(gpu):
    c = _inputs(0)
    r = _head(c, gpu).joint_eval(_t(c["pred"], gpu), _t(c["targets"], gpu), _t(c["n_active"], gpu),
                                 c["K"], 0.3, seed=c["seed"], n_frames=_t(c["n_frames"], gpu),
                                 ped_mask=_t(c["ped_mask"], gpu), want_per_frame=False)
    torch.cuda.synchronize()
    full = _gpu_result(0, 0.3, gpu)
    assert r.per_frame_f is None and r.per_frame_i is None
    assert torch.equal(r.sums_f, full.sums_f) and torch.equal(r.sums_i, full.sums_i)
    R = _reference(0, 0.3)
    assert r.pairs == int(R["sums_i"][:, 0].sum()) and r.ped_pairs == int(R["sums_i"][:, 1].sum())
    assert abs(r.jade - R["sums_f"][:, 0].sum() / r.pairs) <= TOL
    assert r.collision_rate_gt == int(full.sums_i[:, 3].sum()) / r.ped_pairs


def test_evaluation_end_to_end(gpu, tmp_path, data_root):
    """--mode train --loss nll --num_samples 4 --collision_radius 0.2: one
    extra log line; the figures are the checker's on the plan's host tensors
    (pred read back); the CLI on the saved checkpoint gives the same values
    exactly; radius 0 adds nothing."""
    from multimodaltraj_2_amd import checkpoint, evaluate
    from multimodaltraj_2_amd import train as tr
    from multimodaltraj_2_amd.argParser import ArgsParser
    argv = ["--data_root", data_root, "--leaveDataset", "2", "--n_max", "32", "--train_scenes", "64",
            "--train_batch", "32", "--num_epochs", "1", "--loss", "nll", "--num_samples", "4",
            "--collision_radius", "0.2", "--mode", "train", "--save_dir", str(tmp_path),
            "--log_dir", str(tmp_path), "--device", "cuda:0"]
    args = ArgsParser().parser.parse_args(argv)
    logs = []
    tr.run_train_mode(args, gpu, log=logs.append)
    line = [s for s in logs if s.startswith("joint best-of-4")]
    assert len(line) == 1, logs
    assert len([s for s in logs if s.startswith("best-of-4 on dataset 2")]) == 1

    prm = checkpoint.load_params(checkpoint.read_state(str(tmp_path)), device=gpu)
    keep = {}
    res = evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None, keep=keep)
    h = keep["plan"].host(F=1)
    R = joint_eval_ref(keep["pred"].cpu().numpy(), h["targets"], h["n_active"],
                       keep["head"].cpu().numpy(), args.sample_seed, 4, 0.2, keep["n_frames"],
                       h["ped_mask"])
    assert_bracket_is_tight(R, 4, "evaluation")
    members, couples = int(R["sums_i"][:, 0].sum()), int(R["sums_i"][:, 1].sum())
    assert res["pairs"] == members and res["ped_pairs"] == couples and couples > 0
    want = dict(jade=R["sums_f"][:, 0].sum() / members, jfde=R["sums_f"][:, 1].sum() / members)
    for k in ("jade", "jfde"):
        print(f"evaluation {k}: {res[k]:.8g} (checker {want[k]:.8g})")
        assert abs(res[k] - want[k]) <= TOL * max(1.0, abs(want[k])), k
    assert res["jade"] >= res["min_ade"] - TOL and res["jfde"] >= res["min_fde"] - TOL
    si = keep["joint"].sums_i.cpu().numpy()
    pf = keep["joint"].per_frame_f.cpu().numpy()
    kJA = pf[..., 2].astype(np.int64)
    brackets = {2: (R["pred_lo"], R["pred_hi"]), 3: (R["gt_lo"], R["gt_hi"]),
                4: (R["col_lo"].sum(axis=0), R["col_hi"].sum(axis=0)),
                5: (np.take_along_axis(R["col_lo"], kJA[None], axis=0)[0],
                    np.take_along_axis(R["col_hi"], kJA[None], axis=0)[0])}
    for col, (lo, hi) in brackets.items():
        print(f"evaluation column {col}: {si[:, col].sum()} in [{lo.sum()}, {hi.sum()}]")
        assert _between(lo.sum(axis=1), si[:, col], hi.sum(axis=1)), col
    assert res["collision_rate"] == si[:, 4].sum() / (4 * couples)
    assert res["collision_rate_pred"] == si[:, 2].sum() / couples
    assert res["collision_rate_best"] == si[:, 5].sum() / couples
    assert res["collision_rate_gt"] == si[:, 3].sum() / couples
    assert f"JADE_4 {res['jade']:.6g}" in line[0]          # the run logged these figures
    cli = evaluate.main(argv, log=lambda s: None)
    assert [cli[k] for k in evaluate.JOINT_FIGURES] == [res[k] for k in evaluate.JOINT_FIGURES]
    assert [cli[k] for k in evaluate.FIGURES] == [res[k] for k in evaluate.FIGURES]
    # radius 0: no extra launch, line or key
    args.collision_radius = 0.0
    logs0 = []
    res0 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs0.append)
    assert not any(k in res0 for k in evaluate.JOINT_FIGURES)
    assert not any(s.startswith("joint") for s in logs0)
    assert res0 == {k: res[k] for k in res0}
