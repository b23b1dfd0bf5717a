"""GPU: the fused best-of-K sampling evaluation (g2k_best_of_k_f32,
csrc/g2k_bestk.hip; GaussianHead.best_of_k; evaluate.py) against the float64
checker tests/bestk_ref.py.  PARITY UNPINNED: the reference has no
probabilistic head.  Tolerance: the project's rule close(got, ref) <= 1e-4,
|d| <= 1e-4 * max(1, |ref|).  Indices are not compared for equality (the
checker's best and second-best ADE can differ by less than fp32 resolves):
the checker's error AT the kernel's index must be within tolerance of the
checker's minimum.  The shapes are the smallest that reach every branch: the
draws of a pair on 1, 2, 4 and 16 lanes, K not a multiple of the lanes, one
and several frame chunks per scene (the direct and the two-kernel sums), more
pairs than threads, shared targets, NULL mask / n_frames, a seed that wraps."""
import functools

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd.synthetic import make_batch
from tests.bestk_ref import MASK64, best_of_k_ref
from tests.conftest import close

pytestmark = pytest.mark.gpu
TOL = 1e-4
SEED = (7 << 32) + 99

#        S  F   Nmax K   sigma n_active              n_frames          mask   shared seed
CASES = [(5, 3, 20, 20, 0.05, [0, 1, 13, 20, 7], [3, 0, 2, 3, 1], True, False, SEED),
         (2, 2, 256, 3, 1.0, [256, 37], None, False, False, SEED),         # widest tile, NULLs
         (3, 4, 17, 1, 0.3, [17, 1, 0], [4, 2, 4], True, False, SEED),     # K = 1
         (2, 40, 32, 7, 0.3, [32, 21], [40, 33], True, False, SEED),       # many chunks, K % lanes != 0
         (3, 4, 20, 20, 0.05, [20, 0, 13], [4, 4, 0], True, True, SEED),   # shared targets
         (2, 2, 9, 5, 0.3, [9, 4], [2, 1], True, False, (1 << 64) - 2)]    # the seed wraps
IDS = ["s5f3n20k20", "n256", "k1", "f40k7", "shared", "wrap"]


@functools.lru_cache(maxsize=None)
def _inputs(i):
    S, F, N, K, sigma, nact, nfr, masked, shared, seed = CASES[i]
    rng = np.random.default_rng(100 + i)
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


@functools.lru_cache(maxsize=None)
def _reference(i, K=None):
    c = _inputs(i)
    return best_of_k_ref(c["pred"], c["targets"], c["n_active"], c["head"], c["seed"], K or c["K"],
                         c["n_frames"], c["ped_mask"])


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(i, dev, K=None, want_best=True):
    from multimodaltraj_2_amd.nll import GaussianHead
    c = _inputs(i)
    gh = GaussianHead(device=dev)
    gh.head = _t(c["head"], dev)
    pred = _t(c["pred"], dev)
    r = gh.best_of_k(pred, _t(c["targets"], dev), _t(c["n_active"], dev), K or c["K"], seed=c["seed"],
                     n_frames=_t(c["n_frames"], dev), ped_mask=_t(c["ped_mask"], dev),
                     targets_shared=c["shared"], want_best=want_best)
    torch.cuda.synchronize()
    return gh, pred, r


_CACHE = {}


def _gpu_result(i, dev):
    if i not in _CACHE:
        _CACHE[i] = _run(i, dev)
    return _CACHE[i]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_values_match_checker(gpu, i):
    _, _, r = _gpu_result(i, gpu)
    R = _reference(i)
    per, out = r.per_ped.cpu().numpy(), r.sums.cpu().numpy()
    m = R["pairs"]
    print(f"case {IDS[i]}: pairs {int(m.sum())}, per_ped err {close(per[..., :2], R['per_ped'][..., :2]):.3g}, "
          f"sums err {close(out[:, :5], R['out'][:, :5]):.3g}")
    assert close(per[..., :2], R["per_ped"][..., :2]) <= TOL
    assert close(out[:, :5], R["out"][:, :5]) <= TOL
    np.testing.assert_array_equal(out[:, 2], R["out"][:, 2])
    np.testing.assert_array_equal(out[:, 5], R["out"][:, 5])
    assert np.all(out[:, 6:] == 0)
    assert np.all(per[~m] == 0)                           # non-pairs: exactly zero, all four


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_indices_attain_the_minimum(gpu, i):
    _, _, r = _gpu_result(i, gpu)
    R = _reference(i)
    K = CASES[i][3]
    per = r.per_ped.cpu().numpy().astype(np.float64)
    m = R["pairs"]
    for col, errs in ((2, R["ade_k"]), (3, R["fde_k"])):
        k = per[..., col][m]                              # every pair
        assert np.all(k == np.round(k)) and np.all((k >= 0) & (k < K))
        at = np.take_along_axis(errs, per[..., col].astype(np.int64)[None], axis=0)[0][m]
        best = errs.min(axis=0)[m]
        worst = float((np.abs(at - best) / np.maximum(1.0, np.abs(best))).max()) if at.size else 0.0
        print(f"case {IDS[i]} col {col}: {at.size} pairs, checker error at the kernel's index vs "
              f"checker minimum: {worst:.3g}")
        assert worst <= TOL


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_best_is_the_unfused_draw_exactly(gpu, i):
    """best == GaussianHead.sample(pred, seed + kA) gathered per pedestrian,
    bit for bit (the shared draw helper), and pred off the pairs."""
    gh, pred, r = _gpu_result(i, gpu)
    c = _inputs(i)
    pairs = torch.from_numpy(_reference(i)["pairs"]).to(gpu)
    kA = r.per_ped[..., 2]
    want = pred.clone()
    for k in range(c["K"]):
        sel = pairs & (kA == k)
        if bool(sel.any()):
            xk = gh.sample(pred, seed=(c["seed"] + k) & MASK64)
            want = torch.where(sel[:, :, None, :], xk, want)
    assert torch.equal(r.best, want)
    off = ~pairs[:, :, None, :].expand_as(pred)
    assert torch.equal(r.best[off], pred[off])
    if bool(pairs.any()):
        assert not torch.equal(r.best, pred)


def test_nested_draws(gpu):
    """The draws of K = 10 are the first ten of K = 20 (which are dealt to
    more lanes): the minima can only fall, exactly."""
    a = _run(0, gpu, K=10, want_best=False)[2].per_ped
    b = _gpu_result(0, gpu)[2].per_ped
    assert bool((b[..., 0] <= a[..., 0]).all()) and bool((b[..., 1] <= a[..., 1]).all())
    assert bool((b[..., 0] < a[..., 0]).any())


@pytest.mark.parametrize("i", [0, 3], ids=[IDS[0], IDS[3]])
def test_repeated_calls_are_bit_identical(gpu, i):
    a, b = _gpu_result(i, gpu)[2], _run(i, gpu)[2]
    assert torch.equal(a.sums, b.sums) and torch.equal(a.per_ped, b.per_ped)
    assert torch.equal(a.best, b.best)


def test_mean_errors_agree_with_the_fused_step(gpu):
    """out[:, 3:5] (ADE / FDE of the mean prediction) == the fused step's
    metrics[:, 3:5] over the same pairs."""
    from multimodaltraj_2_amd import frame_step as fs
    from multimodaltraj_2_amd.nll import GaussianHead
    b = make_batch(6, 32, 64, F=5)
    t = b.to_device(gpu)
    out = fs.step_fused(fs.init_params(32, seed=0, device=gpu), t["pos"], t["vislet"], t["G"],
                        t["targets"], t["n_active"], t["h0"])
    r = GaussianHead(log_sigma=-2.0, device=gpu).best_of_k(out.pred, t["targets"], t["n_active"], 4)
    torch.cuda.synchronize()
    got, want = r.sums.cpu().numpy(), out.metrics.cpu().numpy()
    assert close(got[:, 3:5], want[:, 3:5]) <= TOL
    np.testing.assert_array_equal(got[:, 2], want[:, 1])
    assert r.pairs == int(b.n_active.sum()) * 5
    assert abs(r.ade - want[:, 3].sum() / want[:, 1].sum()) <= TOL * max(1.0, r.ade)


def test_evaluation_end_to_end(gpu, tmp_path, data_root):
    """--mode train --loss nll --num_samples 4 evaluates the trained
    parameters on the left-out dataset; evaluate_best_of_k's figures are the
    checker's on the same plan's host tensors (pred read back); the CLI on
    the saved checkpoint gives the same figures exactly.  (minADE_K can
    exceed the mean's ADE, so that is not asserted.)"""
    from multimodaltraj_2_amd import checkpoint, evaluate
    from multimodaltraj_2_amd import train as tr
    from multimodaltraj_2_amd.argParser import ArgsParser
    argv = ["--data_root", data_root, "--leaveDataset", "2", "--n_max", "32", "--train_scenes", "64",
            "--train_batch", "32", "--num_epochs", "1", "--loss", "nll", "--num_samples", "4",
            "--mode", "train", "--save_dir", str(tmp_path), "--log_dir", str(tmp_path),
            "--device", "cuda:0"]
    args = ArgsParser().parser.parse_args(argv)
    logs = []
    params, losses = tr.run_train_mode(args, gpu, log=logs.append)      # still (params, losses)
    assert len(losses) == 2 and np.all(np.isfinite(params))
    line = [s for s in logs if s.startswith("best-of-4 on dataset 2")]
    assert len(line) == 1, logs
    assert any("learned head" in s for s in logs)

    prm = checkpoint.load_params(checkpoint.read_state(str(tmp_path)), device=gpu)
    assert prm.head is not None and prm.nmax == 32
    keep = {}
    res = evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None, keep=keep)
    plan = keep["plan"]
    h = plan.host(F=1)
    R = best_of_k_ref(keep["pred"].cpu().numpy(), h["targets"], h["n_active"],
                      keep["head"].cpu().numpy(), args.sample_seed, 4, keep["n_frames"], h["ped_mask"])
    tot = R["out"].sum(axis=0)
    assert res["scenes"] == plan.S and res["K"] == 4
    assert res["pairs"] == int(tot[2]) and res["pairs"] > 0
    want = dict(min_ade=tot[0] / tot[2], min_fde=tot[1] / tot[2], ade=tot[3] / tot[2],
                fde=tot[4] / tot[2])
    for k in evaluate.FIGURES:
        print(f"evaluation {k}: {res[k]:.8g} (checker {want[k]:.8g})")
        assert np.isfinite(res[k])
        assert abs(res[k] - want[k]) <= TOL * max(1.0, abs(want[k])), k
    assert f"minADE_4 {res['min_ade']:.6g}" in line[0]                    # the run logged these figures
    cli = evaluate.main(argv, log=lambda s: None)
    assert [cli[k] for k in evaluate.FIGURES] == [res[k] for k in evaluate.FIGURES]
    assert cli["pairs"] == res["pairs"]
    # parameters without a head: the constant --head_log_sigma head
    prm.head = None
    logs2 = []
    args.head_log_sigma = -3.0
    res2 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs2.append)
    assert any("constant log sigma -3.0" in s for s in logs2)
    assert res2["ade"] == res["ade"] and res2["min_ade"] != res["min_ade"]
