"""GPU: the fused sample scores (g2k_sample_scores_f32,
g2k_fullcov_sample_scores_f32, g2k_mix_sample_scores_f32, csrc/g2k_scores.hip;
the three heads' ``sample_scores``; evaluate.py) against the float64 checker
tests/scores_ref.py fed with the DEVICE's own draws (the head's sampler called
K times at seeds seed + k), so that the comparison sees the kernel's arithmetic
and not the draws'.  PARITY UNPINNED against the reference (it has no
probabilistic head).  Tolerance: the project's metric tolerance,
|got - ref| <= 1e-4 max(1, |ref|) per pair and that times the pair count for a
scene's sums.  The cases (tests/score_cases.py) are the smallest that reach
each path."""
import ctypes

import numpy as np
import pytest
import torch

from tests import score_cases as sc
from tests import scores_ref as sr
from tests.abi_arena import Arena, all_written
from tests.bestk_ref import MASK64

pytestmark = pytest.mark.gpu
ALL = [(i, w) for i in range(len(sc.CASES)) for w in sc.HEADS]
ALL_IDS = [f"{sc.IDS[i]}-{w}" for i, w in ALL]
STEMS = {"per_step": "g2k_sample_scores", "fullcov": "g2k_fullcov_sample_scores",
         "mix": "g2k_mix_sample_scores"}


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_DEV = {}


def _params(h, which):
    return {"per_step": lambda: h.head, "fullcov": lambda: h.chol, "mix": lambda: h.params}[which]()


def _device_inputs(i, which, dev):
    """(head object, dict of device tensors) of case i."""
    if (i, which) not in _DEV:
        from multimodaltraj_2_amd.fullcov import FullCovHead
        from multimodaltraj_2_amd.mixture import MixtureHead
        from multimodaltraj_2_amd.nll import GaussianHead
        c = sc.inputs(i)
        if which == "per_step":
            h = GaussianHead(device=dev)
            h.head = _t(c["head"], dev)
        elif which == "fullcov":
            h = FullCovHead(device=dev)
            h.chol = _t(c["chol"], dev)
        else:
            h = MixtureHead.from_block(c["mix"], device=dev)
        t = {k: _t(c[k], dev) for k in ("pred", "targets", "n_active", "n_frames", "ped_mask")}
        _DEV[(i, which)] = (h, t)
    return _DEV[(i, which)]


def _run(i, which, dev, want_per_ped=True):
    c = sc.inputs(i)
    h, t = _device_inputs(i, which, dev)
    r = h.sample_scores(t["pred"], t["targets"], t["n_active"], c["K"], seed=c["seed"],
                        n_frames=t["n_frames"], ped_mask=t["ped_mask"], want_per_ped=want_per_ped,
                        targets_shared=c["shared"])
    torch.cuda.synchronize()
    return r


_RES, _REF = {}, {}


def _result(i, which, dev):
    if (i, which) not in _RES:
        _RES[(i, which)] = _run(i, which, dev)
    return _RES[(i, which)]


def _recount(i, which, dev):
    """The float64 checker over the device's own K draws (computed once)."""
    if (i, which) not in _REF:
        c = sc.inputs(i)
        h, t = _device_inputs(i, which, dev)
        draws = np.stack([h.sample(t["pred"], seed=(c["seed"] + k) & MASK64).cpu().numpy()
                          for k in range(c["K"])])
        _REF[(i, which)] = sr.sample_scores_ref(draws, c["targets"], c["pairs"])
    return _REF[(i, which)]


def _gate(ref):
    return sr.TOL * np.maximum(1.0, np.abs(ref))


@pytest.mark.parametrize("i,which", ALL, ids=ALL_IDS)
def test_recount_from_the_devices_own_draws(gpu, i, which):
    c = sc.inputs(i)
    r, R = _result(i, which, gpu), _recount(i, which, gpu)
    m = c["pairs"]
    per, out = r.per_ped.cpu().numpy().astype(np.float64), r.out.cpu().numpy().astype(np.float64)
    assert np.isfinite(per).all() and np.isfinite(out).all()
    e_pair = np.abs(per[..., :7] - R["per_ped"][..., :7]) / _gate(R["per_ped"][..., :7])
    npairs = R["out"][:, 7]
    e_out = np.abs(out[:, :7] - R["out"][:, :7]) / (_gate(R["out"][:, :7]) * np.maximum(npairs, 1)[:, None])
    worst = np.unravel_index(np.argmax(e_pair), e_pair.shape)
    print(f"case {sc.IDS[i]} {which}: {int(m.sum())} pairs, worst |kernel - float64| / gate per pair "
          f"{e_pair.max():.3g} (column {sr.COLS[worst[-1]]}), per scene {e_out.max():.3g}")
    assert e_pair.max() <= 1.0
    assert e_out.max() <= 1.0
    np.testing.assert_array_equal(out[:, 7], npairs)                       # pair counts: exact
    assert np.all(per[~m] == 0) and np.all(per[..., 7] == 0)               # non-pairs: exactly zero
    # the result class's figures are the sums'
    if m.any():
        want = sr.figures(R["out"])
        for k, v in want.items():
            assert abs(getattr(r, k) - v) <= sr.TOL * max(1.0, abs(v)), k
        assert r.pairs == int(m.sum()) and r.k == c["K"]
    else:
        assert np.isnan(r.es_traj)


def _raw_call(i, which, dev, per_ped, out, t=None, ws=None):
    """The entry point itself, on caller-made buffers."""
    from multimodaltraj_2_amd import _lib, scores
    from multimodaltraj_2_amd.frame_step import _ptr
    lib = scores.load()
    c = sc.inputs(i)
    h, t0 = _device_inputs(i, which, dev)
    t = t or dict(t0, params=_params(h, which))
    d = h._dims(t0["pred"])
    if c["shared"]:
        d.flags = _lib.STEP_TARGETS_SHARED
    need = int(lib.g2k_sample_scores_workspace_bytes(ctypes.byref(d)))
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = getattr(lib, STEMS[which] + "_f32")(ctypes.byref(d), _ptr(t["pred"]), _ptr(t["targets"]),
                                             _ptr(t["n_active"]), _ptr(t["n_frames"]),
                                             _ptr(t["ped_mask"]), _ptr(t["params"]),
                                             ctypes.c_uint64(c["seed"]), c["K"], _ptr(per_ped), _ptr(out),
                                             _ptr(ws), need, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.g2k_last_error()
    return need


FOOT = [sc.IDS.index(n) for n in ("k20", "passes", "tail")]


@pytest.mark.parametrize("which", sc.HEADS)
@pytest.mark.parametrize("i", FOOT, ids=[sc.IDS[i] for i in FOOT])
def test_determinism_and_footprint(gpu, i, which):
    """Guarded, poisoned outputs: every element written, nothing outside; the
    bits of a second call and of the Python path; per_ped NULL leaves out's
    bits alone; non-pairs exactly zero."""
    c = sc.inputs(i)
    S, F, _, N = c["pred"].shape
    ar = Arena(gpu)
    per, out = ar.alloc((S, F, N, 8), name="per_ped"), ar.alloc((S, 8), name="out")
    out2 = ar.alloc((S, 8), name="out2")
    _raw_call(i, which, gpu, per, out)
    ar.check_guards()
    assert all_written(per) and all_written(out)
    r = _result(i, which, gpu)
    assert torch.equal(per, r.per_ped) and torch.equal(out, r.out)
    again = _run(i, which, gpu)
    assert torch.equal(again.per_ped, r.per_ped) and torch.equal(again.out, r.out)
    _raw_call(i, which, gpu, None, out2)
    ar.check_guards()
    assert all_written(out2) and torch.equal(out2, out)
    assert _run(i, which, gpu, want_per_ped=False).per_ped is None
    assert bool((per[~_t(c["pairs"], gpu)] == 0).all())
    assert not bool(torch.isnan(per).any())                                 # the poisoned columns were never read


@pytest.mark.parametrize("which", sc.HEADS)
def test_relations(gpu, which):
    """Pairs as best_of_k's; the expected error of a draw is never below the
    best draw's; every energy score >= -gate."""
    for name in ("k20", "n256"):
        i = sc.IDS.index(name)
        c = sc.inputs(i)
        h, t = _device_inputs(i, which, gpu)
        r = _result(i, which, gpu)
        bk = h.best_of_k(t["pred"], t["targets"], t["n_active"], c["K"], seed=c["seed"],
                         n_frames=t["n_frames"], ped_mask=t["ped_mask"], want_per_ped=True)
        assert torch.equal(bk.sums[:, 2], r.out[:, 7])
        per = r.per_ped.cpu().numpy().astype(np.float64)
        best = bk.per_ped.cpu().numpy().astype(np.float64)
        m = c["pairs"]
        assert np.all(per[..., 0][m] >= best[..., 0][m] - sr.TOL)          # mA >= minADE
        assert np.all(per[..., 1][m] >= best[..., 1][m] - sr.TOL)          # mF >= minFDE
        for es, mcol in zip(sr.es_columns(per), (0, 1, 2)):
            assert np.all(es[m] >= -sr.TOL * np.maximum(1.0, per[..., mcol][m]))
        assert np.all(per[..., 3:7][m] >= 0)


def test_one_slot_mixture_is_the_fullcov_head(gpu):
    from multimodaltraj_2_amd.mixture import MixtureHead
    for name in ("k20", "k65"):
        i = sc.IDS.index(name)
        c = sc.inputs(i)
        fc, t = _device_inputs(i, "fullcov", gpu)
        mx = MixtureHead.from_fullcov(fc)
        r = mx.sample_scores(t["pred"], t["targets"], t["n_active"], c["K"], seed=c["seed"],
                             n_frames=t["n_frames"], ped_mask=t["ped_mask"], want_per_ped=True,
                             targets_shared=c["shared"])
        f = _result(i, "fullcov", gpu)
        assert torch.equal(r.per_ped, f.per_ped) and torch.equal(r.out, f.out)


@pytest.mark.parametrize("which", sc.HEADS)
def test_at_minimum_alignment(gpu, which):
    """Each entry point at the weakest pointer alignment its header line
    states (targets 8, per_ped 16, workspace 4) and every other pointer at its
    element's own (4; the mask 1): the bits of the aligned call."""
    i = sc.IDS.index("shared")
    c = sc.inputs(i)
    S, F, _, N = c["pred"].shape
    h, _ = _device_inputs(i, which, gpu)
    ar = Arena(gpu)
    t = dict(pred=ar.put(c["pred"], "pred", 4), targets=ar.put(c["targets"], "targets", 8),
             n_active=ar.put(c["n_active"], "n_active", 4), n_frames=ar.put(c["n_frames"], "n_frames", 4),
             ped_mask=ar.put(c["ped_mask"], "ped_mask", 1),
             params=ar.put(_params(h, which).cpu().numpy(), "params", 4))
    assert t["targets"].data_ptr() % 16 == 8 and t["pred"].data_ptr() % 16 == 4
    per, out = ar.alloc((S, F, N, 8), name="per_ped"), ar.alloc((S, 8), name="out", offset=4)
    from multimodaltraj_2_amd import scores
    need = scores.load().g2k_sample_scores_workspace_bytes(ctypes.byref(h._dims(_t(c["pred"], "cpu"))))
    ws = ar.alloc((need,), torch.uint8, name="workspace", offset=4)
    assert _raw_call(i, which, gpu, per, out, t=t, ws=ws) == need
    ar.check_guards()
    r = _result(i, which, gpu)
    assert torch.equal(per, r.per_ped) and torch.equal(out, r.out)


def test_python_argument_checks(gpu):
    for which in sc.HEADS:
        h, t = _device_inputs(0, which, gpu)
        for k in (1, 257):
            with pytest.raises(ValueError, match="2..256"):
                h.sample_scores(t["pred"], t["targets"], t["n_active"], k)
        with pytest.raises(ValueError, match="targets must be"):
            h.sample_scores(t["pred"], t["targets"][:, :1], t["n_active"], 4)
        with pytest.raises(ValueError, match="n_active must be"):
            h.sample_scores(t["pred"], t["targets"], t["n_active"][:1], 4)


def test_evaluation_end_to_end(gpu, tmp_path, data_root):
    """The recipe of tests/test_kde_nll_gpu.py::test_evaluation_end_to_end with
    --num_samples 4 --sample_scores 1, without and with --fullcov_head train and
    --mixture_head train: the new keys in the stated places, finite and equal
    to a direct call on ``keep``'s tensors; the old keys and values unchanged,
    one more log line per head; without the flag the parent's keys; K = 1 with
    the flag raises."""
    from multimodaltraj_2_amd import checkpoint, evaluate
    from multimodaltraj_2_amd import train as tr
    from multimodaltraj_2_amd.argParser import ArgsParser
    from multimodaltraj_2_amd.fullcov import FullCovHead
    from multimodaltraj_2_amd.nll import GaussianHead
    argv = ["--data_root", data_root, "--leaveDataset", "2", "--n_max", "32", "--train_scenes", "64",
            "--train_batch", "32", "--num_epochs", "2", "--loss", "l2", "--num_samples", "4",
            "--mode", "train", "--save_dir", str(tmp_path), "--log_dir", str(tmp_path),
            "--device", "cuda:0"]
    args = ArgsParser().parser.parse_args(argv)
    assert args.sample_scores == 0
    tr.run_train_mode(args, gpu, log=lambda s: None)
    prm = checkpoint.load_params(checkpoint.read_state(str(tmp_path)), device=gpu)
    logs0, keep0 = [], {}
    res0 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs0.append, keep=keep0)
    assert list(res0) == ["scenes", "pairs", "K"] + list(evaluate.FIGURES)
    assert "scores" not in keep0 and not any("sample scores" in s for s in logs0)
    assert evaluate.SCORE_FIGURES == ("es_traj", "es_ade", "es_fde", "mean_ade", "mean_fde", "apd", "vs")

    args.sample_scores = 1
    logs1, keep1 = [], {}
    res1 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs1.append, keep=keep1)
    assert list(res1) == list(res0) + list(evaluate.SCORE_FIGURES)
    assert {k: res1[k] for k in res0} == res0 and len(logs1) == len(logs0) + 1
    assert logs1[:len(logs0)] == logs0
    assert logs1[-1].startswith("sample scores of the 4 draws on dataset 2:")
    t = keep1["plan"].to_device(gpu, F=1)
    one = torch.ones(keep1["plan"].S, dtype=torch.int32, device=gpu)
    gh = GaussianHead(device=gpu)
    gh.head = keep1["head"]
    kw = dict(seed=args.sample_seed, n_frames=one, ped_mask=t["ped_mask"])
    direct = gh.sample_scores(keep1["pred"], t["targets"], t["n_active"], 4, **kw)
    want = evaluate.score_figures(direct)
    assert tuple(want) == evaluate.SCORE_FIGURES
    for k in evaluate.SCORE_FIGURES:
        print(f"evaluation {k}: {res1[k]:.8g}")
        assert np.isfinite(res1[k]) and res1[k] == want[k], k
    assert torch.equal(keep1["scores"].out, direct.out) and direct.pairs == res1["pairs"]
    assert res1["mean_ade"] >= res1["min_ade"] - sr.TOL and res1["mean_fde"] >= res1["min_fde"] - sr.TOL
    assert f"{res1['es_traj']:.6g}" in logs1[-1] and f"{res1['vs']:.6g}" in logs1[-1]

    # with both other heads; the flag off first: the parent's keys
    args.sample_scores, args.fullcov_head, args.mixture_head = 0, "train", "train"
    logs_off = []
    res_off = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs_off.append)
    assert list(res_off) == list(res0) + list(evaluate.FULLCOV_FIGURES) + list(evaluate.MIX_FIGURES)
    args.sample_scores = 1
    logs2, keep2 = [], {}
    res2 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs2.append, keep=keep2)
    assert list(res2) == (list(res1) + list(evaluate.FULLCOV_FIGURES) + list(evaluate.FULLCOV_SCORE_FIGURES)
                          + list(evaluate.MIX_FIGURES) + list(evaluate.MIX_SCORE_FIGURES))
    assert {k: res2[k] for k in res1} == res1 and {k: res2[k] for k in res_off} == res_off
    assert len(logs2) == len(logs_off) + 3
    assert [s for s in logs2 if "sample scores" not in s] == logs_off
    assert sum(s.startswith("full-covariance sample scores of the 4 draws on dataset 2:") for s in logs2) == 1
    assert logs2[-1].startswith("mixture sample scores of the 4 draws on dataset 2:")
    fc = FullCovHead(device=gpu)
    fc.chol = keep2["fullcov_chol"]
    fwant = evaluate.score_figures(
        fc.sample_scores(keep2["pred"], t["targets"], t["n_active"], 4, **kw), "fullcov_")
    mx = keep2["mixture"]["head"]
    mdirect = mx.sample_scores(keep2["pred"], t["targets"], t["n_active"], 4, **kw)
    mwant = evaluate.score_figures(mdirect, "mix_")
    assert tuple(fwant) == evaluate.FULLCOV_SCORE_FIGURES and tuple(mwant) == evaluate.MIX_SCORE_FIGURES
    for k, v in list(fwant.items()) + list(mwant.items()):
        print(f"evaluation {k}: {res2[k]:.8g}")
        assert np.isfinite(res2[k]) and res2[k] == v, k
    assert torch.equal(keep2["mixture"]["scores"].out, mdirect.out)
    assert keep2["fullcov"]["scores"].pairs == mdirect.pairs == res2["pairs"]
    assert "scores" in keep2 and keep2["scores"].per_ped is not None
    # the CLI, and K outside 2..256
    cli = evaluate.main(argv + ["--sample_scores", "1", "--fullcov_head", "train", "--mixture_head",
                                "train"], log=lambda s: None)
    assert list(cli) == list(res2) and [cli[k] for k in res2] == [res2[k] for k in res2]
    args.num_samples = 1
    with pytest.raises(ValueError, match="2 <= K <= 256"):
        evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
    args.num_samples = 257
    with pytest.raises(ValueError, match="2 <= K <= 256"):
        evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
