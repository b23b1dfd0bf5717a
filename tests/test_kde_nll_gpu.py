"""GPU: the fused KDE-NLL evaluation (g2k_kde_nll_f32, g2k_fullcov_kde_nll_f32,
csrc/g2k_kde.hip; GaussianHead.kde_nll, FullCovHead.kde_nll; evaluate.py)
against the float64 checker tests/kde_ref.py fed with the DEVICE's own draws
(the head's sampler called K times at seeds seed + k), so that the comparison
sees the kernel's arithmetic and not the draws'.  PARITY UNPINNED against the
reference (it has no probabilistic head); the checker is pinned against
scipy.stats.gaussian_kde in tests/test_kde_nll.py.  Tolerance: kde_ref.GATE,
absolute, 8 x the checker's own restated-precision error on these inputs
(measured on the CPU, tests/test_kde_nll.py::test_gate_measurement); a scene's
sums get the gate times its pair count.  Clip counts are compared exactly but
for steps whose float64 log density lies within the gate of the floor.  The
cases (tests/kde_cases.py) are the smallest that reach each path."""
import ctypes

import numpy as np
import pytest
import torch

from tests import kde_cases as kc
from tests import kde_ref as kr
from tests.abi_arena import Arena, all_written
from tests.bestk_ref import MASK64

pytestmark = pytest.mark.gpu
FLOOR = -20.0
BOTH = [(i, w) for i in range(len(kc.CASES)) for w in kc.HEADS]
BOTH_IDS = [f"{kc.IDS[i]}-{w}" for i, w in BOTH]


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_DEV = {}


def _device_inputs(i, which, dev):
    """(head object, dict of device tensors) of case i."""
    if (i, which) not in _DEV:
        from multimodaltraj_2_amd.fullcov import FullCovHead
        from multimodaltraj_2_amd.nll import GaussianHead
        c = kc.inputs(i)
        if which == "per_step":
            h = GaussianHead(device=dev)
            h.head = _t(c["head"], dev)
        else:
            h = FullCovHead(device=dev)
            h.chol = _t(c["chol"], dev)
        t = {k: _t(c[k], dev) for k in ("pred", "targets", "n_active", "n_frames", "ped_mask")}
        _DEV[(i, which)] = (h, t)
    return _DEV[(i, which)]


def _run(i, which, dev, log_floor=FLOOR, want_per_ped=True, K=None):
    c = kc.inputs(i)
    h, t = _device_inputs(i, which, dev)
    r = h.kde_nll(t["pred"], t["targets"], t["n_active"], K or c["K"], seed=c["seed"],
                  log_floor=log_floor, n_frames=t["n_frames"], ped_mask=t["ped_mask"],
                  want_per_ped=want_per_ped, targets_shared=c["shared"])
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
        c = kc.inputs(i)
        h, t = _device_inputs(i, which, dev)
        draws = np.stack([h.sample(t["pred"], seed=(c["seed"] + k) & MASK64).cpu().numpy()
                          for k in range(c["K"])])
        _REF[(i, which)] = kr.kde_nll_ref(draws, c["targets"], c["pairs"], FLOOR)
    return _REF[(i, which)]


@pytest.mark.parametrize("i,which", BOTH, ids=BOTH_IDS)
def test_recount_from_the_devices_own_draws(gpu, i, which):
    c = kc.inputs(i)
    r, R = _result(i, which, gpu), _recount(i, which, gpu)
    m = c["pairs"]
    per, out = r.per_ped.cpu().numpy().astype(np.float64), r.out.cpu().numpy().astype(np.float64)
    assert np.isfinite(per).all() and np.isfinite(out).all()
    d_pair = float(np.abs(per[..., :2] - R["per_ped"][..., :2]).max())
    npairs = R["out"][:, 2]
    d_out = np.abs(out[:, :2] - R["out"][:, :2]).max(axis=1)
    print(f"case {kc.IDS[i]} {which}: {int(m.sum())} pairs, worst |kernel - float64| per pair "
          f"{d_pair:.3g} (gate {kr.GATE:.3g}), per scene {d_out.max():.3g} (gate x pairs "
          f"{(kr.GATE * npairs).max():.3g})")
    assert d_pair <= kr.GATE
    assert np.all(d_out <= kr.GATE * npairs)
    np.testing.assert_array_equal(out[:, 2], npairs)
    assert np.all(out[:, 4] == c["K"]) and np.all(out[:, 5] == FLOOR) and np.all(out[:, 6:] == 0)
    assert np.all(per[~m] == 0) and np.all(per[..., 3] == 0)               # non-pairs: exactly zero
    assert np.all(per[..., 0][m] <= -FLOOR) and np.all(per[..., 1][m] <= -FLOOR)
    # the clip counts: exact, but for steps within the gate of the floor
    near = m[..., None] & (np.abs(R["logp"] - FLOOR) <= kr.GATE)
    sure = (R["clip"] & ~near & m[..., None]).sum(axis=-1)
    extra = per[..., 2] - sure
    print(f"   clipped steps {int(per[..., 2].sum())} of {12 * int(m.sum())}, {int(near.sum())} "
          f"within the gate of the floor")
    assert near.sum() <= 0.01 * 12 * max(1, int(m.sum()))
    assert np.all(extra >= 0) and np.all(extra <= near.sum(axis=-1))
    assert np.all(np.abs(out[:, 3] - sure.sum(axis=(1, 2))) <= near.sum(axis=(1, 2, 3)))
    if kc.IDS[i] == "far":
        assert 0.05 <= r.clipped_share <= 0.95
    # the result class's figures are the sums'
    if m.any():
        assert abs(r.kde_nll - R["out"][:, 0].sum() / m.sum()) <= kr.GATE
        assert r.pairs == int(m.sum())


def _raw_call(i, which, dev, per_ped, out, log_floor=FLOOR):
    """The entry point itself, on caller-made buffers."""
    from multimodaltraj_2_amd import _lib
    from multimodaltraj_2_amd.frame_step import _ptr
    lib = _lib.load()
    c = kc.inputs(i)
    h, t = _device_inputs(i, which, dev)
    d = h._dims(t["pred"])
    if c["shared"]:
        d.flags = _lib.STEP_TARGETS_SHARED
    stem = "g2k_kde_nll" if which == "per_step" else "g2k_fullcov_kde_nll"
    need = int(getattr(lib, stem + "_workspace_bytes")(ctypes.byref(d)))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = getattr(lib, stem + "_f32")(ctypes.byref(d), _ptr(t["pred"]), _ptr(t["targets"]),
                                     _ptr(t["n_active"]), _ptr(t["n_frames"]), _ptr(t["ped_mask"]),
                                     _ptr(h.head if which == "per_step" else h.chol),
                                     ctypes.c_uint64(c["seed"]), c["K"], ctypes.c_float(log_floor),
                                     _ptr(per_ped), _ptr(out), _ptr(ws), need, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.g2k_last_error()


@pytest.mark.parametrize("which", kc.HEADS)
@pytest.mark.parametrize("i", [0, 1], ids=[kc.IDS[0], kc.IDS[1]])
def test_determinism_and_footprint(gpu, i, which):
    """Guarded, poisoned outputs: every element written, nothing outside;
    the bits of a second call and of the Python path; per_ped NULL leaves out's
    bits alone; non-pairs exactly zero."""
    c = kc.inputs(i)
    S, F, _, N = c["pred"].shape
    ar = Arena(gpu)
    per, out = ar.alloc((S, F, N, 4), name="per_ped"), ar.alloc((S, 8), name="out")
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
    assert bool((per[~_t(c["pairs"], gpu)] == 0).all())
    assert not bool(torch.isnan(per).any())                                 # the poisoned columns were never read


@pytest.mark.parametrize("which", kc.HEADS)
def test_relations(gpu, which):
    """Pairs as best_of_k's; the floor caps a term, so a higher floor never
    raises kde_nll (and never lowers the clip count); a floor below every
    density clips nothing."""
    i = kc.IDS.index("far")
    c = kc.inputs(i)
    h, t = _device_inputs(i, which, gpu)
    r = _result(i, which, gpu)
    bk = h.best_of_k(t["pred"], t["targets"], t["n_active"], c["K"], seed=c["seed"],
                     n_frames=t["n_frames"], ped_mask=t["ped_mask"], want_per_ped=False)
    assert torch.equal(bk.sums[:, 2], r.out[:, 2])
    hi, lo = _run(i, which, gpu, log_floor=-8.0), _run(i, which, gpu, log_floor=-1e30)
    assert bool((hi.per_ped[..., :2] <= r.per_ped[..., :2]).all())
    assert bool((hi.per_ped[..., 0] < r.per_ped[..., 0]).any())
    assert bool((hi.per_ped[..., 2] >= r.per_ped[..., 2]).all())
    assert bool((lo.per_ped[..., :2] >= r.per_ped[..., :2]).all())
    assert bool((lo.out[:, 3] == 0).all()) and lo.clipped_share == 0.0
    assert bool(torch.isfinite(lo.per_ped).all())
    assert bool((lo.out[:, 5] == np.float32(-1e30)).all())
    # where nothing clipped at -20, the floor does not enter at all
    free = r.per_ped[..., 2] == 0
    assert torch.equal(lo.per_ped[..., :2][free], r.per_ped[..., :2][free])


def test_python_argument_checks(gpu):
    h, t = _device_inputs(0, "per_step", gpu)
    for k in (3, 4097):
        with pytest.raises(ValueError, match="4..4096"):
            h.kde_nll(t["pred"], t["targets"], t["n_active"], k)
    with pytest.raises(ValueError, match="log_floor"):
        h.kde_nll(t["pred"], t["targets"], t["n_active"], 4, log_floor=float("-inf"))
    with pytest.raises(ValueError, match="targets must be"):
        h.kde_nll(t["pred"], t["targets"][:, :1], t["n_active"], 4)


def test_evaluation_end_to_end(gpu, tmp_path, data_root):
    """The recipe of tests/test_fullcov_gpu.py::test_evaluation_end_to_end with
    --num_samples 4 --kde_nll 1, without and with --fullcov_head train: the new
    keys after the old ones, finite and equal to a direct kde_nll call on
    ``keep``'s tensors; one more log line each; without the flag the parent's
    keys."""
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
    tr.run_train_mode(args, gpu, log=lambda s: None)
    prm = checkpoint.load_params(checkpoint.read_state(str(tmp_path)), device=gpu)
    logs0, keep0 = [], {}
    res0 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs0.append, keep=keep0)
    assert list(res0) == ["scenes", "pairs", "K"] + list(evaluate.FIGURES)
    assert "kde" not in keep0 and not any("KDE-NLL" in s for s in logs0)

    args.kde_nll = 1
    logs1, keep1 = [], {}
    res1 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs1.append, keep=keep1)
    assert list(res1) == list(res0) + list(evaluate.KDE_FIGURES)
    assert {k: res1[k] for k in res0} == res0 and len(logs1) == len(logs0) + 1
    assert sum(s.startswith("KDE-NLL of the 4 draws on dataset 2:") for s in logs1) == 1
    t = keep1["plan"].to_device(gpu, F=1)
    one = torch.ones(keep1["plan"].S, dtype=torch.int32, device=gpu)
    gh = GaussianHead(device=gpu)
    gh.head = keep1["head"]
    direct = gh.kde_nll(keep1["pred"], t["targets"], t["n_active"], 4, seed=args.sample_seed,
                        log_floor=args.kde_floor, n_frames=one, ped_mask=t["ped_mask"])
    want = evaluate.kde_figures(direct)
    assert tuple(want) == evaluate.KDE_FIGURES
    for k in evaluate.KDE_FIGURES:
        print(f"evaluation {k}: {res1[k]:.8g}")
        assert np.isfinite(res1[k]) and res1[k] == want[k], k
    assert torch.equal(keep1["kde"].out, direct.out) and direct.pairs == res1["pairs"]
    assert 0.0 <= res1["kde_clipped"] <= 1.0 and res1["kde_nll"] <= -args.kde_floor

    args.fullcov_head = "train"
    logs2, keep2 = [], {}
    res2 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs2.append, keep=keep2)
    assert list(res2) == list(res1) + list(evaluate.FULLCOV_FIGURES) + list(evaluate.FULLCOV_KDE_FIGURES)
    assert {k: res2[k] for k in res1} == res1 and len(logs2) == len(logs1) + 2
    assert logs2[-1].startswith("full-covariance KDE-NLL of the 4 draws on dataset 2:")
    fc = FullCovHead(device=gpu)
    fc.chol = keep2["fullcov_chol"]
    fdirect = fc.kde_nll(keep2["pred"], t["targets"], t["n_active"], 4, seed=args.sample_seed,
                         log_floor=args.kde_floor, n_frames=one, ped_mask=t["ped_mask"])
    fwant = evaluate.kde_figures(fdirect, "fullcov_")
    assert tuple(fwant) == evaluate.FULLCOV_KDE_FIGURES
    for k in evaluate.FULLCOV_KDE_FIGURES:
        print(f"evaluation {k}: {res2[k]:.8g} (per-step head: {res2[k.replace('fullcov_', '')]:.8g})")
        assert np.isfinite(res2[k]) and res2[k] == fwant[k], k
    assert torch.equal(keep2["fullcov"]["kde"].out, fdirect.out)
    assert f"{res2['fullcov_kde_nll']:.6g}" in logs2[-1] and f"{res2['kde_nll']:.6g}" in logs2[-1]
    # the flag off again: the parent's keys with the full-covariance head too
    args.kde_nll = 0
    res3 = evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
    assert list(res3) == list(res0) + list(evaluate.FULLCOV_FIGURES)
    # the CLI, and K below 4
    cli = evaluate.main(argv + ["--kde_nll", "1", "--fullcov_head", "train"], log=lambda s: None)
    assert list(cli) == list(res2) and [cli[k] for k in res2] == [res2[k] for k in res2]
    args.kde_nll, args.num_samples = 1, 3
    with pytest.raises(ValueError, match="K >= 4"):
        evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
