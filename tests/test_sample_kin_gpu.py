"""GPU: the fused kinematic scores (g2k_sample_kin_f32,
g2k_fullcov_sample_kin_f32, g2k_mix_sample_kin_f32, csrc/g2k_kin.hip; the three
heads' ``sample_kin``; evaluate.py) against the checker tests/kin_ref.py fed with
the DEVICE's own draws (the head's sampler called K times at seeds seed + k), so
that the comparison sees the kernel's arithmetic and not the draws'.  PARITY
UNPINNED against the reference (it has no probabilistic head).  The features
are single fp32 operations in a stated order, which the checker restates in
np.float32: the ranks, hist and tot must be EQUAL.  The fp32 sums m, p, d, y
are held to scores_ref.TOL * max(1, |ref|) against the checker's float64 sums,
and that times the scene's pair count for ``sums``.  The cases
(tests/kin_cases.py) are the smallest that reach each path."""
import ctypes

import numpy as np
import pytest
import torch

from tests import kin_cases as kc
from tests import kin_ref as kr
from tests.abi_arena import Arena, all_written
from tests.bestk_ref import MASK64, SEED_A
from tests.scores_ref import TOL
from tests.test_sample_kin import PROP, property_check

pytestmark = pytest.mark.gpu
ALL = [(i, w) for i in range(len(kc.CASES)) for w in kc.HEADS]
ALL_IDS = [f"{kc.IDS[i]}-{w}" for i, w in ALL]
STEMS = {"per_step": "g2k_sample_kin", "fullcov": "g2k_fullcov_sample_kin", "mix": "g2k_mix_sample_kin"}
L = 12


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_DEV = {}


def _params(h, which):
    return {"per_step": lambda: h.head, "fullcov": lambda: h.chol, "mix": lambda: h.params}[which]()


def _head(which, c, dev):
    from multimodaltraj_2_amd.fullcov import FullCovHead
    from multimodaltraj_2_amd.mixture import MixtureHead
    from multimodaltraj_2_amd.nll import GaussianHead
    if which == "per_step":
        h = GaussianHead(device=dev)
        h.head = _t(c["head"], dev)
    elif which == "fullcov":
        h = FullCovHead(device=dev)
        h.chol = _t(c["chol"], dev)
    else:
        h = MixtureHead.from_block(c["mix"], device=dev)
    return h


def _device_inputs(i, which, dev):
    """(head object, dict of device tensors) of case i."""
    if (i, which) not in _DEV:
        c = kc.inputs(i)
        t = {k: _t(c[k], dev) for k in ("pred", "targets", "n_active", "n_frames", "ped_mask")}
        _DEV[(i, which)] = (_head(which, c, dev), t)
    return _DEV[(i, which)]


def _key(i, which, seed):
    """The caches' key: the case's own seed (None), or another."""
    return (i, which) if seed is None else (i, which, seed)


def _run(i, which, dev, want_per_ped=True, seed=None):
    c = kc.inputs(i)
    h, t = _device_inputs(i, which, dev)
    r = h.sample_kin(t["pred"], t["targets"], t["n_active"], c["K"], c["B"],
                     seed=c["seed"] if seed is None else seed, n_frames=t["n_frames"], ped_mask=t["ped_mask"],
                     want_per_ped=want_per_ped, targets_shared=c["shared"])
    torch.cuda.synchronize()
    return r


_RES, _REF = {}, {}


def _result(i, which, dev, seed=None):
    key = _key(i, which, seed)
    if key not in _RES:
        _RES[key] = _run(i, which, dev, seed=seed)
    return _RES[key]


def _recount(i, which, dev, seed=None):
    """The checker over the device's own K draws (computed once)."""
    key = _key(i, which, seed)
    if key not in _REF:
        c = kc.inputs(i)
        h, t = _device_inputs(i, which, dev)
        s0 = c["seed"] if seed is None else seed
        draws = np.stack([h.sample(t["pred"], seed=(s0 + k) & MASK64).cpu().numpy()
                          for k in range(c["K"])])
        _REF[key] = kr.sample_kin_ref(draws.astype(np.float32), c["targets"], c["pairs"])
    return _REF[key]


def _check_against(per, sums, hist, tot, R, K, B, label):
    """The ranks, hist and tot equal to the checker's; the floats within TOL."""
    m = R["pairs"]
    want = R["per"]
    assert np.isfinite(per).all() and np.all(per[~m] == 0)
    off = per[..., :32] != want[..., :32]
    ties = int((R["fx"] == R["fy"][None]).sum())
    err = np.abs(per[..., 32:] - want[..., 32:]) / np.maximum(1.0, np.abs(want[..., 32:]))
    print(f"{label}: {int(m.sum())} pairs, ranks off the float32 restatement {int(off.sum())} of {32 * int(m.sum())} "
          f"(fp32 ties between a draw and the target {ties}), worst float error {err.max() if err.size else 0.0:.3g} "
          f"(tolerance {TOL})")
    np.testing.assert_array_equal(per[..., :32], want[..., :32])
    want_h, want_t = kr.hist_tot(want, m, K, B)
    np.testing.assert_array_equal(hist, want_h)
    np.testing.assert_array_equal(tot, want_t)
    assert np.all(err <= TOL), np.argwhere(err > TOL)[:5]
    n = m.sum(axis=(1, 2)).astype(np.float64)[:, None]
    serr = np.abs(sums - R["sums"]) / np.maximum(1.0, np.abs(R["sums"]))
    print(f"{label}: worst error of sums {serr.max() if serr.size else 0.0:.3g}")
    assert np.all(np.abs(sums - R["sums"]) <= TOL * n * np.maximum(1.0, np.abs(R["sums"])))


def _parity(dev, i, which, seed=None, label=""):
    c = kc.inputs(i)
    r, R = _result(i, which, dev, seed), _recount(i, which, dev, seed)
    per = r.per_ped.cpu().numpy().astype(np.float64)
    sums = r.sums.cpu().numpy().astype(np.float64)
    hist, tot = r.hist.cpu().numpy().astype(np.int64), r.tot.cpu().numpy()
    _check_against(per, sums, hist, tot, R, c["K"], c["B"], f"case {kc.IDS[i]} {which}{label}")
    # the result class's figures are the counts'
    assert r.k == c["K"] and r.bins == c["B"] and r.pairs == int(c["pairs"].sum())
    want = kr.figures(sums, hist, tot, c["K"])
    for g in kr.GROUPS:
        for name, fn in (("crps", r.crps), ("pit_mean", r.pit_mean), ("dev", r.dev), ("draw_mean", r.draw_mean),
                         ("target_mean", r.target_mean)):
            assert fn(g) == pytest.approx(want[g][name], rel=1e-12, abs=1e-12), (g, name)
        assert 0.0 <= r.dev(g) <= 1.0 and 0.0 <= r.pit_mean(g) <= 1.0


@pytest.mark.parametrize("i,which", ALL, ids=ALL_IDS)
def test_ranks_equal_and_sums_within_tolerance(gpu, i, which):
    _parity(gpu, i, which)


@pytest.mark.parametrize("which", kc.HEADS)
def test_seed_whose_low_word_carries(gpu, which):
    """Case k2 with the same assertions at seed A = 2^32 - 1, where draw 1's
    seed carries out of the low word: the launcher's split of the seed and
    drawn_lane's lo / hi arithmetic (csrc/g2k_drawn.h) against the samplers' at
    (seed + k) mod 2^64.  tests/test_sample_kin.py: the checker's integer
    outputs change when the carry is dropped."""
    _parity(gpu, kc.IDS.index("k2"), which, SEED_A, " seed A")


def _raw_call(i, which, dev, per_ped, sums, hist, tot, t=None, ws=None):
    """The entry point itself, on caller-made buffers."""
    from multimodaltraj_2_amd import _lib, kin
    from multimodaltraj_2_amd.frame_step import _ptr
    lib = kin.load()
    c = kc.inputs(i)
    h, t0 = _device_inputs(i, which, dev)
    t = t or dict(t0, params=_params(h, which))
    d = h._dims(t0["pred"])
    if c["shared"]:
        d.flags = _lib.STEP_TARGETS_SHARED
    need = int(lib.g2k_sample_kin_workspace_bytes(ctypes.byref(d), c["B"]))
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc_ = getattr(lib, STEMS[which] + "_f32")(ctypes.byref(d), _ptr(t["pred"]), _ptr(t["targets"]),
                                              _ptr(t["n_active"]), _ptr(t["n_frames"]), _ptr(t["ped_mask"]),
                                              _ptr(t["params"]), ctypes.c_uint64(c["seed"]), c["K"], c["B"],
                                              _ptr(per_ped), _ptr(sums), _ptr(hist), _ptr(tot), _ptr(ws), need,
                                              None)
    torch.cuda.synchronize()
    assert rc_ == 0, lib.g2k_last_error()
    return need


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))      # the bits


FOOT = [kc.IDS.index(n) for n in ("k2", "k20", "passes", "tail")]


@pytest.mark.parametrize("which", kc.HEADS)
@pytest.mark.parametrize("i", FOOT, ids=[kc.IDS[i] for i in FOOT])
def test_determinism_and_footprint(gpu, i, which):
    """Guarded, poisoned outputs: every element written, nothing outside; the
    bits of a second call and of the Python path; per_ped NULL leaves the bits
    of sums, hist and tot alone; non-pairs exactly zero."""
    c = kc.inputs(i)
    S, F, _, N = c["pred"].shape
    B = c["B"]
    ar = Arena(gpu)
    per = ar.alloc((S, F, N, 48), name="per_ped")
    sums, sums2 = ar.alloc((S, 16), name="sums"), ar.alloc((S, 16), name="sums2")
    hist, tot = ar.alloc((S, 32, B), torch.int32, name="hist"), ar.alloc((S, 8), torch.int64, name="tot")
    hist2, tot2 = ar.alloc((S, 32, B), torch.int32, name="hist2"), ar.alloc((S, 8), torch.int64, name="tot2")
    _raw_call(i, which, gpu, per, sums, hist, tot)
    ar.check_guards()
    assert all_written(per) and all_written(sums) and all_written(hist) and all_written(tot)
    r = _result(i, which, gpu)
    assert _same(per, r.per_ped) and _same(sums, r.sums) and torch.equal(hist, r.hist) and torch.equal(tot, r.tot)
    again = _run(i, which, gpu)
    assert _same(again.per_ped, r.per_ped) and _same(again.sums, r.sums)
    assert torch.equal(again.hist, r.hist) and torch.equal(again.tot, r.tot)
    _raw_call(i, which, gpu, None, sums2, hist2, tot2)
    ar.check_guards()
    assert all_written(sums2) and all_written(hist2) and all_written(tot2)
    assert _same(sums2, sums) and torch.equal(hist2, hist) and torch.equal(tot2, tot)
    no = _run(i, which, gpu, want_per_ped=False)
    assert no.per_ped is None and _same(no.sums, r.sums) and torch.equal(no.hist, r.hist) and torch.equal(no.tot, r.tot)
    assert bool((per[~_t(c["pairs"], gpu)] == 0).all())
    assert not bool(torch.isnan(per).any()) and not bool(torch.isnan(sums).any())   # the poison was never read
    assert bool((tot[:, 5:] == 0).all())


def test_no_frames_writes_zeros(gpu):
    """F = 0 with S > 0: sums, hist and tot are written, all zero."""
    from multimodaltraj_2_amd import _lib, kin
    from multimodaltraj_2_amd.frame_step import _ptr
    lib = kin.load()
    d = _lib.G2KDims(3, 0, 8, 12, 16, 64, 16, 8, 0)
    some = torch.zeros(64, device=gpu)                      # pred, targets, head: named, never read
    n_active = torch.full((3,), 16, dtype=torch.int32, device=gpu)
    ar = Arena(gpu)
    sums = ar.alloc((3, 16), name="sums")
    hist, tot = ar.alloc((3, 32, 7), torch.int32, name="hist"), ar.alloc((3, 8), torch.int64, name="tot")
    need = int(lib.g2k_sample_kin_workspace_bytes(ctypes.byref(d), 7))
    ws = ar.alloc((need,), torch.uint8, name="workspace")
    for stem in STEMS.values():
        rc_ = getattr(lib, stem + "_f32")(ctypes.byref(d), _ptr(some), _ptr(some), _ptr(n_active), None, None,
                                          _ptr(some), ctypes.c_uint64(1), 20, 7, None, _ptr(sums), _ptr(hist),
                                          _ptr(tot), _ptr(ws), need, None)
        torch.cuda.synchronize()
        assert rc_ == 0, lib.g2k_last_error()
        ar.check_guards()
        assert all_written(sums) and not bool(sums.any()) and not bool(hist.any()) and not bool(tot.any())
        sums.fill_(5)
        hist.fill_(5)
        tot.fill_(5)


@pytest.mark.parametrize("which", ("per_step", "fullcov"))
def test_identical_draws(gpu, which):
    """sigma = 0 (log sigma = -200; a zero factor): the K draws are the
    prediction itself: p_g = 0, d_g the prediction's feature, every rank 0 or
    K, and everything the checker's on the prediction repeated K times."""
    from multimodaltraj_2_amd.fullcov import FullCovHead
    from multimodaltraj_2_amd.nll import GaussianHead
    K, B, N = 20, 21, 6
    if which == "per_step":
        h = GaussianHead(log_sigma=-200.0, device=gpu)
    else:
        h = FullCovHead(device=gpu)
        h.chol = torch.zeros((24, 24), device=gpu)
    rng = np.random.default_rng(17)
    pred = rng.standard_normal((1, 2, 24, N)).astype(np.float32)
    pred[0, 1] = 3.0                                                 # a frame of pedestrians that stand still
    tg = kr.band_to_xy(pred).astype(np.float32) + (0.3 * rng.standard_normal((1, 2, N, L, 2))).astype(np.float32)
    tg[0, 1, :3] = kr.band_to_xy(pred)[0, 1, :3]                     # ... three of the targets too
    r = h.sample_kin(_t(pred, gpu), _t(tg, gpu), torch.full((1,), N, dtype=torch.int32, device=gpu), K, B,
                     want_per_ped=True)
    per = r.per_ped.cpu().numpy().astype(np.float64)
    pairs = np.ones((1, 2, N), bool)
    R = kr.sample_kin_ref(np.broadcast_to(pred[None], (K,) + pred.shape).copy(), tg, pairs)
    assert set(np.unique(per[..., :32])) <= {0.0, float(K)}
    np.testing.assert_array_equal(per[..., :32], R["per"][..., :32])
    assert not per[..., 36:40].any()                                 # p_g: the draws are one point
    fp = kr.features(kr.band_to_xy(pred)).astype(np.float64)         # [1, 2, N, 32]
    dg = np.stack([fp[..., sl].mean(axis=-1) for sl in kr.GROUPS.values()], axis=-1)
    np.testing.assert_allclose(per[..., 40:44], dg, rtol=TOL, atol=TOL)
    np.testing.assert_allclose(per[..., 32:], R["per"][..., 32:], rtol=TOL, atol=TOL)
    # standing still: len == 0, st = 1; the standing targets tie with the draws everywhere: rank 0
    assert np.all(np.abs(per[0, 1, :, 43] - 1.0) <= TOL) and np.all(per[0, 1, :3, 47] == 1.0)
    assert not per[0, 1, :3, :32].any()
    hist, tot = kr.hist_tot(per, pairs, K, B)
    np.testing.assert_array_equal(r.hist.cpu().numpy(), hist)
    np.testing.assert_array_equal(r.tot.cpu().numpy(), tot)
    assert not hist[:, :, 1:B - 1].any()


@pytest.mark.parametrize("which", kc.HEADS)
def test_at_minimum_alignment(gpu, which):
    """Each entry point at the weakest pointer alignment its header line
    states (targets 8, per_ped 16, sums 4, hist 4, tot 8, workspace 8) and every
    other pointer at its element's own (4; the mask 1): the bits of the aligned
    call."""
    i = kc.IDS.index("shared")
    c = kc.inputs(i)
    S, F, _, N = c["pred"].shape
    h, _ = _device_inputs(i, which, gpu)
    ar = Arena(gpu)
    t = dict(pred=ar.put(c["pred"], "pred", 4), targets=ar.put(c["targets"], "targets", 8),
             n_active=ar.put(c["n_active"], "n_active", 4), n_frames=ar.put(c["n_frames"], "n_frames", 4),
             ped_mask=ar.put(c["ped_mask"], "ped_mask", 1),
             params=ar.put(_params(h, which).cpu().numpy(), "params", 4))
    assert t["targets"].data_ptr() % 16 == 8 and t["pred"].data_ptr() % 16 == 4
    per = ar.alloc((S, F, N, 48), name="per_ped")
    sums = ar.alloc((S, 16), name="sums", offset=4)
    hist = ar.alloc((S, 32, c["B"]), torch.int32, name="hist", offset=4)
    tot = ar.alloc((S, 8), torch.int64, name="tot", offset=8)
    from multimodaltraj_2_amd import kin
    need = kin.load().g2k_sample_kin_workspace_bytes(ctypes.byref(h._dims(_t(c["pred"], "cpu"))), c["B"])
    ws = ar.alloc((need,), torch.uint8, name="workspace", offset=8)
    assert sums.data_ptr() % 8 == 4 and hist.data_ptr() % 8 == 4 and tot.data_ptr() % 16 == 8
    assert ws.data_ptr() % 16 == 8
    assert _raw_call(i, which, gpu, per, sums, hist, tot, t=t, ws=ws) == need
    ar.check_guards()
    r = _result(i, which, gpu)
    assert _same(per, r.per_ped) and _same(sums, r.sums) and torch.equal(hist, r.hist) and torch.equal(tot, r.tot)


def test_heads_are_told_apart_on_the_device(gpu):
    """tests/test_sample_kin.py's property test with the device's samplers and
    the fused call."""
    S, F, N, K, B, seed = (PROP[k] for k in ("S", "F", "N", "K", "B", "seed"))
    c = kc.inputs(kc.IDS.index("k20"))
    pred = _t(kc.property_setup(S, F, N), gpu)
    n_active = torch.full((S,), N, dtype=torch.int32, device=gpu)
    heads = {which: _head(which, c, gpu) for which in kc.HEADS}
    targets = {}
    for which, h in heads.items():
        y = h.sample(pred, seed=seed + K)                                   # [S, F, 24, N]
        targets[which] = torch.stack([y[:, :, :L], y[:, :, L:]], dim=-1).permute(0, 1, 3, 2, 4).contiguous()

    def score(target, scorer):
        r = heads[scorer].sample_kin(pred, targets[target], n_active, K, B, seed=seed)
        assert r.pairs == S * F * N
        return r.counts(), {g: dict(crps=r.crps(g), pit_mean=r.pit_mean(g)) for g in kr.GROUPS}
    property_check(score, "device: ")


def test_python_argument_checks(gpu):
    for which in kc.HEADS:
        h, t = _device_inputs(0, which, gpu)
        for k in (1, 256):
            with pytest.raises(ValueError, match="2..255"):
                h.sample_kin(t["pred"], t["targets"], t["n_active"], k)
        with pytest.raises(ValueError, match="a divisor of k \\+ 1"):
            h.sample_kin(t["pred"], t["targets"], t["n_active"], 20, 4)
        with pytest.raises(ValueError, match="targets must be"):
            h.sample_kin(t["pred"], t["targets"][:, :1], t["n_active"], 4)
        with pytest.raises(ValueError, match="n_active must be"):
            h.sample_kin(t["pred"], t["targets"], t["n_active"][:1], 4)


def test_evaluation_end_to_end(gpu, tmp_path, data_root):
    """The recipe of tests/test_sample_ranks_gpu.py::test_evaluation_end_to_end
    with --num_samples 20 --sample_kinematics 1, without and with
    --fullcov_head train and --mixture_head train: the new keys at the end of
    each head's block, finite and equal to a direct call on ``keep``'s tensors;
    the old keys and values unchanged, one more log line per head; without the
    flag the parent's keys; K = 1 with the flag raises."""
    from multimodaltraj_2_amd import checkpoint, evaluate
    from multimodaltraj_2_amd import train as tr
    from multimodaltraj_2_amd.argParser import ArgsParser
    from multimodaltraj_2_amd.fullcov import FullCovHead
    from multimodaltraj_2_amd.nll import GaussianHead
    argv = ["--data_root", data_root, "--leaveDataset", "2", "--n_max", "32", "--train_scenes", "64",
            "--train_batch", "32", "--num_epochs", "2", "--loss", "l2", "--num_samples", "20",
            "--mode", "train", "--save_dir", str(tmp_path), "--log_dir", str(tmp_path),
            "--device", "cuda:0"]
    args = ArgsParser().parser.parse_args(argv)
    assert args.sample_kinematics == 0 and args.kin_bins == 0
    tr.run_train_mode(args, gpu, log=lambda s: None)
    prm = checkpoint.load_params(checkpoint.read_state(str(tmp_path)), device=gpu)
    logs0, keep0 = [], {}
    res0 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs0.append, keep=keep0)
    assert list(res0) == ["scenes", "pairs", "K"] + list(evaluate.FIGURES)
    assert "kin" not in keep0 and not any("kinematics" in s for s in logs0)

    args.sample_kinematics = 1
    logs1, keep1 = [], {}
    res1 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs1.append, keep=keep1)
    assert list(res1) == list(res0) + list(evaluate.KIN_FIGURES)
    assert {k: res1[k] for k in res0} == res0 and logs1[:len(logs0)] == logs0 and len(logs1) == len(logs0) + 1
    assert logs1[-1].startswith("sample kinematics of the 20 draws on dataset 2: 21 bins")
    t = keep1["plan"].to_device(gpu, F=1)
    one = torch.ones(keep1["plan"].S, dtype=torch.int32, device=gpu)
    gh = GaussianHead(device=gpu)
    gh.head = keep1["head"]
    kw = dict(seed=args.sample_seed, n_frames=one, ped_mask=t["ped_mask"])
    direct = gh.sample_kin(keep1["pred"], t["targets"], t["n_active"], 20, **kw)
    want = evaluate.kin_figures(direct)
    for k in evaluate.KIN_FIGURES:
        print(f"evaluation {k}: {res1[k]:.8g}")
        assert np.isfinite(res1[k]) and res1[k] == want[k], k
    assert torch.equal(keep1["kin"].hist, direct.hist) and torch.equal(keep1["kin"].tot, direct.tot)
    assert _same(keep1["kin"].sums, direct.sums)
    assert direct.pairs == res1["pairs"] and keep1["kin"].per_ped is not None and direct.bins == 21
    assert f"{res1['kin_crps_acc']:.4f}" in logs1[-1]
    # after the rank figures when both are asked for
    args.sample_ranks = 1
    resr = evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
    assert list(resr) == list(res0) + list(evaluate.RANK_FIGURES) + list(evaluate.KIN_FIGURES)
    assert {k: resr[k] for k in res1} == res1
    args.sample_ranks = 0

    # --kin_bins; with both other heads; the flag off first: the parent's keys
    args.kin_bins = 7
    res7 = evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
    assert res7["kin_pit_acc"] == res1["kin_pit_acc"] and res7["kin_crps_speed"] == res1["kin_crps_speed"]
    assert res7["kin_dev_acc"] <= res1["kin_dev_acc"]               # merging bins cannot add distance
    args.sample_kinematics, args.kin_bins, args.fullcov_head, args.mixture_head = 0, 0, "train", "train"
    logs_off = []
    res_off = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs_off.append)
    assert list(res_off) == list(res0) + list(evaluate.FULLCOV_FIGURES) + list(evaluate.MIX_FIGURES)
    args.sample_kinematics = 1
    logs2, keep2 = [], {}
    res2 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs2.append, keep=keep2)
    assert list(res2) == (list(res1) + list(evaluate.FULLCOV_FIGURES) + list(evaluate.FULLCOV_KIN_FIGURES)
                          + list(evaluate.MIX_FIGURES) + list(evaluate.MIX_KIN_FIGURES))
    assert {k: res2[k] for k in res1} == res1 and {k: res2[k] for k in res_off} == res_off
    assert len(logs2) == len(logs_off) + 3
    assert [s for s in logs2 if "sample kinematics" not in s] == logs_off
    assert sum(s.startswith("full-covariance sample kinematics of the 20 draws on dataset 2:") for s in logs2) == 1
    assert logs2[-1].startswith("mixture sample kinematics of the 20 draws on dataset 2:")
    fc = FullCovHead(device=gpu)
    fc.chol = keep2["fullcov_chol"]
    fwant = evaluate.kin_figures(fc.sample_kin(keep2["pred"], t["targets"], t["n_active"], 20, **kw), "fullcov_")
    mdirect = keep2["mixture"]["head"].sample_kin(keep2["pred"], t["targets"], t["n_active"], 20, **kw)
    mwant = evaluate.kin_figures(mdirect, "mix_")
    for k, v in list(fwant.items()) + list(mwant.items()):
        print(f"evaluation {k}: {res2[k]:.8g}")
        assert np.isfinite(res2[k]) and res2[k] == v, k
    assert torch.equal(keep2["mixture"]["kin"].hist, mdirect.hist)
    assert keep2["fullcov"]["kin"].pairs == mdirect.pairs == res2["pairs"]
    # the CLI, and K outside 2..255
    cli = evaluate.main(argv + ["--sample_kinematics", "1", "--fullcov_head", "train", "--mixture_head", "train"],
                        log=lambda s: None)
    assert list(cli) == list(res2) and [cli[k] for k in res2] == [res2[k] for k in res2]
    for k in (1, 256):
        args.num_samples = k
        with pytest.raises(ValueError, match="2 <= K <= 255"):
            evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
