"""GPU: the fused couple-distance scores (g2k_couple_scores_f32,
g2k_fullcov_couple_scores_f32, g2k_mix_couple_scores_f32, csrc/g2k_couples.hip;
the three heads' ``couple_scores``; evaluate.py) against the checker
tests/couples_ref.py fed with the DEVICE's own draws (the head's sampler called
K times at seeds seed + k), so that the comparison sees the kernel's arithmetic
and not the draws'.  PARITY UNPINNED against the reference (it has no
probabilistic head).  The features are single fp32 operations in a stated
order, which the checker restates in np.float32: per_couple, per_frame_i, hist
and tot must be EQUAL.  The fp32 sums are held to scores_ref.TOL * max(1,
|ref|) times the couples summed, against the checker's float64 sums.  The cases
(tests/couples_cases.py) are the smallest that reach each path."""
import ctypes

import numpy as np
import pytest
import torch

from tests import couples_cases as cc
from tests import couples_ref as cr
from tests.abi_arena import Arena, all_written
from tests.bestk_ref import BOUNDARY_SEEDS, MASK64
from tests.scores_ref import TOL
from tests.test_couple_scores import PROP, property_check, property_head, property_targets

pytestmark = pytest.mark.gpu
ALL = [(i, w) for i in range(len(cc.CASES)) for w in cc.HEADS]
ALL_IDS = [f"{cc.IDS[i]}-{w}" for i, w in ALL]
STEMS = {"per_step": "g2k_couple_scores", "fullcov": "g2k_fullcov_couple_scores", "mix": "g2k_mix_couple_scores"}
L = 12
INF = float("inf")


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
        c = cc.inputs(i)
        t = {k: _t(c[k], dev) for k in ("pred", "targets", "n_active", "n_frames", "ped_mask")}
        _DEV[(i, which)] = (_head(which, c, dev), t)
    return _DEV[(i, which)]


def _reach(c):
    return None if np.isinf(c["reach"]) else c["reach"]


def _key(i, which, seed):
    """The caches' key: the case's own seed (None), or another."""
    return (i, which) if seed is None else (i, which, seed)


def _run(i, which, dev, want_per_couple=True, want_per_frame=True, k=None, bins=None, seed=None):
    c = cc.inputs(i)
    h, t = _device_inputs(i, which, dev)
    r = h.couple_scores(t["pred"], t["targets"], t["n_active"], k or c["K"], bins or c["B"],
                        seed=c["seed"] if seed is None else seed, reach=_reach(c), n_frames=t["n_frames"],
                        ped_mask=t["ped_mask"],
                        want_per_couple=want_per_couple, want_per_frame=want_per_frame,
                        targets_shared=c["shared"])
    torch.cuda.synchronize()
    return r


_RES, _DRAWS, _REF = {}, {}, {}


def _result(i, which, dev, seed=None):
    key = _key(i, which, seed)
    if key not in _RES:
        _RES[key] = _run(i, which, dev, seed=seed)
    return _RES[key]


def _draws(i, which, dev, seed=None):
    """The device's own K draws [K, S, F, 24, N] float32 (made once)."""
    key = _key(i, which, seed)
    if key not in _DRAWS:
        c = cc.inputs(i)
        h, t = _device_inputs(i, which, dev)
        s0 = c["seed"] if seed is None else seed
        _DRAWS[key] = np.stack([h.sample(t["pred"], seed=(s0 + k) & MASK64).cpu().numpy()
                                for k in range(c["K"])]).astype(np.float32)
    return _DRAWS[key]


def _recount(i, which, dev, seed=None):
    """The checker over the device's own K draws (computed once)."""
    key = _key(i, which, seed)
    if key not in _REF:
        c = cc.inputs(i)
        _REF[key] = cr.couple_scores_ref(_draws(i, which, dev, seed), c["targets"], c["pred"], c["members"],
                                         c["K"], c["B"], c["reach"])
    return _REF[key]


def _check_against(r, R, label):
    """per_couple, per_frame_i, hist and tot equal to the checker's; the floats within TOL."""
    pc, pi = r.per_couple.cpu().numpy().astype(np.int64), r.per_frame_i.cpu().numpy().astype(np.int64)
    pf, sums = r.per_frame_f.cpu().numpy().astype(np.float64), r.sums.cpu().numpy().astype(np.float64)
    hist, tot = r.hist.cpu().numpy().astype(np.int64), r.tot.cpu().numpy()
    off = int((pc != R["per_couple"]).sum())
    n = R["per_frame_i"][..., :1].astype(np.float64)
    err = np.abs(pf - R["per_frame_f"]) / np.maximum(1.0, np.abs(R["per_frame_f"]))
    serr = np.abs(sums - R["sums"]) / np.maximum(1.0, np.abs(R["sums"]))
    print(f"{label}: {int(R['tot'][:, 0].sum())} couples scored of {int(R['tot'][:, 3].sum())}, per_couple off "
          f"the float32 restatement {off} (fp32 ties between a draw and the target {R['ties']}), worst error "
          f"of per_frame_f {err.max() if err.size else 0.0:.3g}, per couple summed "
          f"{(err / np.maximum(1.0, n)).max() if err.size else 0.0:.3g}, of sums "
          f"{serr.max() if serr.size else 0.0:.3g} (tolerance {TOL} a couple)")
    np.testing.assert_array_equal(pc, R["per_couple"])
    np.testing.assert_array_equal(pi, R["per_frame_i"])
    np.testing.assert_array_equal(hist, R["hist"])
    np.testing.assert_array_equal(tot, R["tot"])
    assert np.isfinite(pf).all() and np.isfinite(sums).all()
    assert np.all(np.abs(pf - R["per_frame_f"]) <= TOL * n * np.maximum(1.0, np.abs(R["per_frame_f"])))
    ns = R["tot"][:, :1].astype(np.float64)
    assert np.all(np.abs(sums - R["sums"]) <= TOL * ns * np.maximum(1.0, np.abs(R["sums"])))


def _parity(dev, i, which, seed=None, label=""):
    c = cc.inputs(i)
    r, R = _result(i, which, dev, seed), _recount(i, which, dev, seed)
    _check_against(r, R, f"case {cc.IDS[i]} {which}{label}")
    if cc.IDS[i] == "none":
        assert r.couples == 0 and r.member_couples > 0 and np.isnan(r.crps("min"))
    if cc.IDS[i] in ("reach", "shared", "deal"):
        assert 0 < r.couples < r.member_couples
    # the result class's figures are the counts'
    assert r.k == c["K"] and r.bins == c["B"] and r.couples == int(R["tot"][:, 0].sum())
    want = cr.figures(r.sums.cpu().numpy().astype(np.float64), r.hist.cpu().numpy(), r.tot.cpu().numpy(), c["K"])
    for g in cr.FEATURES:
        for name, fn in (("crps", r.crps), ("pit_mean", r.pit_mean), ("dev", r.dev), ("draw_mean", r.draw_mean),
                         ("target_mean", r.target_mean)):
            got, exp = fn(g), want[g][name]
            assert (np.isnan(got) and np.isnan(exp)) or got == pytest.approx(exp, rel=1e-12, abs=1e-12), (g, name)
        if r.couples:
            assert 0.0 <= r.dev(g) <= 1.0 and 0.0 <= r.pit_mean(g) <= 1.0


@pytest.mark.parametrize("i,which", ALL, ids=ALL_IDS)
def test_ranks_equal_and_sums_within_tolerance(gpu, i, which):
    _parity(gpu, i, which)


@pytest.mark.parametrize("which", cc.HEADS)
@pytest.mark.parametrize("at", BOUNDARY_SEEDS)
def test_seed_whose_low_word_carries(gpu, at, which):
    """Case k2 with the same assertions at the seeds where draw 1's seed carries
    out of the low word (A = 2^32 - 1) and wraps to 0 (W = 2^64 - 1): the kernel's
    own lo / hi arithmetic (csrc/g2k_couples.hip) against the samplers' at (seed +
    k) mod 2^64.  tests/test_couple_scores.py: the checker's integer outputs
    change when the carry is dropped.  The coupled head's:
    tests/test_coupled_head_gpu.py."""
    _parity(gpu, cc.IDS.index("k2"), which, BOUNDARY_SEEDS[at], f" seed {at}")


def _raw_call(i, which, dev, pc, pf, pi, sums, hist, tot, t=None, ws=None, reach=None, dims=None):
    """The entry point itself, on caller-made buffers."""
    from multimodaltraj_2_amd import _lib, couples
    from multimodaltraj_2_amd.frame_step import _ptr
    lib = couples.load()
    c = cc.inputs(i)
    h, t0 = _device_inputs(i, which, dev)
    t = t or dict(t0, params=_params(h, which))
    d = h._dims(t0["pred"])
    if c["shared"]:
        d.flags = _lib.STEP_TARGETS_SHARED
    need = int(lib.g2k_couple_scores_workspace_bytes(ctypes.byref(d), c["K"], c["B"]))
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc_ = getattr(lib, STEMS[which] + "_f32")(ctypes.byref(d), _ptr(t["pred"]), _ptr(t["targets"]),
                                              _ptr(t["n_active"]), _ptr(t["n_frames"]), _ptr(t["ped_mask"]),
                                              _ptr(t["params"]), ctypes.c_uint64(c["seed"]), c["K"], c["B"],
                                              c["reach"] if reach is None else reach, _ptr(pc), _ptr(pf),
                                              _ptr(pi), _ptr(sums), _ptr(hist), _ptr(tot), _ptr(ws), need, None)
    torch.cuda.synchronize()
    assert rc_ == 0, lib.g2k_last_error()
    return need


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))      # the bits


FOOT = [cc.IDS.index(n) for n in ("k2", "k20", "reach", "k23")]


@pytest.mark.parametrize("which", cc.HEADS)
@pytest.mark.parametrize("i", FOOT, ids=[cc.IDS[i] for i in FOOT])
def test_determinism_and_footprint(gpu, i, which):
    """Guarded, poisoned outputs: every element written, nothing outside; the
    bits of a second call and of the Python path; each optional output NULL
    leaves the bits of the others alone; what is no scored couple exactly
    zero."""
    c = cc.inputs(i)
    S, F, _, N = c["pred"].shape
    B = c["B"]
    ar = Arena(gpu)

    def outs(tag):
        return dict(pc=ar.alloc((S, F, N, N), torch.int32, name="per_couple" + tag),
                    pf=ar.alloc((S, F, 8), name="per_frame_f" + tag),
                    pi=ar.alloc((S, F, 4), torch.int32, name="per_frame_i" + tag),
                    sums=ar.alloc((S, 8), name="sums" + tag), hist=ar.alloc((S, 2, B), torch.int32, name="hist" + tag),
                    tot=ar.alloc((S, 4), torch.int64, name="tot" + tag))
    o = outs("")
    _raw_call(i, which, gpu, **o)
    ar.check_guards()
    assert all(all_written(v) for v in o.values())
    r = _result(i, which, gpu)
    assert torch.equal(o["pc"], r.per_couple) and _same(o["pf"], r.per_frame_f) and torch.equal(o["pi"], r.per_frame_i)
    assert _same(o["sums"], r.sums) and torch.equal(o["hist"], r.hist) and torch.equal(o["tot"], r.tot)
    again = _run(i, which, gpu)
    assert torch.equal(again.per_couple, r.per_couple) and _same(again.per_frame_f, r.per_frame_f)
    assert _same(again.sums, r.sums) and torch.equal(again.hist, r.hist) and torch.equal(again.tot, r.tot)
    for drop in ("pc", "pf", "pi", "all"):
        o2 = outs("_" + drop)
        args = {k: (None if (k == drop or (drop == "all" and k in ("pc", "pf", "pi"))) else v) for k, v in o2.items()}
        _raw_call(i, which, gpu, **args)
        ar.check_guards()
        for k, v in args.items():
            if v is None:
                continue
            assert all_written(v), (drop, k)
            assert torch.equal(v.view(torch.int32), o[k].view(torch.int32)), (drop, k)
    no = _run(i, which, gpu, want_per_couple=False, want_per_frame=False)
    assert no.per_couple is None and no.per_frame_f is None and no.per_frame_i is None
    assert _same(no.sums, r.sums) and torch.equal(no.hist, r.hist) and torch.equal(no.tot, r.tot)
    # what is no member couple a < b: zero
    m = _t(c["members"], gpu)
    couple = (m[:, :, :, None] & m[:, :, None, :]) & torch.ones((N, N), dtype=torch.bool, device=gpu).triu(1)
    assert bool((o["pc"][~couple] == 0).all())
    assert not bool(torch.isnan(o["pf"]).any()) and not bool(torch.isnan(o["sums"]).any())   # the poison was never read
    P = c["members"].sum(axis=2)
    assert bool((o["pf"][_t(P < 2, gpu)] == 0).all()) and bool((o["pi"][_t(P < 2, gpu)] == 0).all())


def test_no_frames_writes_zeros(gpu):
    """F = 0 with S > 0: sums, hist and tot are written, all zero."""
    from multimodaltraj_2_amd import _lib, couples
    from multimodaltraj_2_amd.frame_step import _ptr
    lib = couples.load()
    d = _lib.G2KDims(3, 0, 8, 12, 16, 64, 16, 8, 0)
    some = torch.zeros(64, device=gpu)                      # pred, targets, head: named, never read
    n_active = torch.full((3,), 16, dtype=torch.int32, device=gpu)
    ar = Arena(gpu)
    sums = ar.alloc((3, 8), name="sums")
    hist, tot = ar.alloc((3, 2, 7), torch.int32, name="hist"), ar.alloc((3, 4), torch.int64, name="tot")
    need = int(lib.g2k_couple_scores_workspace_bytes(ctypes.byref(d), 20, 7))
    ws = ar.alloc((need,), torch.uint8, name="workspace")
    for stem in STEMS.values():
        rc_ = getattr(lib, stem + "_f32")(ctypes.byref(d), _ptr(some), _ptr(some), _ptr(n_active), None, None,
                                          _ptr(some), ctypes.c_uint64(1), 20, 7, INF, None, None, None,
                                          _ptr(sums), _ptr(hist), _ptr(tot), _ptr(ws), need, None)
        torch.cuda.synchronize()
        assert rc_ == 0, lib.g2k_last_error()
        ar.check_guards()
        assert all_written(sums) and all_written(hist) and all_written(tot)
        assert not bool(sums.any()) and not bool(hist.any()) and not bool(tot.any())
        sums.fill_(5)
        hist.fill_(5)
        tot.fill_(5)


@pytest.mark.parametrize("which", cc.HEADS)
def test_at_minimum_alignment(gpu, which):
    """Each entry point at the weakest pointer alignment its header line
    states (targets 8, per_couple 4, per_frame_f 4, per_frame_i 4, sums 4, hist
    4, tot 8, workspace 4) and every other pointer at its element's own (4; the
    mask 1): the bits of the aligned call."""
    from multimodaltraj_2_amd import couples
    i = cc.IDS.index("shared")
    c = cc.inputs(i)
    S, F, _, N = c["pred"].shape
    h, _ = _device_inputs(i, which, gpu)
    ar = Arena(gpu)
    t = dict(pred=ar.put(c["pred"], "pred", 4), targets=ar.put(c["targets"], "targets", 8),
             n_active=ar.put(c["n_active"], "n_active", 4), n_frames=ar.put(c["n_frames"], "n_frames", 4),
             ped_mask=ar.put(c["ped_mask"], "ped_mask", 1),
             params=ar.put(_params(h, which).cpu().numpy(), "params", 4))
    assert t["targets"].data_ptr() % 16 == 8 and t["pred"].data_ptr() % 16 == 4
    pc = ar.alloc((S, F, N, N), torch.int32, name="per_couple", offset=4)
    pf = ar.alloc((S, F, 8), name="per_frame_f", offset=4)
    pi = ar.alloc((S, F, 4), torch.int32, name="per_frame_i", offset=4)
    sums = ar.alloc((S, 8), name="sums", offset=4)
    hist = ar.alloc((S, 2, c["B"]), torch.int32, name="hist", offset=4)
    tot = ar.alloc((S, 4), torch.int64, name="tot", offset=8)
    need = couples.load().g2k_couple_scores_workspace_bytes(ctypes.byref(h._dims(_t(c["pred"], "cpu"))), c["K"],
                                                            c["B"])
    ws = ar.alloc((need,), torch.uint8, name="workspace", offset=4)
    for v in (pc, pf, pi, sums, hist, ws):
        assert v.data_ptr() % 8 == 4
    assert tot.data_ptr() % 16 == 8
    assert _raw_call(i, which, gpu, pc, pf, pi, sums, hist, tot, t=t, ws=ws) == need
    ar.check_guards()
    r = _result(i, which, gpu)
    assert torch.equal(pc, r.per_couple) and _same(pf, r.per_frame_f) and torch.equal(pi, r.per_frame_i)
    assert _same(sums, r.sums) and torch.equal(hist, r.hist) and torch.equal(tot, r.tot)


@pytest.mark.parametrize("which", cc.HEADS)
def test_first_draws_of_k_are_the_draws_of_fewer(gpu, which):
    """Draw k does not depend on K: the call at K' = 6 (B 7) on case k20's
    inputs is the checker's on the first six of the device's twenty draws."""
    i = cc.IDS.index("k20")
    c = cc.inputs(i)
    r = _run(i, which, gpu, k=6, bins=7)
    R = cr.couple_scores_ref(_draws(i, which, gpu)[:6], c["targets"], c["pred"], c["members"], 6, 7, c["reach"])
    _check_against(r, R, f"case k20 at K' = 6, {which}")
    assert not torch.equal(r.per_couple, _result(i, which, gpu).per_couple)


@pytest.mark.parametrize("which", cc.HEADS)
def test_every_couple_is_joint_eval_s(gpu, which):
    """reach = +inf scores every member couple, and they are joint_eval's PP."""
    for name in ("k20", "k23", "n256"):
        i = cc.IDS.index(name)
        c = cc.inputs(i)
        assert np.isinf(c["reach"])
        h, t = _device_inputs(i, which, gpu)
        r = _result(i, which, gpu)
        j = h.joint_eval(t["pred"], t["targets"], t["n_active"], 2, 0.1, seed=c["seed"], n_frames=t["n_frames"],
                         ped_mask=t["ped_mask"], targets_shared=c["shared"])
        assert torch.equal(r.tot[:, 3], r.tot[:, 0]) and torch.equal(r.tot[:, 3], j.sums_i[:, 1])
        assert torch.equal(r.per_frame_i[..., 3], j.per_frame_i[..., 1])
        assert r.member_couples == j.ped_pairs == r.couples > 0


def test_coupled_targets_are_told_apart_on_the_device(gpu):
    """tests/test_couple_scores.py's property test with the device's sampler
    and the fused call."""
    from multimodaltraj_2_amd.nll import GaussianHead
    S, F, N, K, B, seed = (PROP[k] for k in ("S", "F", "N", "K", "B", "seed"))
    pred_h = cc.property_setup(S, F, N, PROP["side"])
    pred = _t(pred_h, gpu)
    n_active = torch.full((S,), N, dtype=torch.int32, device=gpu)
    h = GaussianHead(device=gpu)
    h.head = _t(property_head(), gpu)

    def score(kind):
        if kind == "matched":
            y = h.sample(pred, seed=seed + K)                                   # [S, F, 24, N]
            tg = torch.stack([y[:, :, :L], y[:, :, L:]], dim=-1).permute(0, 1, 3, 2, 4).contiguous()
        else:
            tg = _t(property_targets(pred_h, kind), gpu)
        r = h.couple_scores(pred, tg, n_active, K, B, seed=seed)
        assert r.couples == r.member_couples == S * F * N * (N - 1) // 2
        return {g: dict(dev=r.dev(g), crps=r.crps(g), pit_mean=r.pit_mean(g)) for g in cr.FEATURES}
    property_check(score, "device: ")


def test_python_argument_checks(gpu):
    for which in cc.HEADS:
        h, t = _device_inputs(0, which, gpu)
        for k in (1, 65):
            with pytest.raises(ValueError, match="2..64"):
                h.couple_scores(t["pred"], t["targets"], t["n_active"], k)
        with pytest.raises(ValueError, match="a divisor of k \\+ 1"):
            h.couple_scores(t["pred"], t["targets"], t["n_active"], 20, 4)
        for bad in (0.0, -2.0, float("nan")):
            with pytest.raises(ValueError, match="reach"):
                h.couple_scores(t["pred"], t["targets"], t["n_active"], 20, reach=bad)
        with pytest.raises(ValueError, match="targets must be"):
            h.couple_scores(t["pred"], t["targets"][:, :1], t["n_active"], 4)
        with pytest.raises(ValueError, match="n_active must be"):
            h.couple_scores(t["pred"], t["targets"], t["n_active"][:1], 4)


def test_evaluation_end_to_end(gpu, tmp_path, data_root):
    """The recipe of tests/test_sample_kin_gpu.py::test_evaluation_end_to_end
    with --num_samples 20 --couple_scores 1, without and with --fullcov_head
    train and --mixture_head train: the new keys directly after each head's
    kinematic figures, equal to a direct call on ``keep``'s tensors; the old
    keys and values unchanged, one more log line per head; without the flag the
    parent's keys; K outside 2..64 with the flag raises."""
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
    assert args.couple_scores == 0 and args.couple_bins == 0 and args.couple_reach == 0.0
    tr.run_train_mode(args, gpu, log=lambda s: None)
    prm = checkpoint.load_params(checkpoint.read_state(str(tmp_path)), device=gpu)
    args.sample_kinematics = 1
    logs0, keep0 = [], {}
    res0 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs0.append, keep=keep0)
    assert list(res0) == ["scenes", "pairs", "K"] + list(evaluate.FIGURES) + list(evaluate.KIN_FIGURES)
    assert "couples" not in keep0 and not any("couple scores" in s for s in logs0)

    args.couple_scores = 1
    logs1, keep1 = [], {}
    res1 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs1.append, keep=keep1)
    assert list(res1) == list(res0) + list(evaluate.CPL_FIGURES)
    assert {k: res1[k] for k in res0} == res0 and logs1[:len(logs0)] == logs0 and len(logs1) == len(logs0) + 1
    assert logs1[-1].startswith("couple scores of the 20 joint draws on dataset 2:")
    t = keep1["plan"].to_device(gpu, F=1)
    one = torch.ones(keep1["plan"].S, dtype=torch.int32, device=gpu)
    gh = GaussianHead(device=gpu)
    gh.head = keep1["head"]
    kw = dict(seed=args.sample_seed, n_frames=one, ped_mask=t["ped_mask"])
    direct = gh.couple_scores(keep1["pred"], t["targets"], t["n_active"], 20, **kw)
    want = evaluate.couple_figures(direct)
    for k in evaluate.CPL_FIGURES:
        print(f"evaluation {k}: {res1[k]:.8g}")
        assert res1[k] == want[k] or (np.isnan(res1[k]) and np.isnan(want[k])), k
    assert torch.equal(keep1["couples"].hist, direct.hist) and torch.equal(keep1["couples"].tot, direct.tot)
    assert _same(keep1["couples"].sums, direct.sums)
    assert keep1["couples"].per_couple is not None and direct.bins == 21 and direct.couples == direct.member_couples
    je = gh.joint_eval(keep1["pred"], t["targets"], t["n_active"], 2, 0.1, **kw)
    assert res1["cpl_couples"] == je.ped_pairs
    # --couple_bins and --couple_reach
    args.couple_bins, args.couple_reach = 7, 2.0
    res7 = evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
    assert res7["cpl_couples"] <= res1["cpl_couples"]
    near = gh.couple_scores(keep1["pred"], t["targets"], t["n_active"], 20, 7, reach=2.0, **kw)
    assert res7["cpl_couples"] == near.couples and {k: res7[k] for k in res0} == res0
    # with both other heads; the flag off first: the parent's keys
    args.couple_scores, args.couple_bins, args.couple_reach = 0, 0, 0.0
    args.fullcov_head, args.mixture_head = "train", "train"
    logs_off = []
    res_off = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs_off.append)
    assert list(res_off) == (list(res0) + list(evaluate.FULLCOV_FIGURES) + list(evaluate.FULLCOV_KIN_FIGURES)
                             + list(evaluate.MIX_FIGURES) + list(evaluate.MIX_KIN_FIGURES))
    args.couple_scores = 1
    logs2, keep2 = [], {}
    res2 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs2.append, keep=keep2)
    assert list(res2) == (list(res1) + list(evaluate.FULLCOV_FIGURES) + list(evaluate.FULLCOV_KIN_FIGURES)
                          + list(evaluate.FULLCOV_CPL_FIGURES) + list(evaluate.MIX_FIGURES)
                          + list(evaluate.MIX_KIN_FIGURES) + list(evaluate.MIX_CPL_FIGURES))
    assert {k: res2[k] for k in res_off} == res_off
    assert len(logs2) == len(logs_off) + 3 and [s for s in logs2 if "couple scores" not in s] == logs_off
    assert sum(s.startswith("full-covariance couple scores of the 20 joint draws on dataset 2:") for s in logs2) == 1
    assert logs2[-1].startswith("mixture couple scores of the 20 joint draws on dataset 2:")
    fc = FullCovHead(device=gpu)
    fc.chol = keep2["fullcov_chol"]
    fwant = evaluate.couple_figures(fc.couple_scores(keep2["pred"], t["targets"], t["n_active"], 20, **kw), "fullcov_")
    mdirect = keep2["mixture"]["head"].couple_scores(keep2["pred"], t["targets"], t["n_active"], 20, **kw)
    mwant = evaluate.couple_figures(mdirect, "mix_")
    for k, v in list(fwant.items()) + list(mwant.items()):
        print(f"evaluation {k}: {res2[k]:.8g}")
        assert res2[k] == v or (np.isnan(res2[k]) and np.isnan(v)), k
    assert torch.equal(keep2["mixture"]["couples"].hist, mdirect.hist)
    assert keep2["fullcov"]["couples"].couples == mdirect.couples == res2["cpl_couples"]
    args.sample_kinematics = 0
    for k in (1, 65):
        args.num_samples = k
        with pytest.raises(ValueError, match="2 <= K <= 64"):
            evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
