"""GPU: the fused scene-level rank calibration (g2k_scene_ranks_f32,
g2k_fullcov_scene_ranks_f32, g2k_mix_scene_ranks_f32, g2k_coupled_scene_ranks_f32,
csrc/g2k_scene_ranks.hip; the four heads' ``scene_ranks``; evaluate.py) against
the checker tests/scene_ranks_ref.py fed with the DEVICE's own draws (the head's
sampler called K times at seeds seed + k), so that the comparison sees the
kernel's arithmetic and not the draws'.  PARITY UNPINNED against the reference
(it has no probabilistic head).  Both sides are double on the same float32
values, so only the summation order differs: the floats are held to 1e-12 max(1,
|ref|), and each rank to the interval [#{g_k < g_K (1 - 1e-12)}, #{g_k <= g_K
(1 + 1e-12)}]; at most 1 rank in 1000 may have an interval that holds more than
one value, else the test fails as untestable.  hist and tot must equal the
ranks' own recount.  The cases (tests/scene_ranks_cases.py) are the smallest
that reach each path."""
import ctypes

import numpy as np
import pytest
import torch

from tests import couples_cases as cc
from tests import scene_ranks_cases as sc
from tests import scene_ranks_ref as sr
from tests.abi_arena import Arena, all_written
from tests.bestk_ref import BOUNDARY_SEEDS, MASK64

pytestmark = pytest.mark.gpu
ALL = [(i, w) for i in range(len(sc.CASES)) for w in sc.HEADS]
ALL_IDS = [f"{sc.IDS[i]}-{w}" for i, w in ALL]
STEMS = {"per_step": "g2k_scene_ranks", "fullcov": "g2k_fullcov_scene_ranks", "mix": "g2k_mix_scene_ranks",
         "coupled": "g2k_coupled_scene_ranks"}
L = 12
TOL = 1e-12


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _params(h, which):
    return {"per_step": lambda: h.head, "fullcov": lambda: h.chol, "mix": lambda: h.params,
            "coupled": lambda: h.cpl}[which]()


def _head(which, c, dev):
    from multimodaltraj_2_amd.coupled import CoupledHead
    from multimodaltraj_2_amd.fullcov import FullCovHead
    from multimodaltraj_2_amd.mixture import MixtureHead
    from multimodaltraj_2_amd.nll import GaussianHead
    if which == "per_step":
        h = GaussianHead(device=dev)
        h.head = _t(c["head"], dev)
    elif which == "fullcov":
        h = FullCovHead(device=dev)
        h.chol = _t(c["chol"], dev)                          # NaN above the diagonal: never read
    elif which == "mix":
        h = MixtureHead.from_block(c["mix"], device=dev)
    else:
        h = CoupledHead(device=dev)
        h.cpl = _t(c["cpl"], dev)                            # NaN above both diagonals
    return h


_DEV, _RES, _DRAWS, _REF = {}, {}, {}, {}


def _device_inputs(i, which, dev):
    """(head object, dict of device tensors) of case i."""
    if (i, which) not in _DEV:
        c = sc.inputs(i)
        t = {k: _t(c[k], dev) for k in ("pred", "targets", "n_active", "n_frames", "ped_mask")}
        _DEV[(i, which)] = (_head(which, c, dev), t)
    return _DEV[(i, which)]


def _key(i, which, seed):
    """The caches' key: the case's own seed (None), or another."""
    return (i, which) if seed is None else (i, which, seed)


def _run(i, which, dev, want_per_frame=True, k=None, bins=None, stream=None, seed=None):
    c = sc.inputs(i)
    h, t = _device_inputs(i, which, dev)
    r = h.scene_ranks(t["pred"], t["targets"], t["n_active"], k or c["K"], bins or c["B"],
                      seed=c["seed"] if seed is None else seed,
                      n_frames=t["n_frames"], ped_mask=t["ped_mask"], want_per_frame=want_per_frame,
                      targets_shared=c["shared"], stream=stream)
    torch.cuda.synchronize()
    return r


def _result(i, which, dev, seed=None):
    key = _key(i, which, seed)
    if key not in _RES:
        _RES[key] = _run(i, which, dev, seed=seed)
    return _RES[key]


def _draws(i, which, dev, seed=None):
    """The device's own K joint draws [K, S, F, 24, N] float32 (made once)."""
    key = _key(i, which, seed)
    if key not in _DRAWS:
        c = sc.inputs(i)
        h, t = _device_inputs(i, which, dev)
        s0 = c["seed"] if seed is None else seed
        _DRAWS[key] = np.stack([h.sample(t["pred"], seed=(s0 + k) & MASK64).cpu().numpy()
                                for k in range(c["K"])]).astype(np.float32)
    return _DRAWS[key]


def _recount(i, which, dev, seed=None):
    """The checker over the device's own K draws (computed once)."""
    key = _key(i, which, seed)
    if key not in _REF:
        c = sc.inputs(i)
        _REF[key] = sr.scene_ranks_ref(_draws(i, which, dev, seed), c["targets"], c["pred"], c["members"],
                                       c["K"], c["B"])
    return _REF[key]


def _check_against(r, R, K, B, label):
    """The floats within TOL of the checker's, the ranks inside its intervals,
    hist and tot the ranks' own recount."""
    pi = r.per_frame_i.cpu().numpy().astype(np.int64)
    pd, sums = r.per_frame_d.cpu().numpy(), r.sums.cpu().numpy()
    hist, tot = r.hist.cpu().numpy().astype(np.int64), r.tot.cpu().numpy()
    err = np.abs(pd - R["per_frame_d"]) / np.maximum(1.0, np.abs(R["per_frame_d"]))
    serr = np.abs(sums - R["sums"]) / np.maximum(1.0, np.abs(R["sums"]))
    off = int((pi != R["per_frame_i"]).sum())
    print(f"{label}: {int(R['tot'][:, 0].sum())} scene-frames scored, worst error of per_frame_d "
          f"{err.max() if err.size else 0.0:.3g}, of sums {serr.max() if serr.size else 0.0:.3g} (tolerance "
          f"{TOL:g}); {R['ranks']} ranks, {off} off the checker's own, {R['wide']} with an interval of more "
          f"than one value")
    assert R["wide"] * 1000 <= R["ranks"], "untestable: too many ranks within 1e-12 of a draw"
    assert pd.dtype == np.float64 and np.isfinite(pd).all() and np.isfinite(sums).all()
    assert np.all(err <= TOL) and np.all(serr <= TOL)
    np.testing.assert_array_equal(pi[..., 0], R["per_frame_i"][..., 0])
    assert np.all(pi[..., 1:] >= R["lo"]) and np.all(pi[..., 1:] <= R["hi"])
    h2, t2 = sr.recount(pi, K, B)
    np.testing.assert_array_equal(hist, h2)
    np.testing.assert_array_equal(tot, t2)


def _parity(dev, i, which, seed=None, label=""):
    c = sc.inputs(i)
    r, R = _result(i, which, dev, seed), _recount(i, which, dev, seed)
    _check_against(r, R, c["K"], c["B"], f"case {sc.IDS[i]} {which}{label}")
    assert r.k == c["K"] and r.bins == c["B"] and r.frames == int((c["members"].sum(axis=2) >= 2).sum())
    # the result class's figures are the counts'
    want = sr.figures(r.sums.cpu().numpy(), r.hist.cpu().numpy(), r.tot.cpu().numpy(), c["K"])
    assert r.es == pytest.approx(want["es"], rel=1e-12) and r.es > 0.0
    for g in sr.FEATURES:
        assert r.dev(g) == pytest.approx(want[g]["dev"], abs=1e-12) and 0.0 <= r.dev(g) <= 1.0
        assert r.pit(g) == pytest.approx(want[g]["pit"], abs=1e-12) and 0.0 < r.pit(g) < 1.0
    for g in sr.FEATURES[1:]:
        assert r.draw(g) == pytest.approx(want[g]["draw"], rel=1e-12)
        assert r.target(g) == pytest.approx(want[g]["target"], rel=1e-12)


@pytest.mark.parametrize("i,which", ALL, ids=ALL_IDS)
def test_floats_within_tolerance_and_ranks_inside_their_intervals(gpu, i, which):
    _parity(gpu, i, which)


@pytest.mark.parametrize("at,which,row", sc.BOUNDARY, ids=sc.BOUNDARY_IDS)
def test_seed_whose_low_word_carries(gpu, at, which, row):
    """The same parity, same bounds, at the seeds where draw 1's seed carries
    out of the low word (A = 2^32 - 1) and wraps to 0 (W = 2^64 - 1): the kernel's
    own lo / hi arithmetic (csrc/g2k_scene_ranks.hip) against the samplers' at
    (seed + k) mod 2^64; for the coupled head the salt is XORed in after the
    carry.  tests/test_scene_ranks.py: the checker's outputs change when the
    carry is dropped."""
    _parity(gpu, sc.IDS.index(row), which, BOUNDARY_SEEDS[at], f" seed {at}")


def test_ranks_with_an_interval_of_more_than_one_value(gpu):
    """Over every case and head (computed above, or here): the count DESIGN
    records; zero is expected."""
    for i, which in ALL:
        _recount(i, which, gpu)
    own = [R for key, R in _REF.items() if len(key) == 2]             # the cases' own seeds
    ranks = sum(R["ranks"] for R in own)
    wide = sum(R["wide"] for R in own)
    print(f"{ranks} ranks on the device's draws, {wide} with an interval of more than one value")
    assert ranks == 252 and wide * 1000 <= ranks


def _raw_call(i, which, dev, pi, pd, sums, hist, tot, t=None, ws=None, dims=None, stream=None, sync=True):
    """The entry point itself, on caller-made buffers."""
    from multimodaltraj_2_amd import _lib, coupled, sceneranks
    from multimodaltraj_2_amd.frame_step import _ptr, _stream
    lib = coupled.load() if which == "coupled" else sceneranks.load()
    sceneranks.load()
    c = sc.inputs(i)
    h, t0 = _device_inputs(i, which, dev)
    t = t or dict(t0, params=_params(h, which))
    d = dims or h._dims(t0["pred"])
    if c["shared"]:
        d.flags = _lib.STEP_TARGETS_SHARED
    need = int(lib.g2k_scene_ranks_workspace_bytes(ctypes.byref(d), c["K"], c["B"]))
    if ws is None:
        ws = torch.empty(max(8, need), dtype=torch.uint8, device=dev)
    rc_ = getattr(lib, STEMS[which] + "_f32")(ctypes.byref(d), _ptr(t["pred"]), _ptr(t["targets"]),
                                              _ptr(t["n_active"]), _ptr(t["n_frames"]), _ptr(t["ped_mask"]),
                                              _ptr(t["params"]), ctypes.c_uint64(c["seed"]), c["K"], c["B"],
                                              _ptr(pi), _ptr(pd), _ptr(sums), _ptr(hist), _ptr(tot), _ptr(ws),
                                              need, _stream(stream))
    if sync:
        torch.cuda.synchronize()
    assert rc_ == 0, lib.g2k_last_error()
    return need


def _same(a, b):
    w = torch.int64 if a.element_size() == 8 else torch.int32
    return torch.equal(a.view(w), b.view(w))                          # the bits


def _outs(ar, S, F, B, tag="", offs=(0, 0, 0, 0, 0)):
    return dict(pi=ar.alloc((S, F, 4), torch.int32, name="per_frame_i" + tag, offset=offs[0]),
                pd=ar.alloc((S, F, 6), torch.float64, name="per_frame_d" + tag, offset=offs[1]),
                sums=ar.alloc((S, 6), torch.float64, name="sums" + tag, offset=offs[2]),
                hist=ar.alloc((S, 3, B), torch.int32, name="hist" + tag, offset=offs[3]),
                tot=ar.alloc((S, 4), torch.int64, name="tot" + tag, offset=offs[4]))


FOOT = [sc.IDS.index(n) for n in ("k2", "k20", "k32")]


@pytest.mark.parametrize("which", sc.HEADS)
@pytest.mark.parametrize("i", FOOT, ids=[sc.IDS[i] for i in FOOT])
def test_determinism_and_footprint(gpu, i, which):
    """Guarded, poisoned outputs: every element written, nothing outside; the
    bits of a second call and of the Python path; each optional output NULL
    leaves the bits of the others alone; unscored scene-frames exactly zero; the
    NaN poison of the inputs never read."""
    c = sc.inputs(i)
    S, F, _, N = c["pred"].shape
    B = c["B"]
    ar = Arena(gpu)
    o = _outs(ar, S, F, B)
    _raw_call(i, which, gpu, **o)
    ar.check_guards()
    assert all(all_written(v) for v in o.values())
    r = _result(i, which, gpu)
    assert torch.equal(o["pi"], r.per_frame_i) and _same(o["pd"], r.per_frame_d) and _same(o["sums"], r.sums)
    assert torch.equal(o["hist"], r.hist) and torch.equal(o["tot"], r.tot)
    again = _run(i, which, gpu)
    assert torch.equal(again.per_frame_i, r.per_frame_i) and _same(again.per_frame_d, r.per_frame_d)
    assert _same(again.sums, r.sums) and torch.equal(again.hist, r.hist) and torch.equal(again.tot, r.tot)
    for drop in ("pi", "pd", "all"):
        o2 = _outs(ar, S, F, B, "_" + drop)
        args = {k: (None if (k == drop or (drop == "all" and k in ("pi", "pd"))) else v) for k, v in o2.items()}
        _raw_call(i, which, gpu, **args)
        ar.check_guards()
        for k, v in args.items():
            if v is None:
                continue
            assert all_written(v), (drop, k)
            assert _same(v, o[k]), (drop, k)
    no = _run(i, which, gpu, want_per_frame=False)
    assert no.per_frame_i is None and no.per_frame_d is None
    assert _same(no.sums, r.sums) and torch.equal(no.hist, r.hist) and torch.equal(no.tot, r.tot)
    assert not bool(torch.isnan(o["pd"]).any()) and not bool(torch.isnan(o["sums"]).any())
    unscored = _t(c["members"].sum(axis=2) < 2, gpu)
    assert bool((o["pd"][unscored] == 0).all()) and bool((o["pi"][unscored] == 0).all())
    assert bool((o["pi"][~unscored][:, 0] >= 2).all())


def test_no_frames_writes_zeros(gpu):
    """F = 0 with S > 0: sums, hist and tot are written, all zero."""
    from multimodaltraj_2_amd import _lib, coupled, sceneranks
    from multimodaltraj_2_amd.frame_step import _ptr
    lib = coupled.load()
    sceneranks.load()
    d = _lib.G2KDims(3, 0, 8, 12, 16, 64, 16, 8, 0)
    some = torch.zeros(64, device=gpu)                      # pred, targets, head: named, never read
    n_active = torch.full((3,), 16, dtype=torch.int32, device=gpu)
    ar = Arena(gpu)
    sums = ar.alloc((3, 6), torch.float64, name="sums")
    hist, tot = ar.alloc((3, 3, 7), torch.int32, name="hist"), ar.alloc((3, 4), torch.int64, name="tot")
    need = int(lib.g2k_scene_ranks_workspace_bytes(ctypes.byref(d), 20, 7))
    assert need == 3 * 64
    ws = ar.alloc((need,), torch.uint8, name="workspace")
    for stem in STEMS.values():
        rc_ = getattr(lib, stem + "_f32")(ctypes.byref(d), _ptr(some), _ptr(some), _ptr(n_active), None, None,
                                          _ptr(some), ctypes.c_uint64(1), 20, 7, None, None, _ptr(sums),
                                          _ptr(hist), _ptr(tot), _ptr(ws), need, None)
        torch.cuda.synchronize()
        assert rc_ == 0, lib.g2k_last_error()
        ar.check_guards()
        assert all_written(sums) and all_written(hist) and all_written(tot)
        assert not bool(sums.any()) and not bool(hist.any()) and not bool(tot.any())
        sums.fill_(5)
        hist.fill_(5)
        tot.fill_(5)


@pytest.mark.parametrize("which", sc.HEADS)
def test_at_minimum_alignment(gpu, which):
    """Each entry point at the weakest pointer alignment its header line
    states (targets 8, per_frame_i 4, per_frame_d 8, sums 8, hist 4, tot 8,
    workspace 8) and every other pointer at its element's own (4; the mask 1):
    the bits of the aligned call."""
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
    o = _outs(ar, S, F, c["B"], offs=(4, 8, 8, 4, 8))
    ws = ar.alloc((S * F * 64,), torch.uint8, name="workspace", offset=8)
    for k in ("pi", "hist"):
        assert o[k].data_ptr() % 8 == 4
    for v in (o["pd"], o["sums"], o["tot"], ws):
        assert v.data_ptr() % 16 == 8
    assert _raw_call(i, which, gpu, t=t, ws=ws, **o) == S * F * 64
    ar.check_guards()
    r = _result(i, which, gpu)
    assert torch.equal(o["pi"], r.per_frame_i) and _same(o["pd"], r.per_frame_d) and _same(o["sums"], r.sums)
    assert torch.equal(o["hist"], r.hist) and torch.equal(o["tot"], r.tot)


@pytest.mark.parametrize("which", sc.HEADS)
def test_under_graph_capture(gpu, which):
    """The call is capturable and allocates nothing: captured on a side
    stream and replayed twice, the bits of the plain call."""
    i = sc.IDS.index("k20")
    c = sc.inputs(i)
    S, F, _, N = c["pred"].shape
    r = _result(i, which, gpu)
    o = dict(pi=torch.zeros((S, F, 4), dtype=torch.int32, device=gpu),
             pd=torch.zeros((S, F, 6), dtype=torch.float64, device=gpu),
             sums=torch.zeros((S, 6), dtype=torch.float64, device=gpu),
             hist=torch.zeros((S, 3, c["B"]), dtype=torch.int32, device=gpu),
             tot=torch.zeros((S, 4), dtype=torch.int64, device=gpu))
    ws = torch.empty(S * F * 64, dtype=torch.uint8, device=gpu)
    _device_inputs(i, which, gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        _raw_call(i, which, gpu, ws=ws, stream=torch.cuda.current_stream(), sync=False, **o)
    for _ in range(2):
        for v in o.values():
            v.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(o["pi"], r.per_frame_i) and _same(o["pd"], r.per_frame_d) and _same(o["sums"], r.sums)
        assert torch.equal(o["hist"], r.hist) and torch.equal(o["tot"], r.tot)


def test_coupled_without_a_shared_part_is_the_full_covariance_head(gpu):
    """Lb = 0: every output bit of g2k_coupled_scene_ranks_f32 is
    g2k_fullcov_scene_ranks_f32's with chol = Lw."""
    from multimodaltraj_2_amd.coupled import CoupledHead
    from multimodaltraj_2_amd.fullcov import FullCovHead
    for name in ("k20", "k64"):
        i = sc.IDS.index(name)
        c = sc.inputs(i)
        _, t = _device_inputs(i, "coupled", gpu)
        co, fc = CoupledHead(device=gpu), FullCovHead(device=gpu)
        co.cpl = _t(np.stack([c["cpl"][0], np.zeros((24, 24), np.float32)]), gpu)
        fc.chol = _t(c["cpl"][0], gpu)
        kw = dict(seed=c["seed"], n_frames=t["n_frames"], ped_mask=t["ped_mask"], want_per_frame=True)
        a = co.scene_ranks(t["pred"], t["targets"], t["n_active"], c["K"], c["B"], **kw)
        b = fc.scene_ranks(t["pred"], t["targets"], t["n_active"], c["K"], c["B"], **kw)
        assert torch.equal(a.per_frame_i, b.per_frame_i) and _same(a.per_frame_d, b.per_frame_d)
        assert _same(a.sums, b.sums) and torch.equal(a.hist, b.hist) and torch.equal(a.tot, b.tot)
        assert a.frames > 0
        # and with its shared part it is another law
        assert not _same(_result(i, "coupled", gpu).per_frame_d, b.per_frame_d)


@pytest.mark.parametrize("which", sc.HEADS)
def test_first_scene_does_not_depend_on_what_follows(gpu, which):
    """The first scene's results do not change when more scenes are appended:
    case k20's first scene alone against the whole launch."""
    i = sc.IDS.index("k20")
    c = sc.inputs(i)
    h, t = _device_inputs(i, which, gpu)
    r = _result(i, which, gpu)
    one = h.scene_ranks(t["pred"][:1].contiguous(), t["targets"][:1].contiguous(), t["n_active"][:1].contiguous(),
                        c["K"], c["B"], seed=c["seed"], n_frames=t["n_frames"][:1].contiguous(),
                        ped_mask=t["ped_mask"][:1].contiguous(), want_per_frame=True)
    assert torch.equal(one.per_frame_i, r.per_frame_i[:1]) and _same(one.per_frame_d, r.per_frame_d[:1].contiguous())
    assert _same(one.sums, r.sums[:1].contiguous()) and torch.equal(one.hist, r.hist[:1])
    assert torch.equal(one.tot, r.tot[:1]) and one.frames == 3


def test_the_coupled_head_is_calibrated_on_the_device(gpu):
    """tests/test_scene_ranks.py's property with the device's fits, samplers
    and the fused call: CoupledHead.fit and FullCovHead.fit on the first target
    set, scene_ranks on the second.  It cannot pass without the feature."""
    from multimodaltraj_2_amd.coupled import CoupledHead
    from multimodaltraj_2_amd.fullcov import FullCovHead
    S, F, N, K, B, seed = (sc.PROP[k] for k in ("S", "F", "N", "K", "B", "seed"))
    pred_h = cc.property_setup(S, F, N, sc.PROP["side"])
    pred = _t(pred_h, gpu)
    n_active = _t(sc.property_n_active(), gpu)
    fit_tg, score_tg = (_t(cc.coupled_targets(pred_h, sc.PROP["sigma"], sc.PROP["share"],
                                              rng_seed=sc.PROP[w + "_seed"]), gpu) for w in ("fit", "score"))
    co, fc = CoupledHead(device=gpu), FullCovHead(device=gpu)
    st = co.fit(pred, fit_tg, n_active)
    fc.fit(pred, fit_tg, n_active)
    print(f"device: fitted share {st.share:.4f}, clipped {co.clipped}")
    assert abs(st.share - sc.PROP["share"]) < 0.03

    def score(kind):
        h = co if kind == "coupled" else fc
        r = h.scene_ranks(pred, score_tg, n_active, K, B, seed=seed)
        assert r.frames == S * F
        fig = dict(frames=r.frames, es=r.es)
        for g in sr.FEATURES:
            fig[g] = dict(dev=r.dev(g), pit=r.pit(g))
        return fig
    sc.property_check(score, "device: ")


def test_python_argument_checks(gpu):
    for which in sc.HEADS:
        h, t = _device_inputs(0, which, gpu)
        for k in (1, 65):
            with pytest.raises(ValueError, match="2..64"):
                h.scene_ranks(t["pred"], t["targets"], t["n_active"], k)
        with pytest.raises(ValueError, match="a divisor of k \\+ 1"):
            h.scene_ranks(t["pred"], t["targets"], t["n_active"], 20, 4)
        with pytest.raises(ValueError, match="targets must be"):
            h.scene_ranks(t["pred"], t["targets"][:, :1], t["n_active"], 4)
        with pytest.raises(ValueError, match="n_active must be"):
            h.scene_ranks(t["pred"], t["targets"], t["n_active"][:1], 4)


def test_evaluation_end_to_end(gpu, tmp_path, data_root):
    """The recipe of tests/test_couple_scores_gpu.py::test_evaluation_end_to_end
    with --num_samples 20 --couple_scores 1 --scene_ranks 1, without and with
    the other three heads: the new keys directly after each head's
    couple-distance figures, equal to a direct call on ``keep``'s tensors; the
    old keys and values unchanged, one more log line per head; without the flag
    the parent's keys; the command line gives what the API gives."""
    from multimodaltraj_2_amd import checkpoint, evaluate
    from multimodaltraj_2_amd import train as tr
    from multimodaltraj_2_amd.argParser import ArgsParser
    from multimodaltraj_2_amd.fullcov import FullCovHead
    from multimodaltraj_2_amd.nll import GaussianHead
    argv = ["--data_root", data_root, "--leaveDataset", "2", "--n_max", "32", "--train_scenes", "64",
            "--train_batch", "32", "--num_epochs", "2", "--loss", "l2", "--num_samples", "20",
            "--mode", "train", "--save_dir", str(tmp_path), "--log_dir", str(tmp_path),
            "--device", "cuda:0", "--couple_scores", "1"]
    args = ArgsParser().parser.parse_args(argv)
    assert args.scene_ranks == 0 and args.scene_bins == 0
    tr.run_train_mode(args, gpu, log=lambda s: None)
    prm = checkpoint.load_params(checkpoint.read_state(str(tmp_path)), device=gpu)
    logs0 = []
    res0 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs0.append, keep={})
    assert list(res0) == ["scenes", "pairs", "K"] + list(evaluate.FIGURES) + list(evaluate.CPL_FIGURES)
    assert not any("scene ranks" in s for s in logs0)

    args.scene_ranks = 1
    logs1, keep1 = [], {}
    res1 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs1.append, keep=keep1)
    assert list(res1) == list(res0) + list(evaluate.SCN_FIGURES)
    assert {k: res1[k] for k in res0} == res0 and logs1[:len(logs0)] == logs0 and len(logs1) == len(logs0) + 1
    assert logs1[-1].startswith("scene ranks of the 20 joint draws on dataset 2:")
    t = keep1["plan"].to_device(gpu, F=1)
    one = torch.ones(keep1["plan"].S, dtype=torch.int32, device=gpu)
    gh = GaussianHead(device=gpu)
    gh.head = keep1["head"]
    kw = dict(seed=args.sample_seed, n_frames=one, ped_mask=t["ped_mask"])
    direct = gh.scene_ranks(keep1["pred"], t["targets"], t["n_active"], 20, **kw)
    want = evaluate.scene_figures(direct)
    for k in evaluate.SCN_FIGURES:
        print(f"evaluation {k}: {res1[k]:.8g}")
        assert res1[k] == want[k] or (np.isnan(res1[k]) and np.isnan(want[k])), k
    assert torch.equal(keep1["scene_ranks"].hist, direct.hist) and torch.equal(keep1["scene_ranks"].tot, direct.tot)
    assert _same(keep1["scene_ranks"].sums, direct.sums) and keep1["scene_ranks"].per_frame_d is not None
    assert direct.bins == 21 and 0 < direct.frames <= keep1["plan"].S
    je = gh.joint_eval(keep1["pred"], t["targets"], t["n_active"], 2, 0.1, **kw)
    assert direct.frames == int((je.per_frame_i[..., 1] > 0).sum())       # the scene-frames with a couple
    # --scene_bins
    args.scene_bins = 7
    res7 = evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
    seven = gh.scene_ranks(keep1["pred"], t["targets"], t["n_active"], 20, 7, **kw)
    assert res7["scn_dev_loc"] == seven.dev("loc") and res7["scn_es"] == res1["scn_es"]
    assert {k: res7[k] for k in res0} == res0
    # with the other three heads; the flag off first: the parent's keys
    args.scene_ranks, args.scene_bins = 0, 0
    args.fullcov_head, args.mixture_head, args.coupled_head = "train", "train", "train"
    logs_off = []
    res_off = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs_off.append)
    args.scene_ranks = 1
    logs2, keep2 = [], {}
    res2 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs2.append, keep=keep2)
    keys, i = list(res_off), 0
    expect = []
    for k in keys:
        expect.append(k)
        for prefix, names in (("", evaluate.SCN_FIGURES), ("fullcov_", evaluate.FULLCOV_SCN_FIGURES),
                              ("mix_", evaluate.MIX_SCN_FIGURES), ("coupled_", evaluate.COUPLED_SCN_FIGURES)):
            if k == prefix + evaluate.CPL_FIGURES[-1]:
                expect += list(names)
    assert list(res2) == expect and len(expect) == len(keys) + 4 * len(evaluate.SCN_FIGURES)
    assert {k: res2[k] for k in res_off} == res_off
    assert len(logs2) == len(logs_off) + 4 and [s for s in logs2 if "scene ranks" not in s] == logs_off
    for name in ("scene ranks", "full-covariance scene ranks", "mixture scene ranks", "coupled scene ranks"):
        assert sum(s.startswith(name + " of the 20 joint draws on dataset 2:") for s in logs2) == 1
    fc = FullCovHead(device=gpu)
    fc.chol = keep2["fullcov_chol"]
    wants = dict(evaluate.scene_figures(fc.scene_ranks(keep2["pred"], t["targets"], t["n_active"], 20, **kw), "fullcov_"))
    wants.update(evaluate.scene_figures(keep2["mixture"]["head"].scene_ranks(keep2["pred"], t["targets"],
                                                                            t["n_active"], 20, **kw), "mix_"))
    wants.update(evaluate.scene_figures(keep2["coupled"]["head"].scene_ranks(keep2["pred"], t["targets"],
                                                                            t["n_active"], 20, **kw), "coupled_"))
    for k, v in wants.items():
        print(f"evaluation {k}: {res2[k]:.8g}")
        assert res2[k] == v or (np.isnan(res2[k]) and np.isnan(v)), k
    assert keep2["coupled"]["scene_ranks"].frames == keep2["fullcov"]["scene_ranks"].frames == res2["scn_frames"]
    # the command line: evaluate.main on the same checkpoint prints the API's figures
    lines = []
    evaluate.main(["--data_root", data_root, "--leaveDataset", "2", "--n_max", "32", "--num_samples", "20",
                   "--save_dir", str(tmp_path), "--device", "cuda:0", "--scene_ranks", "1"], log=lines.append)
    line = [s for s in lines if isinstance(s, str) and s.startswith("scene ranks of the 20 joint draws")]
    assert line == [logs1[-1]]
    args.couple_scores = 0
    for k in (1, 65):
        args.num_samples = k
        with pytest.raises(ValueError, match="2 <= K <= 64"):
            evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
