"""GPU: the fused k-medoid reduction of joint samples to scene modes
(g2k_scene_modes_f32, g2k_fullcov_scene_modes_f32, g2k_mix_scene_modes_f32,
g2k_coupled_scene_modes_f32, csrc/g2k_scene_modes.hip; the four heads'
``scene_modes``; evaluate.py) against the checker tests/scene_modes_ref.py fed
with the DEVICE's own draws (the head's sampler called K times at seeds seed +
k), so that the comparison sees the kernel's arithmetic and not the draws'.
PARITY UNPINNED against the reference (it has no probabilistic head).  Both
sides are double on the same float32 values, so only the summation order
differs: the doubles are held to 1e-12 max(1, |ref|) — a double sum of at most
12 * 256 correctly rounded terms is off by 3072 * 1.1e-16 = 3.4e-13 at the worst
— and the integers (per_frame_i, medoids, counts, tot) must be EQUAL.  A
scene-frame in which the device's draws bring the two best candidates of an
argmin or argmax within 1e-9 relative without being bit-equal is left out of the
equality; above 1 % of the scene-frames the test fails as untestable.  The
cases (tests/scene_modes_cases.py) are the smallest that reach each path."""
import ctypes

import numpy as np
import pytest
import torch

from tests import couples_cases as cc
from tests import scene_modes_cases as mc
from tests import scene_modes_ref as mr
from tests import scene_ranks_cases as sc
from tests.abi_arena import Arena, all_written
from tests.bestk_ref import BOUNDARY_SEEDS, MASK64

pytestmark = pytest.mark.gpu
ALL = [(i, w) for i in range(len(mc.CASES)) for w in mc.HEADS]
ALL_IDS = [f"{mc.IDS[i]}-{w}" for i, w in ALL]
STEMS = {"per_step": "g2k_scene_modes", "fullcov": "g2k_fullcov_scene_modes", "mix": "g2k_mix_scene_modes",
         "coupled": "g2k_coupled_scene_modes"}
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


_DEV, _RES, _DRAWS, _REF, _WORST = {}, {}, {}, {}, {}


def _device_inputs(i, which, dev):
    """(head object, dict of device tensors) of case i's shape (shared by the
    cases of one shape)."""
    b = mc.base(i)
    if (b, which) not in _DEV:
        c = mc.inputs(i)
        t = {k: _t(c[k], dev) for k in ("pred", "targets", "n_active", "n_frames", "ped_mask")}
        _DEV[(b, which)] = (_head(which, c, dev), t)
    return _DEV[(b, which)]


def _key(i, which, seed):
    """The caches' key: the case's own seed (None), or another."""
    return (i, which) if seed is None else (i, which, seed)


def _run(i, which, dev, want_per_frame=True, want_modes=True, stream=None, seed=None):
    c = mc.inputs(i)
    h, t = _device_inputs(i, which, dev)
    r = h.scene_modes(t["pred"], t["targets"], t["n_active"], c["K"], c["M"], c["iters"], c["radius"],
                      seed=c["seed"] if seed is None else seed, n_frames=t["n_frames"], ped_mask=t["ped_mask"],
                      want_per_frame=want_per_frame, want_modes=want_modes, targets_shared=c["shared"],
                      stream=stream)
    torch.cuda.synchronize()
    return r


def _result(i, which, dev, seed=None):
    key = _key(i, which, seed)
    if key not in _RES:
        _RES[key] = _run(i, which, dev, seed=seed)
    return _RES[key]


def _draws(i, which, dev, seed=None):
    """The device's own K joint draws [K, S, F, 24, N] float32 (made once per shape)."""
    key = _key(mc.base(i), which, seed)
    if key not in _DRAWS:
        c = mc.inputs(i)
        h, t = _device_inputs(i, which, dev)
        s0 = c["seed"] if seed is None else seed
        _DRAWS[key] = np.stack([h.sample(t["pred"], seed=(s0 + k) & MASK64).cpu().numpy()
                                for k in range(c["K"])]).astype(np.float32)
    return _DRAWS[key]


def _recount(i, which, dev, seed=None):
    """The checker over the device's own K draws (computed once)."""
    key = _key(i, which, seed)
    if key not in _REF:
        c = mc.inputs(i)
        _REF[key] = mr.scene_modes_ref(_draws(i, which, dev, seed), c["targets"], c["members"], c["K"], c["M"],
                                       c["iters"], c["radius"])
    return _REF[key]


def _check_against(r, R, label, worst=_WORST):
    """The doubles within TOL of the checker's, the integers equal to it,
    outside the scene-frames the checker marks ambiguous; tot the rows' own
    recount."""
    pi = r.per_frame_i.cpu().numpy().astype(np.int64)
    pd, sums = r.per_frame_d.cpu().numpy(), r.sums.cpu().numpy()
    med, cnt = r.medoids.cpu().numpy().astype(np.int64), r.counts.cpu().numpy().astype(np.int64)
    tot = r.tot.cpu().numpy()
    keep = ~R["ambiguous"]
    err = np.abs(pd - R["per_frame_d"]) / np.maximum(1.0, np.abs(R["per_frame_d"]))
    serr = np.abs(sums - R["sums"]) / np.maximum(1.0, np.abs(R["sums"]))
    off = int((pi[keep] != R["per_frame_i"][keep]).sum() + (med[keep] != R["medoids"][keep]).sum()
              + (cnt[keep] != R["counts"][keep]).sum())
    worst_d = float(err[keep].max()) if err[keep].size else 0.0
    print(f"{label}: {R['frames']} scene-frames scored, {int(R['ambiguous'].sum())} left out as ambiguous; worst "
          f"error of per_frame_d {worst_d:.3g}, of sums {serr.max() if serr.size else 0.0:.3g} (tolerance {TOL:g}); "
          f"{off} integers off the checker's own")
    worst[label] = (worst_d, float(serr.max()) if serr.size else 0.0, R["frames"], int(R["ambiguous"].sum()))
    assert pd.dtype == np.float64 and np.isfinite(pd).all() and np.isfinite(sums).all()
    assert np.all(err[keep] <= TOL)
    np.testing.assert_array_equal(pi[keep], R["per_frame_i"][keep])
    np.testing.assert_array_equal(med[keep], R["medoids"][keep])
    np.testing.assert_array_equal(cnt[keep], R["counts"][keep])
    np.testing.assert_array_equal(pi[..., 0], R["per_frame_i"][..., 0])
    # the scene's rows, recounted from the device's own per-frame outputs: exact for the integers
    scored = pi[..., 0] > 0
    missed = scored & (pd[..., 7] > float(np.float32(r.miss_radius)))
    want = np.stack([scored.sum(axis=1), pi[..., 0].sum(axis=1), missed.sum(axis=1), pi[..., 3].sum(axis=1)], axis=1)
    np.testing.assert_array_equal(tot, want)
    if not R["ambiguous"].any():
        np.testing.assert_array_equal(tot, R["tot"])
        assert np.all(serr <= TOL)


def _parity(dev, i, which, seed=None, label="", worst=_WORST):
    c = mc.inputs(i)
    r, R = _result(i, which, dev, seed), _recount(i, which, dev, seed)
    _check_against(r, R, f"case {mc.IDS[i]} {which}{label}", worst)
    assert (r.k, r.modes, r.iters) == (c["K"], c["M"], c["iters"])
    assert r.frames == int((c["members"].sum(axis=2) >= 1).sum())
    # the result class's figures are the sums'
    want = mr.figures(r.sums.cpu().numpy(), r.tot.cpu().numpy())
    for k, v in want.items():
        assert getattr(r, k) == pytest.approx(v, rel=1e-12), k
    assert r.all_jade <= r.jade and r.all_jade <= r.raw_jade and 0.0 <= r.miss_rate <= 1.0
    if c["M"] == c["K"]:
        assert r.jade == r.all_jade and r.cost == 0.0


@pytest.mark.parametrize("i,which", ALL, ids=ALL_IDS)
def test_doubles_within_tolerance_and_integers_equal(gpu, i, which):
    _parity(gpu, i, which)


@pytest.mark.parametrize("which", mc.HEADS)
@pytest.mark.parametrize("at", BOUNDARY_SEEDS)
def test_seed_whose_low_word_carries(gpu, at, which):
    """Case k2 with the same assertions at the seeds where draw 1's seed carries
    out of the low word (A = 2^32 - 1) and wraps to 0 (W = 2^64 - 1): the kernel's
    own lo / hi arithmetic (csrc/g2k_scene_modes.hip) against the samplers' at
    (seed + k) mod 2^64; for the coupled head the salt is XORed in after the
    carry.  tests/test_scene_modes.py: the restated draws leave no scene-frame
    ambiguous there, and the checker's integer outputs change when the carry
    is dropped."""
    _parity(gpu, mc.IDS.index("k2"), which, BOUNDARY_SEEDS[at], f" seed {at}", worst={})


def test_scene_frames_left_out_as_ambiguous(gpu):
    """Over every case and head (computed above, or here): at most 1 % of the
    scene-frames may be left out of the equality; zero is expected.  Prints the
    worst deviation DESIGN records."""
    for i, which in ALL:
        _check_against(_result(i, which, gpu), _recount(i, which, gpu), f"case {mc.IDS[i]} {which}")
    frames = sum(v[2] for v in _WORST.values())
    out = sum(v[3] for v in _WORST.values())
    print(f"{frames} scene-frames on the device's draws, {out} left out as ambiguous; worst deviation of "
          f"per_frame_d {max(v[0] for v in _WORST.values()):.3g}, of sums {max(v[1] for v in _WORST.values()):.3g}")
    assert frames == 4 * 40 and out * 100 <= frames


def _raw_call(i, which, dev, pi, pd, med, cnt, sums, tot, t=None, ws=None, stream=None, sync=True):
    """The entry point itself, on caller-made buffers."""
    from multimodaltraj_2_amd import _lib, coupled, scenemodes
    from multimodaltraj_2_amd.frame_step import _ptr, _stream
    lib = coupled.load() if which == "coupled" else scenemodes.load()
    scenemodes.load()
    c = mc.inputs(i)
    h, t0 = _device_inputs(i, which, dev)
    t = t or dict(t0, params=_params(h, which))
    d = h._dims(t0["pred"])
    if c["shared"]:
        d.flags = _lib.STEP_TARGETS_SHARED
    need = int(lib.g2k_scene_modes_workspace_bytes(ctypes.byref(d), c["K"], c["M"]))
    if ws is None:
        ws = torch.empty(max(8, need), dtype=torch.uint8, device=dev)
    rc_ = getattr(lib, STEMS[which] + "_f32")(ctypes.byref(d), _ptr(t["pred"]), _ptr(t["targets"]),
                                              _ptr(t["n_active"]), _ptr(t["n_frames"]), _ptr(t["ped_mask"]),
                                              _ptr(t["params"]), ctypes.c_uint64(c["seed"]), c["K"], c["M"],
                                              c["iters"], ctypes.c_float(c["radius"]), _ptr(pi), _ptr(pd),
                                              _ptr(med), _ptr(cnt), _ptr(sums), _ptr(tot), _ptr(ws), need,
                                              _stream(stream))
    if sync:
        torch.cuda.synchronize()
    assert rc_ == 0, lib.g2k_last_error()
    return need


def _same(a, b):
    w = torch.int64 if a.element_size() == 8 else torch.int32
    return torch.equal(a.view(w), b.view(w))                          # the bits


def _outs(ar, S, F, M, tag="", offs=(0, 0, 0, 0, 0, 0)):
    return dict(pi=ar.alloc((S, F, 4), torch.int32, name="per_frame_i" + tag, offset=offs[0]),
                pd=ar.alloc((S, F, 8), torch.float64, name="per_frame_d" + tag, offset=offs[1]),
                med=ar.alloc((S, F, M), torch.int32, name="medoids" + tag, offset=offs[2]),
                cnt=ar.alloc((S, F, M), torch.int32, name="counts" + tag, offset=offs[3]),
                sums=ar.alloc((S, 8), torch.float64, name="sums" + tag, offset=offs[4]),
                tot=ar.alloc((S, 4), torch.int64, name="tot" + tag, offset=offs[5]))


def _equal(o, r):
    return (torch.equal(o["pi"], r.per_frame_i) and _same(o["pd"], r.per_frame_d)
            and torch.equal(o["med"], r.medoids) and torch.equal(o["cnt"], r.counts)
            and _same(o["sums"], r.sums) and torch.equal(o["tot"], r.tot))


FOOT = [mc.IDS.index(n) for n in ("k2", "k20", "k32")]
OPTIONAL = ("pi", "pd", "med", "cnt")


@pytest.mark.parametrize("which", mc.HEADS)
@pytest.mark.parametrize("i", FOOT, ids=[mc.IDS[i] for i in FOOT])
def test_determinism_and_footprint(gpu, i, which):
    """Guarded, poisoned outputs: every element written, nothing outside; the
    bits of a second call and of the Python path; each optional output NULL
    leaves the bits of the others alone; unscored scene-frames exactly zero; the
    NaN poison of the inputs never read."""
    c = mc.inputs(i)
    S, F, _, N = c["pred"].shape
    M = c["M"]
    ar = Arena(gpu)
    o = _outs(ar, S, F, M)
    _raw_call(i, which, gpu, **o)
    ar.check_guards()
    assert all(all_written(v) for v in o.values())
    r = _result(i, which, gpu)
    assert _equal(o, r)
    again = _run(i, which, gpu)
    assert _equal(dict(pi=again.per_frame_i, pd=again.per_frame_d, med=again.medoids, cnt=again.counts,
                       sums=again.sums, tot=again.tot), r)
    for drop in OPTIONAL + ("all",):
        o2 = _outs(ar, S, F, M, "_" + drop)
        args = {k: (None if (k == drop or (drop == "all" and k in OPTIONAL)) else v) for k, v in o2.items()}
        _raw_call(i, which, gpu, **args)
        ar.check_guards()
        for k, v in args.items():
            if v is None:
                continue
            assert all_written(v), (drop, k)
            assert _same(v, o[k]), (drop, k)
    no = _run(i, which, gpu, want_per_frame=False, want_modes=False)
    assert no.per_frame_i is None and no.per_frame_d is None and no.medoids is None and no.counts is None
    assert _same(no.sums, r.sums) and torch.equal(no.tot, r.tot)
    assert not bool(torch.isnan(o["pd"]).any()) and not bool(torch.isnan(o["sums"]).any())
    unscored = _t(c["members"].sum(axis=2) < 1, gpu)
    assert bool((o["pd"][unscored] == 0).all()) and bool((o["pi"][unscored] == 0).all())
    assert bool((o["med"][unscored] == 0).all()) and bool((o["cnt"][unscored] == 0).all())
    assert bool((o["pi"][~unscored][:, 0] >= 1).all()) and bool((o["cnt"][~unscored].sum(dim=1) == c["K"]).all())
    assert bool((o["sums"][:, 7] == 0).all())


def test_no_frames_writes_zeros(gpu):
    """F = 0 with S > 0: sums and tot are written, all zero."""
    from multimodaltraj_2_amd import _lib, coupled, scenemodes
    from multimodaltraj_2_amd.frame_step import _ptr
    lib = coupled.load()
    scenemodes.load()
    d = _lib.G2KDims(3, 0, 8, 12, 16, 64, 16, 8, 0)
    some = torch.zeros(64, device=gpu)                      # pred, targets, head: named, never read
    n_active = torch.full((3,), 16, dtype=torch.int32, device=gpu)
    ar = Arena(gpu)
    sums, tot = ar.alloc((3, 8), torch.float64, name="sums"), ar.alloc((3, 4), torch.int64, name="tot")
    need = int(lib.g2k_scene_modes_workspace_bytes(ctypes.byref(d), 20, 6))
    assert need == 3 * 136
    ws = ar.alloc((need,), torch.uint8, name="workspace")
    for stem in STEMS.values():
        rc_ = getattr(lib, stem + "_f32")(ctypes.byref(d), _ptr(some), _ptr(some), _ptr(n_active), None, None,
                                          _ptr(some), ctypes.c_uint64(1), 20, 6, 10, ctypes.c_float(1.0), None,
                                          None, None, None, _ptr(sums), _ptr(tot), _ptr(ws), need, None)
        torch.cuda.synchronize()
        assert rc_ == 0, lib.g2k_last_error()
        ar.check_guards()
        assert all_written(sums) and all_written(tot)
        assert not bool(sums.any()) and not bool(tot.any())
        sums.fill_(5)
        tot.fill_(5)


@pytest.mark.parametrize("which", mc.HEADS)
def test_at_minimum_alignment(gpu, which):
    """Each entry point at the weakest pointer alignment its header line
    states (targets 8, per_frame_i 4, per_frame_d 8, medoids 4, counts 4, sums
    8, tot 8, workspace 8) and every other pointer at its element's own (4;
    the mask 1): the bits of the aligned call."""
    i = mc.IDS.index("shared")
    c = mc.inputs(i)
    S, F, _, N = c["pred"].shape
    h, _ = _device_inputs(i, which, gpu)
    ar = Arena(gpu)
    t = dict(pred=ar.put(c["pred"], "pred", 4), targets=ar.put(c["targets"], "targets", 8),
             n_active=ar.put(c["n_active"], "n_active", 4), n_frames=ar.put(c["n_frames"], "n_frames", 4),
             ped_mask=ar.put(c["ped_mask"], "ped_mask", 1),
             params=ar.put(_params(h, which).cpu().numpy(), "params", 4))
    assert t["targets"].data_ptr() % 16 == 8 and t["pred"].data_ptr() % 16 == 4
    o = _outs(ar, S, F, c["M"], offs=(4, 8, 4, 4, 8, 8))
    row = 88 + 8 * c["M"]
    ws = ar.alloc((S * F * row,), torch.uint8, name="workspace", offset=8)
    for k in ("pi", "med", "cnt"):
        assert o[k].data_ptr() % 8 == 4
    for v in (o["pd"], o["sums"], o["tot"], ws):
        assert v.data_ptr() % 16 == 8
    assert _raw_call(i, which, gpu, t=t, ws=ws, **o) == S * F * row
    ar.check_guards()
    assert _equal(o, _result(i, which, gpu))


@pytest.mark.parametrize("which", mc.HEADS)
def test_under_graph_capture(gpu, which):
    """The call is capturable and allocates nothing: captured on a side
    stream and replayed twice, the bits of the plain call."""
    i = mc.IDS.index("k20")
    c = mc.inputs(i)
    S, F, _, N = c["pred"].shape
    M = c["M"]
    r = _result(i, which, gpu)
    o = dict(pi=torch.zeros((S, F, 4), dtype=torch.int32, device=gpu),
             pd=torch.zeros((S, F, 8), dtype=torch.float64, device=gpu),
             med=torch.zeros((S, F, M), dtype=torch.int32, device=gpu),
             cnt=torch.zeros((S, F, M), dtype=torch.int32, device=gpu),
             sums=torch.zeros((S, 8), dtype=torch.float64, device=gpu),
             tot=torch.zeros((S, 4), dtype=torch.int64, device=gpu))
    ws = torch.empty(S * F * (88 + 8 * M), dtype=torch.uint8, device=gpu)
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
        assert _equal(o, r)


def test_coupled_without_a_shared_part_is_the_full_covariance_head(gpu):
    """Lb = 0: every output bit of g2k_coupled_scene_modes_f32 is
    g2k_fullcov_scene_modes_f32's with chol = Lw."""
    from multimodaltraj_2_amd.coupled import CoupledHead
    from multimodaltraj_2_amd.fullcov import FullCovHead
    for name in ("k20", "k64"):
        i = mc.IDS.index(name)
        c = mc.inputs(i)
        _, t = _device_inputs(i, "coupled", gpu)
        co, fc = CoupledHead(device=gpu), FullCovHead(device=gpu)
        co.cpl = _t(np.stack([c["cpl"][0], np.zeros((24, 24), np.float32)]), gpu)
        fc.chol = _t(c["cpl"][0], gpu)
        kw = dict(seed=c["seed"], n_frames=t["n_frames"], ped_mask=t["ped_mask"], want_per_frame=True)
        a = co.scene_modes(t["pred"], t["targets"], t["n_active"], c["K"], c["M"], c["iters"], c["radius"], **kw)
        b = fc.scene_modes(t["pred"], t["targets"], t["n_active"], c["K"], c["M"], c["iters"], c["radius"], **kw)
        assert _equal(dict(pi=a.per_frame_i, pd=a.per_frame_d, med=a.medoids, cnt=a.counts, sums=a.sums,
                           tot=a.tot), b)
        assert a.frames > 0
        # and with its shared part it is another law
        assert not _same(_result(i, "coupled", gpu).per_frame_d, b.per_frame_d)


@pytest.mark.parametrize("which", mc.HEADS)
def test_the_floor_is_joint_evals_best_of_k(gpu, which):
    """P all is joint_eval's P minJADE_K at the same K and seed, and where
    every draw is a medoid (M = K) P cF is its P minJFDE_K, within that
    kernel's fp32 accumulation bound, (12 P + 4) 2^-24 relative."""
    for name in ("k2", "k20", "n256", "k32", "shared"):
        i = mc.IDS.index(name)
        c = mc.inputs(i)
        h, t = _device_inputs(i, which, gpu)
        r = _result(i, which, gpu)
        je = h.joint_eval(t["pred"], t["targets"], t["n_active"], c["K"], 0.1, seed=c["seed"],
                          n_frames=t["n_frames"], ped_mask=t["ped_mask"], targets_shared=c["shared"],
                          want_per_frame=True)
        Pn = r.per_frame_i[..., 0].double()
        assert torch.equal(je.per_frame_i[..., 0], r.per_frame_i[..., 0]) and je.pairs == r.totals()[1]
        bound = (12.0 * Pn + 4.0) * 2.0 ** -24
        jf = je.per_frame_f.double()
        mine, theirs = Pn * r.per_frame_d[..., 6], Pn * jf[..., 0]
        rel = ((mine - theirs).abs() / mine.clamp_min(1e-300))[Pn > 0]
        print(f"case {name} {which}: P all against joint_eval's P minJADE_K, worst {float(rel.max()):.3g} "
              f"(bound {float(bound.max()):.3g})")
        assert bool(((mine - theirs).abs() <= bound * mine).all())
        if c["M"] == c["K"]:
            mine, theirs = Pn * r.per_frame_d[..., 1], Pn * jf[..., 1]
            assert bool(((mine - theirs).abs() <= bound * mine).all())


@pytest.mark.parametrize("which", mc.HEADS)
def test_trajectories_are_the_medoid_draws(gpu, which):
    """SceneModes.trajectories regenerates the modes: the JADE of the gathered
    medoids against the targets in torch float64 is cA, within 1e-12."""
    for name in ("k20", "shared", "k2"):
        i = mc.IDS.index(name)
        c = mc.inputs(i)
        h, t = _device_inputs(i, which, gpu)
        r = _result(i, which, gpu)
        tr = r.trajectories(h, t["pred"])
        S, F, _, N = c["pred"].shape
        assert tuple(tr.shape) == (S, F, c["M"], 24, N) and tr.dtype == torch.float32
        xy = torch.stack([tr[:, :, :, :L], tr[:, :, :, L:]], dim=-1).double()        # [S, F, M, L, N, 2]
        tg = t["targets"].double().expand(S, F, N, L, 2).permute(0, 1, 3, 2, 4)      # [S, F, L, N, 2]
        e = (xy - tg[:, :, None]).pow(2).sum(dim=-1).sqrt()                          # [S, F, M, L, N]
        mem = _t(c["members"], gpu)[:, :, None, None, :]
        e = torch.where(mem, e, torch.zeros_like(e))
        Pn = r.per_frame_i[..., 0].double()
        jade = e.sum(dim=(3, 4)) / (12.0 * Pn.clamp_min(1.0))[..., None]             # [S, F, M]
        cA, mA = jade.min(dim=2)
        scored = Pn > 0
        err = ((cA - r.per_frame_d[..., 0]).abs() / r.per_frame_d[..., 0].abs().clamp_min(1.0))[scored]
        print(f"case {name} {which}: JADE of the regenerated medoids against cA, worst {float(err.max()):.3g}")
        assert bool((err <= TOL).all())
        assert torch.equal(mA[scored].int(), r.per_frame_i[..., 1][scored])
        # each mode is the draw its index names
        m0 = int(r.medoids[0, 0, 0])
        again = h.sample(t["pred"], seed=(c["seed"] + m0) & MASK64)
        assert _same(tr[0, 0, 0].contiguous(), again[0, 0].contiguous())         # the bits: poison included


def test_the_coupled_heads_modes_cover_the_scene_on_the_device(gpu):
    """tests/test_scene_modes.py's property with the device's fits, samplers
    and the fused call: CoupledHead.fit and FullCovHead.fit on the first target
    set, scene_modes on the second.  It cannot pass without the feature."""
    from multimodaltraj_2_amd.coupled import CoupledHead
    from multimodaltraj_2_amd.fullcov import FullCovHead
    S, F, N, K, M, iters, seed = (mc.PROP[k] for k in ("S", "F", "N", "K", "M", "iters", "seed"))
    pred_h = cc.property_setup(S, F, N, mc.PROP["side"])
    pred = _t(pred_h, gpu)
    n_active = _t(sc.property_n_active(), gpu)
    fit_tg, score_tg = (_t(cc.coupled_targets(pred_h, mc.PROP["sigma"], mc.PROP["share"],
                                              rng_seed=mc.PROP[w + "_seed"]), gpu) for w in ("fit", "score"))
    co, fc = CoupledHead(device=gpu), FullCovHead(device=gpu)
    st = co.fit(pred, fit_tg, n_active)
    fc.fit(pred, fit_tg, n_active)
    print(f"device: fitted share {st.share:.4f}, clipped {co.clipped}")
    assert abs(st.share - mc.PROP["share"]) < 0.03

    def score(kind):
        h = co if kind == "coupled" else fc
        r = h.scene_modes(pred, score_tg, n_active, K, M, iters, mc.PROPERTY["radius"], seed=seed)
        assert r.frames == S * F
        return {k: getattr(r, k) for k in ("frames", "jade", "jfde", "brier_jade", "brier_jfde", "miss_rate",
                                           "cost", "raw_jade", "all_jade", "rounds")}
    mc.property_check(score, "device: ")


def test_evaluation_end_to_end(gpu, tmp_path, data_root):
    """The recipe of tests/test_scene_ranks_gpu.py::test_evaluation_end_to_end
    with --num_samples 20 --couple_scores 1 --scene_ranks 1 --scene_modes 6,
    without and with the other three heads: the new keys directly after each
    head's scene-rank figures, equal to a direct call on ``keep``'s tensors;
    the old keys and values unchanged, one more log line per head; the command
    line gives what the API gives."""
    from multimodaltraj_2_amd import checkpoint, evaluate
    from multimodaltraj_2_amd import train as tr
    from multimodaltraj_2_amd.argParser import ArgsParser
    from multimodaltraj_2_amd.fullcov import FullCovHead
    from multimodaltraj_2_amd.nll import GaussianHead
    argv = ["--data_root", data_root, "--leaveDataset", "2", "--n_max", "32", "--train_scenes", "64",
            "--train_batch", "32", "--num_epochs", "2", "--loss", "l2", "--num_samples", "20",
            "--mode", "train", "--save_dir", str(tmp_path), "--log_dir", str(tmp_path),
            "--device", "cuda:0", "--couple_scores", "1", "--scene_ranks", "1", "--miss_radius", "0.5"]
    args = ArgsParser().parser.parse_args(argv)
    assert args.scene_modes == 0 and args.scene_modes_iters == 10
    tr.run_train_mode(args, gpu, log=lambda s: None)
    prm = checkpoint.load_params(checkpoint.read_state(str(tmp_path)), device=gpu)
    logs0 = []
    res0 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs0.append, keep={})
    assert list(res0) == (["scenes", "pairs", "K"] + list(evaluate.FIGURES) + list(evaluate.CPL_FIGURES)
                          + list(evaluate.SCN_FIGURES))
    assert not any("scene modes" in s for s in logs0)

    args.scene_modes = 6
    logs1, keep1 = [], {}
    res1 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs1.append, keep=keep1)
    assert list(res1) == list(res0) + list(evaluate.SMD_FIGURES)
    assert {k: res1[k] for k in res0} == res0 and logs1[:len(logs0)] == logs0 and len(logs1) == len(logs0) + 1
    assert logs1[-1].startswith("scene modes of the 20 joint draws on dataset 2:")
    t = keep1["plan"].to_device(gpu, F=1)
    one = torch.ones(keep1["plan"].S, dtype=torch.int32, device=gpu)
    gh = GaussianHead(device=gpu)
    gh.head = keep1["head"]
    kw = dict(seed=args.sample_seed, n_frames=one, ped_mask=t["ped_mask"])
    direct = gh.scene_modes(keep1["pred"], t["targets"], t["n_active"], 20, 6, 10, 0.5, **kw)
    want = evaluate.scene_mode_figures(direct)
    for k in evaluate.SMD_FIGURES:
        print(f"evaluation {k}: {res1[k]:.8g}")
        assert res1[k] == want[k] or (np.isnan(res1[k]) and np.isnan(want[k])), k
    kept = keep1["scene_modes"]
    assert torch.equal(kept.tot, direct.tot) and _same(kept.sums, direct.sums) and kept.per_frame_d is not None
    assert torch.equal(kept.medoids, direct.medoids) and torch.equal(kept.counts, direct.counts)
    je = gh.joint_eval(keep1["pred"], t["targets"], t["n_active"], 20, 0.1, **kw)
    assert direct.frames == int((je.per_frame_i[..., 0] > 0).sum()) and direct.totals()[1] == je.pairs
    assert res1["smd_all_jade"] <= res1["smd_jade"] and res1["smd_all_jade"] == pytest.approx(je.jade, rel=1e-4)
    # --scene_modes_iters
    args.scene_modes_iters = 0
    res_b = evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
    assert res_b["smd_rounds"] == 0.0 and res_b["smd_all_jade"] == res1["smd_all_jade"]
    assert {k: res_b[k] for k in res0} == res0
    # with the other three heads; the flag off first: the parent's keys
    args.scene_modes, args.scene_modes_iters = 0, 10
    args.fullcov_head, args.mixture_head, args.coupled_head = "train", "train", "train"
    logs_off = []
    res_off = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs_off.append)
    args.scene_modes = 6
    logs2, keep2 = [], {}
    res2 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs2.append, keep=keep2)
    expect = []
    for k in res_off:
        expect.append(k)
        for prefix, names in (("", evaluate.SMD_FIGURES), ("fullcov_", evaluate.FULLCOV_SMD_FIGURES),
                              ("mix_", evaluate.MIX_SMD_FIGURES), ("coupled_", evaluate.COUPLED_SMD_FIGURES)):
            if k == prefix + evaluate.SCN_FIGURES[-1]:
                expect += list(names)
    assert list(res2) == expect and len(expect) == len(res_off) + 4 * len(evaluate.SMD_FIGURES)
    assert {k: res2[k] for k in res_off} == res_off
    assert len(logs2) == len(logs_off) + 4 and [s for s in logs2 if "scene modes" not in s] == logs_off
    for name in ("scene modes", "full-covariance scene modes", "mixture scene modes", "coupled scene modes"):
        assert sum(s.startswith(name + " of the 20 joint draws on dataset 2:") for s in logs2) == 1
    fc = FullCovHead(device=gpu)
    fc.chol = keep2["fullcov_chol"]
    call = lambda h: h.scene_modes(keep2["pred"], t["targets"], t["n_active"], 20, 6, 10, 0.5, **kw)
    wants = dict(evaluate.scene_mode_figures(call(fc), "fullcov_"))
    wants.update(evaluate.scene_mode_figures(call(keep2["mixture"]["head"]), "mix_"))
    wants.update(evaluate.scene_mode_figures(call(keep2["coupled"]["head"]), "coupled_"))
    for k, v in wants.items():
        print(f"evaluation {k}: {res2[k]:.8g}")
        assert res2[k] == v or (np.isnan(res2[k]) and np.isnan(v)), k
    assert keep2["coupled"]["scene_modes"].frames == keep2["fullcov"]["scene_modes"].frames == res2["smd_frames"]
    assert keep2["mixture"]["scene_modes"].frames == res2["smd_frames"]
    # the command line: evaluate.main on the same checkpoint prints the API's figures
    lines = []
    evaluate.main(["--data_root", data_root, "--leaveDataset", "2", "--n_max", "32", "--num_samples", "20",
                   "--save_dir", str(tmp_path), "--device", "cuda:0", "--scene_modes", "6", "--miss_radius", "0.5"],
                  log=lines.append)
    line = [s for s in lines if isinstance(s, str) and s.startswith("scene modes of the 20 joint draws")]
    assert line == [logs1[-1]]
    for k in (5, 65):
        args.num_samples = k
        with pytest.raises(ValueError, match="K <= 64"):
            evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
