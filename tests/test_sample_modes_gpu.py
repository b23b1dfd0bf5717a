"""GPU: the fused k-means reduction of the heads' samples
(g2k_sample_modes_f32, g2k_fullcov_sample_modes_f32, g2k_mix_sample_modes_f32,
csrc/g2k_modes.hip; the three heads' ``sample_modes``; evaluate.py) against the
float64 checker tests/modes_ref.py fed with the DEVICE's own draws (the head's
sampler called K times at seeds seed + k), so that the comparison sees the
kernel's arithmetic and not the draws'.  PARITY UNPINNED against the reference
(it has no probabilistic head).

A pair whose checker margin is below 1e-9 is fragile and left out of the value
comparison (not of the structural checks); at most 1 % of a case's pairs may be
fragile, asserted here on the device's draws before anything is compared.  The
``collapsed`` case has exact ties by construction and is compared in full: ties
go to the lowest index on both sides.

Tolerances: the project's metric tolerance for cA, cF and the
inertia, |got - ref| <= 1e-4 max(1, |ref|) per pair and that times the pair
count for a scene's sums; the indices and the live count exact; the two weights
within 1e-6; the centres within 1e-5 max(1, |ref|); the weights exact to f32
rounding.  The cases (tests/modes_cases.py) are the smallest that reach each
path."""
import ctypes

import numpy as np
import pytest
import torch

from tests import bestk_ref
from tests import modes_cases as mc
from tests import modes_ref as mo
from tests.abi_arena import Arena, all_written
from tests.bestk_ref import MASK64, SEED_A

pytestmark = pytest.mark.gpu
STEMS = {"per_step": "g2k_sample_modes", "fullcov": "g2k_fullcov_sample_modes",
         "mix": "g2k_mix_sample_modes"}


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
        c = mc.inputs(i)
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


def _key(i, which, seed):
    """The caches' key: the case's own seed (None), or another."""
    return (i, which) if seed is None else (i, which, seed)


def _run(i, which, dev, want_per_ped=True, want_centres=True, head=None, seed=None):
    c = mc.inputs(i)
    h, t = _device_inputs(i, which, dev)
    r = (head or h).sample_modes(t["pred"], t["targets"], t["n_active"], c["K"], c["M"], c["iters"],
                                 seed=c["seed"] if seed is None else seed, miss_radius=mc.MISS_RADIUS,
                                 n_frames=t["n_frames"], ped_mask=t["ped_mask"], want_per_ped=want_per_ped,
                                 want_centres=want_centres, targets_shared=c["shared"])
    torch.cuda.synchronize()
    return r


_RES, _REF = {}, {}


def _result(i, which, dev, seed=None):
    key = _key(i, which, seed)
    if key not in _RES:
        _RES[key] = _run(i, which, dev, seed=seed)
    return _RES[key]


def _recount(i, which, dev, seed=None):
    """The float64 checker over the device's own K draws (computed once)."""
    key = _key(i, which, seed)
    if key not in _REF:
        c = mc.inputs(i)
        h, t = _device_inputs(i, which, dev)
        s0 = c["seed"] if seed is None else seed
        draws = np.stack([h.sample(t["pred"], seed=(s0 + k) & MASK64).cpu().numpy()
                          for k in range(c["K"])])
        _REF[key] = mo.sample_modes_ref(draws, c["targets"], c["pairs"], c["M"], c["iters"], mc.MISS_RADIUS)
    return _REF[key]


def _gate(ref, tol=mo.TOL):
    return tol * np.maximum(1.0, np.abs(ref))


def _parity(dev, i, which, seed=None, label=""):
    c = mc.inputs(i)
    r, R = _result(i, which, dev, seed), _recount(i, which, dev, seed)
    m = c["pairs"]
    n = int(m.sum())
    # the cap on fragile pairs: a condition on the inputs, on the device's draws
    frag = m & (R["margin"] < mo.FRAGILE)
    if mc.IDS[i] == "collapsed":
        assert frag[m].all()                 # exact ties by construction: compared in full
        ok = m
    else:
        assert int(frag.sum()) <= mo.FRAGILE_SHARE * n, (int(frag.sum()), n)
        ok = m & ~frag
    per, out = r.per_ped.cpu().numpy().astype(np.float64), r.out.cpu().numpy().astype(np.float64)
    cen, wts = r.centres.cpu().numpy().astype(np.float64), r.weights.cpu().numpy()
    assert np.isfinite(per).all() and np.isfinite(out).all() and np.isfinite(cen).all()
    P, Rp = per[ok], R["per_ped"][ok]
    e_val = (np.abs(P[:, [0, 1, 6]] - Rp[:, [0, 1, 6]]) / _gate(Rp[:, [0, 1, 6]])).max(initial=0.0)
    e_w = np.abs(P[:, 4:6] - Rp[:, 4:6]).max(initial=0.0)
    cg, cr = np.moveaxis(cen, 4, 2)[ok], np.moveaxis(R["centres"], 4, 2)[ok]     # [P, M, 24]
    e_cen = (np.abs(cg - cr) / _gate(cr, 1e-5)).max(initial=0.0)
    print(f"case {mc.IDS[i]} {which}{label}: {n} pairs, {int(frag.sum())} fragile (smallest margin "
          f"{R['margin'][m].min() if n else float('inf'):.3g}); worst |kernel - float64| / gate: cA, cF, "
          f"inertia {e_val:.3g}, centres {e_cen:.3g}; weights of the best centres off by {e_w:.3g}")
    assert e_val <= 1.0
    np.testing.assert_array_equal(P[:, [2, 3, 7]], Rp[:, [2, 3, 7]])          # mA, mF, live: exact
    assert e_w <= 1e-6
    assert e_cen <= 1.0
    np.testing.assert_array_equal(np.moveaxis(wts, 2, 3)[ok],                  # exact to f32 rounding
                                  np.moveaxis(R["weights"], 2, 3)[ok].astype(np.float32))
    # the scene sums: against the checker's where no pair of the scene is fragile ...
    npairs = R["out"][:, 7]
    clean = ~(frag & (mc.IDS[i] != "collapsed")).any(axis=(1, 2))
    e_out = np.abs(out[:, :7] - R["out"][:, :7]) / (_gate(R["out"][:, :7]) * np.maximum(npairs, 1)[:, None])
    assert e_out[clean].max(initial=0.0) <= 1.0
    # ... and always against the float64 sums of the kernel's own per_ped
    rad = float(np.float32(mc.MISS_RADIUS))
    own = np.stack([per[..., 0], per[..., 1], (1 - per[..., 4]) ** 2 * m, (1 - per[..., 5]) ** 2 * m,
                    (per[..., 1] > rad) * m, per[..., 6], per[..., 7]], axis=-1).sum(axis=(1, 2))
    e_own = np.abs(out[:, :7] - own) / (_gate(own) * np.maximum(npairs, 1)[:, None])
    print(f"   scene sums: against the checker {e_out[clean].max(initial=0.0):.3g}, against the "
          f"kernel's own per_ped {e_own.max(initial=0.0):.3g} (of the gate)")
    assert e_own.max(initial=0.0) <= 1.0
    np.testing.assert_array_equal(out[:, 7], npairs)                           # pair counts: exact
    assert np.all(per[~m] == 0)                                                # non-pairs: exactly zero
    assert np.all(np.moveaxis(cen, 4, 2)[~m] == 0) and np.all(np.moveaxis(wts, 2, 3)[~m] == 0)
    # structure, fragile pairs included: a pair's weights add to 1, live counts them, the indices
    # are centres, the weights are the named centres'
    np.testing.assert_allclose(wts.astype(np.float64).sum(axis=2)[m], 1.0, atol=1e-6)
    np.testing.assert_array_equal((wts > 0).sum(axis=2)[m], per[..., 7][m])
    assert np.all((per[..., 2:4][m] >= 0) & (per[..., 2:4][m] < c["M"]))
    wm = np.moveaxis(wts, 2, 3)[m]                                             # [P, M]
    for col in (0, 1):
        idx = per[..., 2 + col][m].astype(int)
        np.testing.assert_array_equal(per[..., 4 + col][m].astype(np.float32), wm[np.arange(n), idx])
    # the result class's figures are the sums'
    if n:
        want = mo.figures(out)
        for k, v in want.items():
            assert abs(getattr(r, k) - v) <= 1e-12 * max(1.0, abs(v)), k
        assert r.pairs == n and (r.k, r.modes, r.iters) == (c["K"], c["M"], c["iters"])
        assert r.miss_radius == mc.MISS_RADIUS
    else:
        assert np.isnan(r.min_ade) and np.isnan(r.miss_rate) and r.pairs == 0


@pytest.mark.parametrize("i,which", mc.ALL, ids=mc.ALL_IDS)
def test_recount_from_the_devices_own_draws(gpu, i, which):
    _parity(gpu, i, which)


@pytest.mark.parametrize("which", mc.HEADS)
def test_seed_whose_low_word_carries(gpu, which):
    """Case mk (tests/modes_cases.BOUNDARY_ROW) with the same assertions at seed
    A = 2^32 - 1, where draw 1's seed carries out of the low word: the
    launcher's split of the seed and drawn_lane's lo / hi arithmetic
    (csrc/g2k_drawn.h) against the samplers' at (seed + k) mod 2^64.
    tests/test_sample_modes.py: the checker's integer outputs change when the
    carry is dropped."""
    _parity(gpu, mc.IDS.index(mc.BOUNDARY_ROW), which, SEED_A, " seed A")


@pytest.mark.parametrize("which", mc.HEADS)
def test_closed_forms_on_the_device(gpu, which):
    """mk: the centres are the draws themselves, bit for bit what the sampler
    writes; m1: w = 1 and no Brier term."""
    i = mc.IDS.index("mk")
    c = mc.inputs(i)
    h, t = _device_inputs(i, which, gpu)
    r = _result(i, which, gpu)
    m = _t(c["pairs"], gpu)
    for k in range(c["K"]):
        d = h.sample(t["pred"], seed=(c["seed"] + k) & MASK64)
        assert torch.equal(r.centres[:, :, k].movedim(2, 3)[m], d.movedim(2, 3)[m])
    assert bool((r.weights.movedim(2, 3)[m] == 0.125).all()) and bool((r.per_ped[..., 6] == 0).all())
    r1 = _result(mc.IDS.index("m1"), which, gpu)
    m1 = _t(mc.inputs(mc.IDS.index("m1"))["pairs"], gpu)
    assert bool((r1.per_ped[..., 4:6][m1] == 1).all()) and bool((r1.out[:, 2:4] == 0).all())


@pytest.mark.parametrize("which", mc.HEADS)
def test_no_iteration_is_best_of_k_of_the_first_m_draws(gpu, which):
    """iters = 0: the centres are the first M draws, so cA / cF and their
    indices are the existing best_of_k's at K = M (an f32 kernel: the indices
    are compared where the checker's margin is above 1e-5, ten times what 12
    f32 distances and their sum can move an ADE by)."""
    i = mc.IDS.index("it0")
    c = mc.inputs(i)
    h, t = _device_inputs(i, which, gpu)
    r, R = _result(i, which, gpu), _recount(i, which, gpu)
    bk = h.best_of_k(t["pred"], t["targets"], t["n_active"], c["M"], seed=c["seed"],
                     n_frames=t["n_frames"], ped_mask=t["ped_mask"], want_per_ped=True)
    m = c["pairs"]
    per, best = r.per_ped.cpu().numpy().astype(np.float64), bk.per_ped.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(per[..., :2] - best[..., :2])[m] <= _gate(best[..., :2])[m])
    sure = m & (R["margin"] >= 1e-5)
    assert sure.sum() >= 0.9 * m.sum()
    np.testing.assert_array_equal(per[..., 2:4][sure], best[..., 2:4][sure])
    assert torch.equal(bk.sums[:, 2], r.out[:, 7])


def _raw_call(i, which, dev, per_ped, centres, weights, out, t=None, ws=None):
    """The entry point itself, on caller-made buffers."""
    from multimodaltraj_2_amd import _lib, modes
    from multimodaltraj_2_amd.frame_step import _ptr
    lib = modes.load()
    c = mc.inputs(i)
    h, t0 = _device_inputs(i, which, dev)
    t = t or dict(t0, params=_params(h, which))
    d = h._dims(t0["pred"])
    if c["shared"]:
        d.flags = _lib.STEP_TARGETS_SHARED
    need = int(lib.g2k_sample_modes_workspace_bytes(ctypes.byref(d)))
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = getattr(lib, STEMS[which] + "_f32")(ctypes.byref(d), _ptr(t["pred"]), _ptr(t["targets"]),
                                             _ptr(t["n_active"]), _ptr(t["n_frames"]),
                                             _ptr(t["ped_mask"]), _ptr(t["params"]),
                                             ctypes.c_uint64(c["seed"]), c["K"], c["M"], c["iters"],
                                             mc.MISS_RADIUS, _ptr(per_ped), _ptr(centres), _ptr(weights),
                                             _ptr(out), _ptr(ws), need, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.g2k_last_error()
    return need


FOOT = [mc.IDS.index(n) for n in ("eval", "passes", "tail", "m32")]


@pytest.mark.parametrize("which", mc.HEADS)
@pytest.mark.parametrize("i", FOOT, ids=[mc.IDS[i] for i in FOOT])
def test_determinism_and_footprint(gpu, i, which):
    """Guarded, poisoned outputs: every element written, nothing outside; the
    bits of a second call and of the Python path; every optional output NULL
    (and each alone) leaves out's bits alone; non-pairs exactly zero."""
    c = mc.inputs(i)
    S, F, _, N = c["pred"].shape
    M = c["M"]
    ar = Arena(gpu)
    per, out = ar.alloc((S, F, N, 8), name="per_ped"), ar.alloc((S, 8), name="out")
    cen, wts = ar.alloc((S, F, M, 24, N), name="centres"), ar.alloc((S, F, M, N), name="weights")
    out2, out3 = ar.alloc((S, 8), name="out2"), ar.alloc((S, 8), name="out3")
    cen3 = ar.alloc((S, F, M, 24, N), name="centres3")
    _raw_call(i, which, gpu, per, cen, wts, out)
    ar.check_guards()
    assert all_written(per) and all_written(out) and all_written(cen) and all_written(wts)
    r = _result(i, which, gpu)
    assert torch.equal(per, r.per_ped) and torch.equal(out, r.out)
    assert torch.equal(cen, r.centres) and torch.equal(wts, r.weights)
    again = _run(i, which, gpu)
    assert torch.equal(again.per_ped, r.per_ped) and torch.equal(again.out, r.out)
    assert torch.equal(again.centres, r.centres) and torch.equal(again.weights, r.weights)
    _raw_call(i, which, gpu, None, None, None, out2)
    ar.check_guards()
    assert all_written(out2) and torch.equal(out2, out)
    _raw_call(i, which, gpu, None, cen3, None, out3)
    ar.check_guards()
    assert all_written(out3) and torch.equal(out3, out) and torch.equal(cen3, cen)
    bare = _run(i, which, gpu, want_per_ped=False, want_centres=False)
    assert bare.per_ped is None and bare.centres is None and bare.weights is None
    assert torch.equal(bare.out, r.out)
    pairs = _t(c["pairs"], gpu)
    assert bool((per[~pairs] == 0).all()) and bool((cen.movedim(4, 2)[~pairs] == 0).all())
    assert bool((wts.movedim(2, 3)[~pairs] == 0).all())
    assert not bool(torch.isnan(per).any()) and not bool(torch.isnan(cen).any())   # the poison was never read


@pytest.mark.parametrize("which", mc.HEADS)
def test_centres_feed_the_other_entry_points(gpu, which):
    """A [:, :, m] slice of ``centres`` is laid out as pred: the ADE / FDE of
    the M slices against the targets have cA / cF as their per-pair minimum,
    and a slice passed as ``pred`` to best_of_k gives that slice's ADE
    (BestOfK.ade: the error of ``pred`` itself)."""
    i = mc.IDS.index("eval")
    c = mc.inputs(i)
    h, t = _device_inputs(i, which, gpu)
    r = _result(i, which, gpu)
    m = c["pairs"]
    a = np.full((c["M"],) + m.shape, np.inf)
    f = np.full((c["M"],) + m.shape, np.inf)
    for k in range(c["M"]):
        sl = r.centres[:, :, k].contiguous()
        assert sl.shape == t["pred"].shape
        ade, fde = bestk_ref.draw_errors(sl.cpu().numpy().astype(np.float64), c["targets"])
        a[k], f[k] = ade, fde
    per = r.per_ped.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(a.min(axis=0) - per[..., 0])[m] <= _gate(per[..., 0])[m])
    assert np.all(np.abs(f.min(axis=0) - per[..., 1])[m] <= _gate(per[..., 1])[m])
    # and through an entry point: slice 0 as pred
    sl = r.centres[:, :, 0].contiguous()
    bk = h.best_of_k(sl, t["targets"], t["n_active"], 1, seed=1, n_frames=t["n_frames"],
                     ped_mask=t["ped_mask"], want_per_ped=False)
    want = float(a[0][m].mean())
    assert abs(bk.ade - want) <= mo.TOL * max(1.0, want)


def test_one_slot_mixture_is_the_fullcov_head(gpu):
    from multimodaltraj_2_amd.mixture import MixtureHead
    for name in ("eval", "k65"):
        i = mc.IDS.index(name)
        fc, _ = _device_inputs(i, "fullcov", gpu)
        r = _run(i, "fullcov", gpu, head=MixtureHead.from_fullcov(fc))
        f = _result(i, "fullcov", gpu)
        assert torch.equal(r.per_ped, f.per_ped) and torch.equal(r.out, f.out)
        assert torch.equal(r.centres, f.centres) and torch.equal(r.weights, f.weights)


@pytest.mark.parametrize("which", mc.HEADS)
def test_at_minimum_alignment(gpu, which):
    """Each entry point at the weakest pointer alignment its header line
    states (targets 8, per_ped 16, workspace 8) and every other pointer at its
    element's own (4; the mask 1): the bits of the aligned call."""
    i = mc.IDS.index("shared")
    c = mc.inputs(i)
    S, F, _, N = c["pred"].shape
    M = c["M"]
    h, _ = _device_inputs(i, which, gpu)
    ar = Arena(gpu)
    t = dict(pred=ar.put(c["pred"], "pred", 4), targets=ar.put(c["targets"], "targets", 8),
             n_active=ar.put(c["n_active"], "n_active", 4), n_frames=ar.put(c["n_frames"], "n_frames", 4),
             ped_mask=ar.put(c["ped_mask"], "ped_mask", 1),
             params=ar.put(_params(h, which).cpu().numpy(), "params", 4))
    assert t["targets"].data_ptr() % 16 == 8 and t["pred"].data_ptr() % 16 == 4
    per, out = ar.alloc((S, F, N, 8), name="per_ped"), ar.alloc((S, 8), name="out", offset=4)
    cen = ar.alloc((S, F, M, 24, N), name="centres", offset=4)
    wts = ar.alloc((S, F, M, N), name="weights", offset=12)
    from multimodaltraj_2_amd import modes
    need = modes.load().g2k_sample_modes_workspace_bytes(ctypes.byref(h._dims(_t(c["pred"], "cpu"))))
    ws = ar.alloc((need,), torch.uint8, name="workspace", offset=8)
    assert _raw_call(i, which, gpu, per, cen, wts, out, t=t, ws=ws) == need
    ar.check_guards()
    r = _result(i, which, gpu)
    assert torch.equal(per, r.per_ped) and torch.equal(out, r.out)
    assert torch.equal(cen, r.centres) and torch.equal(wts, r.weights)


def test_workspace_rows_at_minimum_alignment(gpu):
    """The same with several workgroups per scene: the rows of doubles in a
    workspace that is 8 and not 16 bytes aligned."""
    i = mc.IDS.index("passes")
    c = mc.inputs(i)
    S = c["pred"].shape[0]
    h, _ = _device_inputs(i, "fullcov", gpu)
    ar = Arena(gpu)
    from multimodaltraj_2_amd import modes
    need = modes.load().g2k_sample_modes_workspace_bytes(ctypes.byref(h._dims(_t(c["pred"], "cpu"))))
    ws = ar.alloc((need,), torch.uint8, name="workspace", offset=8)
    out = ar.alloc((S, 8), name="out")
    _raw_call(i, "fullcov", gpu, None, None, None, out, ws=ws)
    ar.check_guards()
    assert torch.equal(out, _result(i, "fullcov", gpu).out)


def test_python_argument_checks(gpu):
    for which in mc.HEADS:
        h, t = _device_inputs(0, which, gpu)
        a = (t["pred"], t["targets"], t["n_active"])
        for m in (0, 33):
            with pytest.raises(ValueError, match="modes = "):
                h.sample_modes(*a, 64, m)
        for k, m in ((4, 5), (257, 5), (0, 1)):
            with pytest.raises(ValueError, match="k = "):
                h.sample_modes(*a, k, m)
        for it in (-1, 65):
            with pytest.raises(ValueError, match="iters = "):
                h.sample_modes(*a, 8, 2, it)
        for rad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="miss_radius = "):
                h.sample_modes(*a, 8, 2, miss_radius=rad)
        with pytest.raises(ValueError, match="targets must be"):
            h.sample_modes(t["pred"], t["targets"][:, :, :1], t["n_active"], 8, 2)
        with pytest.raises(ValueError, match="n_active must be"):
            h.sample_modes(t["pred"], t["targets"], t["n_active"][:0], 8, 2)
        r = h.sample_modes(*a, 8, 2)                 # the defaults: per_ped, no centres
        assert r.per_ped is not None and r.centres is None and r.weights is None
        assert (r.k, r.modes, r.iters, r.miss_radius) == (8, 2, 10, 0.0)


def test_evaluation_end_to_end(gpu, tmp_path, data_root):
    """The recipe of tests/test_sample_scores_gpu.py::test_evaluation_end_to_end
    with --num_samples 4 --sample_scores 1: without --sample_modes the keys and
    their order are today's; with --sample_modes 5 --modes_draws 64 the
    MODES_FIGURES and their twins appear directly after each head's score
    figures, finite and equal to a direct call on ``keep``'s tensors, one more
    log line per head; ``modes_miss_rate`` only with --miss_radius > 0; the
    CLI takes the flags; out-of-range flags raise."""
    from multimodaltraj_2_amd import checkpoint, evaluate
    from multimodaltraj_2_amd import train as tr
    from multimodaltraj_2_amd.argParser import ArgsParser
    from multimodaltraj_2_amd.fullcov import FullCovHead
    from multimodaltraj_2_amd.nll import GaussianHead
    argv = ["--data_root", data_root, "--leaveDataset", "2", "--n_max", "32", "--train_scenes", "64",
            "--train_batch", "32", "--num_epochs", "2", "--loss", "l2", "--num_samples", "4",
            "--mode", "train", "--save_dir", str(tmp_path), "--log_dir", str(tmp_path),
            "--device", "cuda:0", "--sample_scores", "1", "--fullcov_head", "train", "--mixture_head",
            "train"]
    args = ArgsParser().parser.parse_args(argv)
    assert (args.sample_modes, args.modes_draws, args.modes_iters, args.miss_radius) == (0, 256, 10, 0.0)
    assert evaluate.MODES_FIGURES == ("modes_min_ade", "modes_min_fde", "modes_brier_ade",
                                      "modes_brier_fde", "modes_inertia", "modes_live")
    args.num_samples = 0                              # train only
    tr.run_train_mode(args, gpu, log=lambda s: None)
    args.num_samples = 4
    prm = checkpoint.load_params(checkpoint.read_state(str(tmp_path)), device=gpu)
    logs0, keep0 = [], {}
    res0 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs0.append, keep=keep0)
    base = ["scenes", "pairs", "K"] + list(evaluate.FIGURES) + list(evaluate.SCORE_FIGURES)
    assert list(res0) == (base + list(evaluate.FULLCOV_FIGURES) + list(evaluate.FULLCOV_SCORE_FIGURES)
                          + list(evaluate.MIX_FIGURES) + list(evaluate.MIX_SCORE_FIGURES))
    assert "modes" not in keep0 and "modes" not in keep0["fullcov"] and "modes" not in keep0["mixture"]
    assert not any("sample modes" in s for s in logs0)

    args.sample_modes, args.modes_draws = 5, 64
    logs1, keep1 = [], {}
    res1 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs1.append, keep=keep1)
    F_, X_ = evaluate.FULLCOV_MODES_FIGURES, evaluate.MIX_MODES_FIGURES
    assert F_ == tuple("fullcov_" + k for k in evaluate.MODES_FIGURES)
    assert X_ == tuple("mix_" + k for k in evaluate.MODES_FIGURES)
    assert list(res1) == (base + list(evaluate.MODES_FIGURES)
                          + list(evaluate.FULLCOV_FIGURES) + list(evaluate.FULLCOV_SCORE_FIGURES) + list(F_)
                          + list(evaluate.MIX_FIGURES) + list(evaluate.MIX_SCORE_FIGURES) + list(X_))
    assert {k: res1[k] for k in res0} == res0 and len(logs1) == len(logs0) + 3
    assert [s for s in logs1 if "sample modes" not in s] == logs0
    t = keep1["plan"].to_device(gpu, F=1)
    one = torch.ones(keep1["plan"].S, dtype=torch.int32, device=gpu)
    gh = GaussianHead(device=gpu)
    gh.head = keep1["head"]
    fc = FullCovHead(device=gpu)
    fc.chol = keep1["fullcov_chol"]
    mx = keep1["mixture"]["head"]
    kw = dict(seed=args.sample_seed, n_frames=one, ped_mask=t["ped_mask"])
    for head, prefix, kept, name in ((gh, "", keep1["modes"], "sample modes"),
                                     (fc, "fullcov_", keep1["fullcov"]["modes"],
                                      "full-covariance sample modes"),
                                     (mx, "mix_", keep1["mixture"]["modes"], "mixture sample modes")):
        direct = head.sample_modes(keep1["pred"], t["targets"], t["n_active"], 64, 5, 10, **kw)
        want = evaluate.modes_figures(direct, prefix)
        assert tuple(want) == tuple(prefix + k for k in evaluate.MODES_FIGURES)
        for k, v in want.items():
            print(f"evaluation {k}: {res1[k]:.8g}")
            assert np.isfinite(res1[k]) and res1[k] == v, k
        assert torch.equal(kept.out, direct.out) and torch.equal(kept.per_ped, direct.per_ped)
        assert direct.pairs == res1["pairs"] and kept.centres is None
        line = [s for s in logs1 if s.startswith(f"{name} on dataset 2: 5 centres of 64 draws after 10 ")]
        assert len(line) == 1
        assert f"minADE_5 {res1[prefix + 'modes_min_ade']:.6g}" in line[0]
        assert f"{res1[prefix + 'min_ade']:.6g} / {res1[prefix + 'min_fde']:.6g}" in line[0]
        assert "miss rate" not in line[0]
        assert 1.0 <= res1[prefix + "modes_live"] <= 5.0
        # the first --num_samples draws are the best-of-K call's own: five centres of four draws'
        # superset cannot be compared value for value, but no iteration at M = K = 4 can
        same = head.sample_modes(keep1["pred"], t["targets"], t["n_active"], 4, 4, 0, **kw)
        assert abs(same.min_ade - res1[prefix + "min_ade"]) <= mo.TOL * max(1.0, res1[prefix + "min_ade"])
        assert abs(same.min_fde - res1[prefix + "min_fde"]) <= mo.TOL * max(1.0, res1[prefix + "min_fde"])

    # the miss rate: only with --miss_radius > 0, after the head's MODES_FIGURES
    args.miss_radius = 0.5
    logs2 = []
    res2 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs2.append)
    order = list(res2)
    for prefix in ("", "fullcov_", "mix_"):
        k = prefix + "modes_miss_rate"
        assert k not in res1 and order[order.index(k) - 1] == prefix + "modes_live"
        assert 0.0 <= res2[k] <= 1.0
    assert [k for k in order if not k.endswith("modes_miss_rate")] == list(res1)
    assert {k: res2[k] for k in res1} == res1
    assert sum("miss rate at 0.5 " in s for s in logs2) == 3
    # the CLI
    cli = evaluate.main(argv + ["--sample_modes", "5", "--modes_draws", "64", "--miss_radius", "0.5"],
                        log=lambda s: None)
    assert list(cli) == list(res2) and [cli[k] for k in res2] == [res2[k] for k in res2]
    # out-of-range flags
    for name, bad in (("sample_modes", 33), ("sample_modes", -1), ("modes_draws", 4), ("modes_draws", 257),
                      ("modes_iters", -1), ("modes_iters", 65), ("miss_radius", -0.5),
                      ("miss_radius", float("inf"))):
        old = getattr(args, name)
        setattr(args, name, bad)
        with pytest.raises(ValueError, match="--" + name):
            evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
        setattr(args, name, old)
