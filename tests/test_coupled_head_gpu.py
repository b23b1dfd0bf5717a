"""GPU: the scene-coupled head (g2k_coupled_stats_f32, g2k_coupled_sample_f32,
csrc/g2k_coupled.hip; g2k_coupled_joint_eval_f32, csrc/g2k_joint.hip;
g2k_coupled_couple_scores_f32, csrc/g2k_couples.hip; coupled.CoupledHead;
evaluate.py) against the float64 checker tests/coupled_ref.py.  PARITY UNPINNED
against the reference (it has no probabilistic head).

The stats' sums are doubles of exact f32 differences: held to 1e-12 max(1,
|ref|), tests/test_fullcov_gpu.py's bound for ``moments``; the counts equal.
The sampler is held to that file's bound for the full-covariance sampler, 1e-4
max(1, |ref|), and with Lb = 0 to the BITS of g2k_fullcov_sample_f32.  The two
fused calls are compared with their checkers (tests/couples_ref.py,
tests/fullcov_joint_ref.recount) fed with the DEVICE's own K sampler draws, as
tests/test_couple_scores_gpu.py and tests/test_fullcov_joint_gpu.py do, at
those files' tolerances; with Lb = 0 every output bit is the ``fullcov_`` twin's."""
import ctypes

import numpy as np
import pytest
import torch

from tests import coupled_cases as cx
from tests import coupled_ref as cr
from tests import couples_ref as cpr
from tests import fullcov_joint_ref as fj
from tests import fullcov_ref as fr
from tests import test_fullcov_joint_gpu as tj
from tests.abi_arena import Arena, all_written
from tests.bestk_ref import BOUNDARY_SEEDS, MASK64, draw_errors
from tests.conftest import close
from tests.scores_ref import TOL as CPL_TOL
from tests.test_coupled_head import PROP, property_check, property_pred, property_targets
from tests.test_couple_scores_gpu import _check_against

pytestmark = pytest.mark.gpu
DIM = 24
TOL = 1e-4                      # tests/test_fullcov_gpu.py's for the sampler; the joint tests' for JADE / JFDE
REL = tj.REL


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(a, b):
    return torch.equal(a.view(torch.int64 if a.element_size() == 8 else torch.int32),
                       b.view(torch.int64 if b.element_size() == 8 else torch.int32))


def _head(cpl, dev):
    """The head with exactly these parameters (NaN above the diagonals included)."""
    from multimodaltraj_2_amd.coupled import CoupledHead
    h = CoupledHead(device=dev)
    h.cpl = cpl if isinstance(cpl, torch.Tensor) else _t(cpl, dev)
    return h


def _fullcov(chol, dev):
    from multimodaltraj_2_amd.fullcov import FullCovHead
    fc = FullCovHead(device=dev)
    fc.chol = chol if isinstance(chol, torch.Tensor) else _t(chol, dev)
    return fc


def _dev_inputs(c, dev):
    return {k: _t(c[k], dev) for k in ("pred", "targets", "n_active", "n_frames", "ped_mask")}


# ---------------------------------------------------------------------------
# stats
# ---------------------------------------------------------------------------
_ST = {}


def _stats(j, dev, use_head=True):
    if (j, use_head) not in _ST:
        c = cx.stats_inputs(j)
        t = _dev_inputs(c, dev)
        h = _head(c["cpl"], dev)
        r = h.stats(t["pred"], t["targets"], t["n_active"], n_frames=t["n_frames"], ped_mask=t["ped_mask"],
                    targets_shared=c["shared"], use_head=use_head)
        torch.cuda.synchronize()
        _ST[(j, use_head)] = (h, t, r)
    return _ST[(j, use_head)]


@pytest.mark.parametrize("j", range(len(cx.STATS)), ids=cx.STATS_IDS)
def test_stats_match_checker(gpu, j):
    """within, between and stats at 1e-12 max(1, |ref|), the counts equal; the
    inputs' NaN (non-members, frames >= n_frames, above the factors' diagonals)
    was never read; without a head stats is exact zeros and the sums' bits are
    the same; a second call repeats every bit."""
    c = cx.stats_inputs(j)
    h, t, r = _stats(j, gpu)
    A, lam = h.whitener()
    R = cr.stats_ref(c["pred"], c["targets"], c["n_active"], (A, lam), c["n_frames"], c["ped_mask"])
    got = {k: getattr(r, k).cpu().numpy() for k in ("within", "between", "stats", "counts")}
    err = {k: close(got[k], R[k], 1e-12) for k in ("within", "between", "stats")}
    print(f"case {cx.STATS_IDS[j]}: counts {list(got['counts'])}, errors {err}")
    np.testing.assert_array_equal(got["counts"], R["counts"])
    assert got["counts"].dtype == np.int64
    for k, e in err.items():
        assert np.isfinite(got[k]).all() and e <= 1e-12, k
    np.testing.assert_array_equal(got["within"], got["within"].T)
    np.testing.assert_array_equal(got["between"], got["between"].T)
    n = int(R["counts"][0])
    if n:
        assert r.pairs == n and r.groups == int(R["counts"][1])
        const = 12 * cr.LOG_2PI + float(np.log(np.diag(fr.lower(c["cpl"][0]))).sum())
        assert r.nll == pytest.approx(R["stats"][0] / n + const, rel=1e-11)
        assert r.nll_independent == pytest.approx(R["stats"][1] / n + const, rel=1e-11)
        assert r.nll_gain == pytest.approx((R["stats"][1] - R["stats"][0]) / n, rel=1e-9, abs=1e-12)
    else:
        assert not got["within"].any() and not got["between"].any() and not got["stats"].any()
        assert np.isnan(r.nll)
    _, _, r0 = _stats(j, gpu, use_head=False)
    assert not r0.stats.cpu().numpy().any() and r0.nll is None
    assert _same(r0.within, r.within) and _same(r0.between, r.between) and torch.equal(r0.counts, r.counts)
    again = h.stats(t["pred"], t["targets"], t["n_active"], n_frames=t["n_frames"], ped_mask=t["ped_mask"],
                    targets_shared=c["shared"])
    assert _same(again.within, r.within) and _same(again.between, r.between) and _same(again.stats, r.stats)
    assert torch.equal(again.counts, r.counts)


def _raw_stats(c, t, dev, whiten, within, between, counts, stats, ws=None, S=None, F=None):
    from multimodaltraj_2_amd import _lib, coupled
    from multimodaltraj_2_amd.frame_step import _ptr
    lib = coupled.load()
    S0, F0, _, N = c["pred"].shape
    d = _lib.G2KDims(S0 if S is None else S, F0 if F is None else F, 8, 12, 16, 64, N, 8,
                     _lib.STEP_TARGETS_SHARED if c["shared"] else 0)
    need = int(lib.g2k_coupled_stats_workspace_bytes(ctypes.byref(d)))
    if ws is None:
        ws = torch.empty(max(8, need), dtype=torch.uint8, device=dev)
    rc_ = lib.g2k_coupled_stats_f32(ctypes.byref(d), _ptr(t["pred"]), _ptr(t["targets"]), _ptr(t["n_active"]),
                                    _ptr(t["n_frames"]), _ptr(t["ped_mask"]), _ptr(whiten), _ptr(within),
                                    _ptr(between), _ptr(counts), _ptr(stats), _ptr(ws), need, None)
    torch.cuda.synchronize()
    assert rc_ == 0, lib.g2k_last_error()
    return need


@pytest.mark.parametrize("name", ["k2", "reach", "nopair"])
def test_stats_write_footprint(gpu, name):
    """Guarded, poisoned outputs: every element written, nothing outside, with
    and without whiten, on one workgroup and on the rows path; F = 0 writes
    zeros."""
    j = cx.STATS_IDS.index(name)
    c = cx.stats_inputs(j)
    h, t, r = _stats(j, gpu)
    A, lam = h.whitener()
    wh = _t(np.concatenate([A, lam[None]]), gpu)
    for whiten in (wh, None):
        ar = Arena(gpu)
        o = dict(within=ar.alloc((DIM, DIM), torch.float64, name="within"),
                 between=ar.alloc((DIM, DIM), torch.float64, name="between"),
                 counts=ar.alloc((4,), torch.int64, name="counts"), stats=ar.alloc((6,), torch.float64, name="stats"))
        _raw_stats(c, t, gpu, whiten, **o)
        ar.check_guards()
        assert all(all_written(v) for v in o.values())
        assert _same(o["within"], r.within) and _same(o["between"], r.between) and torch.equal(o["counts"], r.counts)
        if whiten is not None:
            assert _same(o["stats"], r.stats)
        else:
            assert not bool(o["stats"].any())
    ar = Arena(gpu)
    o = dict(within=ar.alloc((DIM, DIM), torch.float64), between=ar.alloc((DIM, DIM), torch.float64),
             counts=ar.alloc((4,), torch.int64), stats=ar.alloc((6,), torch.float64))
    _raw_stats(c, t, gpu, wh, F=0, **o)
    ar.check_guards()
    assert all(all_written(v) and not bool(v.any()) for v in o.values())


def test_stats_at_minimum_alignment(gpu):
    """targets, whiten, the four outputs and the workspace 8 bytes past a
    16-byte boundary, pred 4: the bits of the aligned call (the rows path)."""
    j = cx.STATS_IDS.index("reach")
    c = cx.stats_inputs(j)
    h, _, r = _stats(j, gpu)
    A, lam = h.whitener()
    ar = Arena(gpu)
    t = dict(pred=ar.put(c["pred"], "pred", 4), targets=ar.put(c["targets"], "targets", 8),
             n_active=ar.put(c["n_active"], "n_active", 4), n_frames=None, ped_mask=None)
    wh = ar.put(np.concatenate([A, lam[None]]), "whiten", 8)
    o = dict(within=ar.alloc((DIM, DIM), torch.float64, offset=8), between=ar.alloc((DIM, DIM), torch.float64, offset=8),
             counts=ar.alloc((4,), torch.int64, offset=8), stats=ar.alloc((6,), torch.float64, offset=8))
    from multimodaltraj_2_amd import coupled
    S, F, _, N = c["pred"].shape
    need = cx.stats_geometry(S, F, N)[0] * 920 * 8
    ws = ar.alloc((need,), torch.uint8, name="workspace", offset=8)
    assert _raw_stats(c, t, gpu, wh, ws=ws, **o) == need > 0
    ar.check_guards()
    assert coupled.load() is not None
    assert _same(o["within"], r.within) and _same(o["between"], r.between) and _same(o["stats"], r.stats)
    assert torch.equal(o["counts"], r.counts)


def test_fit_sets_the_factors_and_refuses_single_members(gpu):
    """fit = one stats launch and the host projection: the checker's factors;
    N == G and no pair raise before anything is set."""
    j = cx.STATS_IDS.index("reach")
    c = cx.stats_inputs(j)
    t = _dev_inputs(c, gpu)
    from multimodaltraj_2_amd.coupled import CoupledHead
    h = CoupledHead(device=gpu)
    st = h.fit(t["pred"], t["targets"], t["n_active"])
    s = cr.sums(cr.group_residuals(c["pred"], c["targets"], c["n_active"]))
    want = cr.project(*cr.moments_fit(s["within"], s["between"], s["counts"]))
    Lw, Lb = h.cpl[0].double().cpu().numpy(), h.cpl[1].double().cpu().numpy()
    assert close(Lw, want["Lw"]) <= TOL and close(Lb @ Lb.T, want["Lb"] @ want["Lb"].T) <= TOL
    assert h.clipped == want["clipped"] and st.pairs == int(s["counts"][0]) and st.nll is None
    np.testing.assert_allclose(h.whitener()[1], want["lam"], rtol=1e-8, atol=1e-10)
    # the fitted head's own calibration on the data it was fitted on
    at = h.stats(t["pred"], t["targets"], t["n_active"])
    assert at.q_within_ratio == pytest.approx(1.0, abs=1e-4) and np.isfinite(at.nll_gain)
    for name in ("single", "nopair"):
        c1 = cx.stats_inputs(cx.STATS_IDS.index(name))
        t1 = _dev_inputs(c1, gpu)
        h1 = CoupledHead(device=gpu)
        with pytest.raises(ValueError, match="two members"):
            h1.fit(t1["pred"], t1["targets"], t1["n_active"], n_frames=t1["n_frames"])
        assert torch.equal(h1.cpl[0], torch.eye(DIM, device=gpu)) and not bool(h1.cpl[1].any())


# ---------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------
SAMPLE = ["k2", "k20", "reach", "k23", "n256"]


@pytest.mark.parametrize("name", SAMPLE)
def test_sampler_matches_checker(gpu, name):
    """1e-4 max(1, |ref|) at the members, the full-covariance sampler's bound
    (measured here: below 1e-6); every element written; the seed wraps."""
    i = cx.IDS.index(name)
    c = cx.inputs(i)
    h = _head(c["cpl"], gpu)
    pred_h = np.nan_to_num(c["pred"])                        # the sampler draws every column
    pred = _t(pred_h, gpu)
    for seed in (c["seed"], (1 << 64) - 1):
        x = h.sample(pred, seed=seed).cpu().numpy()
        ref = cr.sample(pred_h, c["cpl"], seed)
        err = close(x, ref)
        print(f"case {name} seed {seed}: sampler err {err:.3g}")
        assert np.isfinite(x).all() and err <= TOL
    ar = Arena(gpu)
    out = ar.alloc(c["pred"].shape, name="out", offset=4)
    p4 = ar.put(pred_h, "pred", 4)
    cpl4 = ar.put(c["cpl"], "cpl", 4)
    from multimodaltraj_2_amd import _lib, coupled
    from multimodaltraj_2_amd.frame_step import _ptr
    S, F, _, N = c["pred"].shape
    d = _lib.G2KDims(S, F, 8, 12, 16, 64, N, 8, 0)
    assert coupled.load().g2k_coupled_sample_f32(ctypes.byref(d), _ptr(p4), _ptr(cpl4), ctypes.c_uint64(c["seed"]),
                                                 _ptr(out), None) == 0
    torch.cuda.synchronize()
    ar.check_guards()
    assert all_written(out) and torch.equal(out, h.sample(pred, seed=c["seed"]))


@pytest.mark.parametrize("name", SAMPLE)
def test_zero_lb_is_the_fullcov_sampler_bit_for_bit(gpu, name):
    i = cx.IDS.index(name)
    c = cx.inputs(i)
    cpl = np.stack([c["chol"], np.zeros((DIM, DIM), np.float32)])
    cpl[0][np.triu_indices(DIM, 1)] = np.nan
    pred = _t(np.nan_to_num(c["pred"]), gpu)
    h, fc = _head(cpl, gpu), _fullcov(cpl[0], gpu)
    for seed in (c["seed"], c["seed"] + 1, (1 << 64) - 1):
        assert torch.equal(h.sample(pred, seed=seed), fc.sample(pred, seed=seed & MASK64))


def test_members_of_a_scene_frame_share_c(gpu):
    """Lw = 1e-6 I (a zero diagonal is outside the contract): x - mu is c up to
    1e-5 for every column of a scene-frame, and differs between scene-frames."""
    i = cx.IDS.index("reach")
    c = cx.inputs(i)
    cpl = np.stack([1e-6 * np.eye(DIM, dtype=np.float32), np.nan_to_num(c["cpl"][1])])
    pred_h = np.nan_to_num(c["pred"])
    x = _head(cpl, gpu).sample(_t(pred_h, gpu), seed=c["seed"]).cpu().numpy().astype(np.float64)
    d = x - pred_h                                           # [S, F, 24, N]
    want = cr.shared_part(pred_h.shape, cpl[1], c["seed"])   # [S, F, 1, 24] time-major
    band = np.concatenate([want[..., 0::2], want[..., 1::2]], axis=-1)[:, :, 0, :, None]
    print(f"spread within a scene-frame {np.ptp(d, axis=3).max():.3g}, |c| mean {np.abs(band).mean():.3g}")
    assert np.ptp(d, axis=3).max() <= 2e-5 and np.abs(d - band).max() <= 1e-4
    assert np.abs(band).mean() > 0.05 and np.abs(d[0, 0] - d[0, 1]).mean() > 0.05


# ---------------------------------------------------------------------------
# couple scores
# ---------------------------------------------------------------------------
CPL = ["k2", "k20", "reach", "k64", "k23", "shared", "n256"]
_CP, _DRAWS = {}, {}


def _cpl_case(name, dev):
    i = cx.IDS.index(name)
    if name not in _CP:
        c = cx.inputs(i)
        _CP[name] = (c, _head(c["cpl"], dev), _dev_inputs(c, dev))
    return _CP[name]


def _cpl_run(name, dev, head=None, k=None, bins=None, seed=None, **kw):
    c, h, t = _cpl_case(name, dev)
    r = (head or h).couple_scores(t["pred"], t["targets"], t["n_active"], k or c["K"], bins or c["B"],
                                  seed=c["seed"] if seed is None else seed,
                                  reach=None if np.isinf(c["reach"]) else c["reach"], n_frames=t["n_frames"],
                                  ped_mask=t["ped_mask"], targets_shared=c["shared"],
                                  **dict(dict(want_per_couple=True, want_per_frame=True), **kw))
    torch.cuda.synchronize()
    return r


def _cpl_draws(name, dev, seed=None):
    """The device's own K joint draws [K, S, F, 24, N] float32 (made once)."""
    key = name if seed is None else (name, seed)
    if key not in _DRAWS:
        c, h, t = _cpl_case(name, dev)
        s0 = c["seed"] if seed is None else seed
        _DRAWS[key] = np.stack([h.sample(t["pred"], seed=(s0 + k) & MASK64).cpu().numpy()
                                for k in range(c["K"])]).astype(np.float32)
    return _DRAWS[key]


def _cpl_parity(dev, name, seed=None, label=""):
    c, h, t = _cpl_case(name, dev)
    r = _cpl_run(name, dev, seed=seed)
    R = cpr.couple_scores_ref(_cpl_draws(name, dev, seed), c["targets"], c["pred"], c["members"], c["K"], c["B"],
                              c["reach"])
    _check_against(r, R, f"coupled, case {name}{label}")
    assert CPL_TOL <= 1e-4
    again = _cpl_run(name, dev, seed=seed)
    assert torch.equal(again.per_couple, r.per_couple) and _same(again.per_frame_f, r.per_frame_f)
    assert _same(again.sums, r.sums) and torch.equal(again.hist, r.hist) and torch.equal(again.tot, r.tot)
    no = _cpl_run(name, dev, seed=seed, want_per_couple=False, want_per_frame=False)
    assert no.per_couple is None and _same(no.sums, r.sums) and torch.equal(no.hist, r.hist)


@pytest.mark.parametrize("name", CPL)
def test_couple_scores_against_the_devices_own_draws(gpu, name):
    """per_couple, per_frame_i, hist and tot EQUAL to the float32 restatement,
    the fp32 sums within scores_ref.TOL a couple; a second call repeats the bits."""
    _cpl_parity(gpu, name)


@pytest.mark.parametrize("at", BOUNDARY_SEEDS)
def test_couple_scores_at_a_seed_whose_low_word_carries(gpu, at):
    """Case k2 with the same assertions at the seeds where draw 1's seed carries
    out of the low word (A = 2^32 - 1) and wraps to 0 (W = 2^64 - 1): the salt is
    XORed into the halves after the carry (csrc/g2k_couples.hip,
    CoupledHead::draw).  tests/test_coupled_head.py: the checker's integer
    outputs change when the carry is dropped."""
    _cpl_parity(gpu, "k2", BOUNDARY_SEEDS[at], f" seed {at}")


@pytest.mark.parametrize("name", CPL)
def test_couple_scores_with_zero_lb_are_the_fullcov_twins(gpu, name):
    c, _, t = _cpl_case(name, gpu)
    cpl = np.stack([c["chol"], np.zeros((DIM, DIM), np.float32)])
    a = _cpl_run(name, gpu, head=_head(cpl, gpu))
    b = _cpl_run(name, gpu, head=_fullcov(c["chol"], gpu))
    assert torch.equal(a.per_couple, b.per_couple) and torch.equal(a.per_frame_i, b.per_frame_i)
    assert _same(a.per_frame_f, b.per_frame_f) and _same(a.sums, b.sums)
    assert torch.equal(a.hist, b.hist) and torch.equal(a.tot, b.tot)
    if a.couples:
        assert not torch.equal(a.per_couple, _cpl_run(name, gpu).per_couple)        # Lb matters


def test_couple_scores_first_draws_of_k_are_the_draws_of_fewer(gpu):
    c, h, t = _cpl_case("k20", gpu)
    r = _cpl_run("k20", gpu, k=6, bins=7)
    R = cpr.couple_scores_ref(_cpl_draws("k20", gpu)[:6], c["targets"], c["pred"], c["members"], 6, 7, c["reach"])
    _check_against(r, R, "coupled, case k20 at K' = 6")


def _raw_couples(name, dev, pc, pf, pi, sums, hist, tot, t=None, ws=None):
    from multimodaltraj_2_amd import _lib, coupled
    from multimodaltraj_2_amd.frame_step import _ptr
    lib = coupled.load()
    c, h, t0 = _cpl_case(name, dev)
    t = t or dict(t0, params=h.cpl)
    d = h._dims(t0["pred"])
    if c["shared"]:
        d.flags = _lib.STEP_TARGETS_SHARED
    need = int(lib.g2k_couple_scores_workspace_bytes(ctypes.byref(d), c["K"], c["B"]))
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc_ = lib.g2k_coupled_couple_scores_f32(ctypes.byref(d), _ptr(t["pred"]), _ptr(t["targets"]), _ptr(t["n_active"]),
                                            _ptr(t["n_frames"]), _ptr(t["ped_mask"]), _ptr(t["params"]),
                                            ctypes.c_uint64(c["seed"]), c["K"], c["B"], c["reach"], _ptr(pc),
                                            _ptr(pf), _ptr(pi), _ptr(sums), _ptr(hist), _ptr(tot), _ptr(ws), need,
                                            None)
    torch.cuda.synchronize()
    assert rc_ == 0, lib.g2k_last_error()
    return need


def _cpl_outs(ar, c, off4=0, off8=0):
    S, F, _, N = c["pred"].shape
    return dict(pc=ar.alloc((S, F, N, N), torch.int32, name="per_couple", offset=off4),
                pf=ar.alloc((S, F, 8), name="per_frame_f", offset=off4),
                pi=ar.alloc((S, F, 4), torch.int32, name="per_frame_i", offset=off4),
                sums=ar.alloc((S, 8), name="sums", offset=off4),
                hist=ar.alloc((S, 2, c["B"]), torch.int32, name="hist", offset=off4),
                tot=ar.alloc((S, 4), torch.int64, name="tot", offset=off8))


@pytest.mark.parametrize("name", ["k2", "k20", "reach", "k23"])
def test_couple_scores_write_footprint(gpu, name):
    c, h, t = _cpl_case(name, gpu)
    ar = Arena(gpu)
    o = _cpl_outs(ar, c)
    _raw_couples(name, gpu, **o)
    ar.check_guards()
    assert all(all_written(v) for v in o.values())
    r = _cpl_run(name, gpu)
    assert torch.equal(o["pc"], r.per_couple) and _same(o["pf"], r.per_frame_f) and torch.equal(o["pi"], r.per_frame_i)
    assert _same(o["sums"], r.sums) and torch.equal(o["hist"], r.hist) and torch.equal(o["tot"], r.tot)
    o2 = _cpl_outs(ar, c)
    _raw_couples(name, gpu, **dict(o2, pc=None, pf=None, pi=None))
    ar.check_guards()
    assert _same(o2["sums"], r.sums) and torch.equal(o2["hist"], r.hist) and torch.equal(o2["tot"], r.tot)
    assert not bool(torch.isnan(o["pf"]).any()) and not bool(torch.isnan(o["sums"]).any())   # the poison was never read


def test_couple_scores_at_minimum_alignment(gpu):
    from multimodaltraj_2_amd import coupled
    name = "shared"
    c, h, _ = _cpl_case(name, gpu)
    ar = Arena(gpu)
    t = dict(pred=ar.put(c["pred"], "pred", 4), targets=ar.put(c["targets"], "targets", 8),
             n_active=ar.put(c["n_active"], "n_active", 4), n_frames=ar.put(c["n_frames"], "n_frames", 4),
             ped_mask=ar.put(c["ped_mask"], "ped_mask", 1), params=ar.put(c["cpl"], "cpl", 4))
    o = _cpl_outs(ar, c, 4, 8)
    need = coupled.load().g2k_couple_scores_workspace_bytes(ctypes.byref(h._dims(_t(c["pred"], "cpu"))), c["K"], c["B"])
    ws = ar.alloc((need,), torch.uint8, name="workspace", offset=4)
    assert _raw_couples(name, gpu, t=t, ws=ws, **o) == need
    ar.check_guards()
    r = _cpl_run(name, gpu)
    assert torch.equal(o["pc"], r.per_couple) and _same(o["pf"], r.per_frame_f) and torch.equal(o["pi"], r.per_frame_i)
    assert _same(o["sums"], r.sums) and torch.equal(o["hist"], r.hist) and torch.equal(o["tot"], r.tot)


# ---------------------------------------------------------------------------
# joint evaluation: tests/test_fullcov_joint_gpu.py's smallest cases that reach
# joint_wave_kernel (Nmax <= 64: s5f3n20k20, shared, wrap, n64) and joint_kernel
# (n256waves)
# ---------------------------------------------------------------------------
JOINT = ["s5f3n20k20", "shared", "wrap", "n64", "n256waves"]
RADIUS = 0.3
_JT = {}


def _joint_case(name, dev):
    if name not in _JT:
        i = tj.IDS.index(name)
        c = dict(tj._inputs(i))
        sigma = tj.CASES[i][4]
        Lb = fj.nan_above(0.8 * fj.walk_factor(sigma, np.random.default_rng(4000 + i)))
        c["cpl"] = np.stack([fj.nan_above(np.float32(np.sqrt(0.5)) * np.nan_to_num(c["chol"])), Lb])
        _JT[name] = (c, _head(c["cpl"], dev))
    return _JT[name]


def _joint_run(name, dev, head=None, K=None, **over):
    c, h = _joint_case(name, dev)
    a, kw = tj._args(c, dev)
    kw.update(over)
    r = (head or h).joint_eval(*a, K or c["K"], RADIUS, seed=c["seed"], **kw)
    torch.cuda.synchronize()
    return r


def _joint_check(c, r, xs, K, label):
    """The kernel against float64 recomputation from the device's own draws."""
    pf, pi, sf, si = tj._host(r)
    S, F, _, N = c["pred"].shape
    from tests.bestk_ref import pair_mask
    m = pair_mask(S, F, N, c["n_active"], c["n_frames"], c["ped_mask"])
    P = m.sum(axis=2)
    np.testing.assert_array_equal(pi[..., 0], P)
    np.testing.assert_array_equal(pi[..., 1], P * (P - 1) // 2)
    np.testing.assert_array_equal(si, pi.sum(axis=1))
    lo, hi, amb = fj.recount(xs, m, RADIUS, REL)
    tj.assert_cap(int(amb.sum()), K * int(pi[..., 1].sum()), int(lo.sum()), label)
    assert tj._between(lo.sum(axis=0), pi[..., 4], hi.sum(axis=0))
    kJA = pf[..., 2].astype(np.int64)
    on = P > 0
    assert tj._between(np.take_along_axis(lo, kJA[None], axis=0)[0][on], pi[..., 5][on],
                       np.take_along_axis(hi, kJA[None], axis=0)[0][on])
    Pd = np.maximum(P, 1)
    jade, jfde = np.empty(lo.shape), np.empty(lo.shape)
    for k in range(K):
        a, f = draw_errors(xs[k].astype(np.float64), c["targets"])
        jade[k], jfde[k] = (a * m).sum(axis=2) / Pd, (f * m).sum(axis=2) / Pd
    err = close(pf[..., 0], jade.min(axis=0) * on), close(pf[..., 1], jfde.min(axis=0) * on)
    print(f"{label}: minJADE / minJFDE vs float64 from the device's draws {err[0]:.3g} / {err[1]:.3g}, "
          f"sum col_k {pi[..., 4].sum()} in [{lo.sum()}, {hi.sum()}]")
    assert max(err) <= TOL
    assert close(np.take_along_axis(jade, kJA[None], axis=0)[0] * on, jade.min(axis=0) * on) <= TOL
    assert np.all(sf[:, 2] == K) and np.all(sf[:, 3] == 0) and np.all(pf[~on] == 0) and np.all(pi[~on] == 0)
    return pi


@pytest.mark.parametrize("name", JOINT)
def test_joint_eval_against_the_devices_own_draws(gpu, name):
    c, h = _joint_case(name, gpu)
    pred = _t(c["pred"], gpu)
    xs = np.stack([h.sample(pred, seed=(c["seed"] + k) & MASK64).cpu().numpy() for k in range(c["K"])])
    r = _joint_run(name, gpu)
    _joint_check(c, r, xs, c["K"], f"coupled joint, case {name}")
    # the columns that do not depend on the head are the twin's
    fc = _joint_run(name, gpu, head=_fullcov(c["chol"], gpu))
    assert torch.equal(r.per_frame_i[..., :4], fc.per_frame_i[..., :4])
    again = _joint_run(name, gpu)
    assert _same(again.per_frame_f, r.per_frame_f) and torch.equal(again.per_frame_i, r.per_frame_i)
    assert _same(again.sums_f, r.sums_f) and torch.equal(again.sums_i, r.sums_i)
    no = _joint_run(name, gpu, want_per_frame=False)
    assert no.per_frame_f is None and _same(no.sums_f, r.sums_f) and torch.equal(no.sums_i, r.sums_i)
    if c["K"] > 2:                                           # the first draws of K are the draws of fewer
        _joint_check(c, _joint_run(name, gpu, K=2), xs[:2], 2, f"coupled joint, case {name} at K' = 2")


@pytest.mark.parametrize("name", JOINT)
def test_joint_eval_with_zero_lb_is_the_fullcov_twin(gpu, name):
    c, _ = _joint_case(name, gpu)
    cpl = np.stack([c["chol"], np.zeros((DIM, DIM), np.float32)])
    a = _joint_run(name, gpu, head=_head(cpl, gpu))
    b = _joint_run(name, gpu, head=_fullcov(c["chol"], gpu))
    assert _same(a.per_frame_f, b.per_frame_f) and torch.equal(a.per_frame_i, b.per_frame_i)
    assert _same(a.sums_f, b.sums_f) and torch.equal(a.sums_i, b.sums_i)
    assert not _same(a.per_frame_f, _joint_run(name, gpu).per_frame_f)                  # Lb matters


@pytest.mark.parametrize("name", ["s5f3n20k20", "n256waves"])
def test_joint_eval_footprint_at_minimum_alignment(gpu, name):
    """Guarded outputs, targets and sums_i 8 bytes and the rest 4 bytes past a
    16-byte boundary: every element written, the bits of the Python call."""
    from multimodaltraj_2_amd import _lib, coupled
    from multimodaltraj_2_amd.frame_step import _ptr
    lib = coupled.load()
    c, h = _joint_case(name, gpu)
    S, F, _, N = c["pred"].shape
    ar = Arena(gpu)
    pred, tg = ar.put(c["pred"], "pred", 4), ar.put(c["targets"], "targets", 8)
    na = ar.put(c["n_active"], "n_active", 4)
    nf = None if c["n_frames"] is None else ar.put(c["n_frames"], "n_frames", 4)
    pm = None if c["ped_mask"] is None else ar.put(c["ped_mask"], "ped_mask", 1)
    cpl = ar.put(c["cpl"], "cpl", 4)
    pf, pi = ar.alloc((S, F, 4), name="per_frame_f", offset=4), ar.alloc((S, F, 6), torch.int32, name="per_frame_i", offset=4)
    sf, si = ar.alloc((S, 4), name="sums_f", offset=4), ar.alloc((S, 6), torch.int64, name="sums_i", offset=8)
    d = _lib.G2KDims(S, F, 8, 12, 16, 64, N, 8, _lib.STEP_TARGETS_SHARED if c["shared"] else 0)
    need = int(lib.g2k_coupled_joint_eval_workspace_bytes(ctypes.byref(d)))
    ws = ar.alloc((need,), torch.uint8, name="workspace", offset=4)
    rc_ = lib.g2k_coupled_joint_eval_f32(ctypes.byref(d), _ptr(pred), _ptr(tg), _ptr(na), _ptr(nf), _ptr(pm),
                                         _ptr(cpl), ctypes.c_uint64(c["seed"]), c["K"], RADIUS, _ptr(pf), _ptr(pi),
                                         _ptr(sf), _ptr(si), _ptr(ws), need, None)
    torch.cuda.synchronize()
    assert rc_ == 0, lib.g2k_last_error()
    ar.check_guards()
    assert all(all_written(v) for v in (pf, pi, sf, si))
    r = _joint_run(name, gpu)
    assert _same(pf, r.per_frame_f) and torch.equal(pi, r.per_frame_i) and _same(sf, r.sums_f) and torch.equal(si, r.sums_i)


# ---------------------------------------------------------------------------
# what the head is for, on the device
# ---------------------------------------------------------------------------
def test_coupled_targets_are_matched_on_the_device(gpu):
    """tests/test_coupled_head.py's property with the device's fit, sampler and
    fused call: CoupledHead.fit on the first target set, couple_scores on the
    second; the FullCovHead fitted on the same data fails the thresholds.  It
    cannot pass without the head."""
    from multimodaltraj_2_amd.coupled import CoupledHead
    from multimodaltraj_2_amd.fullcov import FullCovHead
    S, F, N, K, B, seed = (PROP[k] for k in ("S", "F", "N", "K", "B", "seed"))
    pred_h = property_pred()
    pred = _t(pred_h, gpu)
    n_active = torch.full((S,), N, dtype=torch.int32, device=gpu)
    fit_tg, score_tg = (_t(property_targets(pred_h, w), gpu) for w in ("fit", "score"))
    co, fc = CoupledHead(device=gpu), FullCovHead(device=gpu)
    st = co.fit(pred, fit_tg, n_active)
    fc.fit(pred, fit_tg, n_active)
    share = float(np.trace(co.cpl[1].double().cpu().numpy() @ co.cpl[1].double().cpu().numpy().T)
                  / np.trace(co.marginal().chol.double().cpu().numpy() @ co.marginal().chol.double().cpu().numpy().T))
    print(f"device fit: share {share:.4f} (raw {st.share:.4f}), clipped {co.clipped}, pairs {st.pairs} in {st.groups}")
    assert abs(share - PROP["share"]) < 0.03 and co.clipped == 0 and st.pairs == S * F * N and st.groups == S * F
    # the marginals agree: the two heads differ in the dependence between pedestrians alone
    assert close(co.marginal().chol.cpu().numpy(), fc.chol.cpu().numpy()) <= 1e-2
    at = co.stats(pred, score_tg, n_active)
    print(f"on the scoring set: nll {at.nll:.4f}, independent {at.nll_independent:.4f}, gain {at.nll_gain:.4f}, "
          f"q_within {at.q_within_ratio:.4f}, q_between {at.q_between_ratio:.4f}")
    # out of sample a quadratic form under a covariance ESTIMATED from n draws of d = 24 dimensions has
    # mean d n / (n - d - 2), the inverse Wishart's: 960 / 934 = 1.03 for W (n = N - G) and 64 / 38 = 1.68
    # for B (n = G = 64 scene-frames), with 24 * 64 degrees of freedom behind the latter (sd 0.06)
    assert at.nll_gain > 1.0 and abs(at.q_within_ratio - 960 / 934) < 0.05
    assert abs(at.q_between_ratio - 64 / 38) < 0.35

    def score(kind):
        r = (co if kind == "coupled" else fc).couple_scores(pred, score_tg, n_active, K, B, seed=seed)
        assert r.couples == r.member_couples == S * F * N * (N - 1) // 2
        return {g: dict(dev=r.dev(g), crps=r.crps(g), pit_mean=r.pit_mean(g)) for g in cpr.FEATURES}
    property_check(score, "device: ")


def test_evaluation_end_to_end(gpu, tmp_path, data_root):
    """The recipe of tests/test_couple_scores_gpu.py::test_evaluation_end_to_end
    with --coupled_head eval --couple_scores 1 --collision_radius 0.1: every new
    figure logged after the other heads', all finite and equal to direct calls
    on ``keep``'s tensors; coupled_nll_gain has the sign of coupled_share > 0;
    with the flag off the keys and values of before."""
    from multimodaltraj_2_amd import checkpoint, evaluate
    from multimodaltraj_2_amd import train as tr
    from multimodaltraj_2_amd.argParser import ArgsParser
    argv = ["--data_root", data_root, "--leaveDataset", "2", "--n_max", "32", "--train_scenes", "64",
            "--train_batch", "32", "--num_epochs", "2", "--loss", "l2", "--num_samples", "20",
            "--mode", "train", "--save_dir", str(tmp_path), "--log_dir", str(tmp_path),
            "--device", "cuda:0"]
    args = ArgsParser().parser.parse_args(argv)
    assert args.coupled_head == "off"
    tr.run_train_mode(args, gpu, log=lambda s: None)
    prm = checkpoint.load_params(checkpoint.read_state(str(tmp_path)), device=gpu)
    args.couple_scores, args.collision_radius = 1, 0.1
    logs0 = []
    res0 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs0.append)
    assert not any(k.startswith("coupled_") for k in res0)
    args.coupled_head = "eval"
    logs1, keep = [], {}
    res1 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs1.append, keep=keep)
    new = list(evaluate.COUPLED_FIGURES) + list(evaluate.COUPLED_JOINT_FIGURES) + list(evaluate.COUPLED_CPL_FIGURES)
    assert list(res1) == list(res0) + new
    assert {k: res1[k] for k in res0} == res0 and logs1[:len(logs0)] == logs0 and len(logs1) == len(logs0) + 3
    assert logs1[-3].startswith("coupled head on dataset 2: closed-form fit on the left-out dataset itself")
    assert logs1[-2].startswith("coupled joint best-of-K on dataset 2:")
    assert logs1[-1].startswith("coupled couple scores of the 20 joint draws on dataset 2:")
    for k in new:
        print(f"evaluation {k}: {res1[k]:.8g}")
        assert np.isfinite(res1[k]), k
    assert (res1["coupled_nll_gain"] > 0) == (res1["coupled_share"] > 0)
    assert res1["coupled_clipped"] == keep["coupled"]["head"].clipped >= 0
    t = keep["plan"].to_device(gpu, F=1)
    one = torch.ones(keep["plan"].S, dtype=torch.int32, device=gpu)
    co = keep["coupled"]["head"]
    kw = dict(seed=args.sample_seed, n_frames=one, ped_mask=t["ped_mask"])
    direct = co.couple_scores(keep["pred"], t["targets"], t["n_active"], 20, **kw)
    for k, v in evaluate.couple_figures(direct, "coupled_").items():
        assert res1[k] == v or (np.isnan(res1[k]) and np.isnan(v)), k
    je = co.joint_eval(keep["pred"], t["targets"], t["n_active"], 20, 0.1, **kw)
    assert evaluate.coupled_joint_figures(je) == {k: res1[k] for k in evaluate.COUPLED_JOINT_FIGURES}
    assert res1["coupled_cpl_couples"] == res1["cpl_couples"] == je.ped_pairs
    st = co.stats(keep["pred"], t["targets"], t["n_active"], n_frames=one, ped_mask=t["ped_mask"])
    assert evaluate.coupled_figures(co, st) == {k: res1[k] for k in evaluate.COUPLED_FIGURES}
    # in-sample q_within is tr(A W_raw A^T) / 24 with A from the RIDGED W: 1 for a well-conditioned W, below
    # it by the share of W's directions that the ridge carries (these targets stand still, quirk Q11, and
    # the short-trained predictions hardly differ between steps: W is numerically rank-deficient)
    assert 0.0 < res1["coupled_q_within"] <= 1.0 + 1e-6
    # train: fitted on the fold's training scenes
    args.coupled_head, args.couple_scores, args.collision_radius = "train", 0, 0.0
    logs2 = []
    res2 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs2.append)
    assert list(res2)[-len(evaluate.COUPLED_FIGURES):] == list(evaluate.COUPLED_FIGURES)
    assert "scenes of the fold's training datasets" in logs2[-1]
    assert all(np.isfinite(res2[k]) for k in evaluate.COUPLED_FIGURES)
