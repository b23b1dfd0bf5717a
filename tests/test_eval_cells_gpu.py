"""GPU: every cell of tests/eval_cells.py against the float64 checkers
(tests/bestk_ref.py, fullcov_ref.py, calib_ref.py, joint_ref.py,
fullcov_joint_ref.py), never against a sibling GPU path alone, through the raw
C ABI into guarded, poisoned outputs (tests/abi_arena.py).  PARITY UNPINNED: the
reference has no probabilistic head.  tests/test_eval_cells.py proves on the CPU
that each cell reaches the geometry it claims; the train cells run in
tests/test_train_gpu.py and tests/test_ops_domain_gpu.py, the KDE pair takes
"ks32-fill" through tests/kde_cases.py.

Which branch each cell reaches, and why its shape is the smallest that does:

per-pair (best_of_k_kernel<Head>, both heads, with and without `best`)
  ks8        (2, 2, 9, K 9): KS doubles while 2 KS <= K, so K 9 is the first
             K with 8 lanes and one that is no multiple of them (lane 0 draws
             twice); Nmax 9 x KS 8 leaves FC 2 = F, one workgroup per scene.
  ks32-fill  (33, 2, 256, K 64): KS stops at the first value with S F Nmax KS
             >= 2^19.  At Nmax 256 (the widest) and F 2 (the fewest frames
             with C > 1) that is 32 from S 33 on (S 32: 2^19 / 32 = 16384 =
             32 x 2 x 256 slots, still 64).  S 33 is also the first S with
             S 8 > 256: g2k_bestk_rows_kernel's second workgroup.  One scene at
             256, one empty, the rest <= 6: the items loop's trip count is 32
             in one workgroup and 0 or 1 in its neighbours.
  ks64       (1, 1, 16, K 64 and K 130), n_active 2: the cap of 64 lanes needs
             K >= 64; one pair per wave, two pairs in all.  K 64 gives every
             lane one draw, K 130 lanes 0, 1 three and the rest two.
stats (g2k_head_stats_f32 / g2k_fullcov_stats_f32, with head and levels, and
without: moments and fit only), Nmax 256 and F 2 so that S alone sets W = S:
  w17   W 17: the first W at which thread j = 1 of g2k_head_stats_rows_kernel
        has a row (slice 16) and g2k_fullcov_rows_kernel takes a second trip.
  w33   W 33: the first W with a second trip (r0 += 32) of the former; the
        third of the latter.
  cap   (17, 32, 256): 272 x 512 slots, W capped at 256, U 544: the first S at
        F 32 past the cap; 544 % 256 = 32, ranges end inside a scene-frame.
joint (both heads, radius 0.3)
  kd1-waves  (8, 65, 65, K 3): Nmax 65 is the first width on joint_kernel
             (four waves), S F = 520 the first multiple of F 65 with ceil(512 /
             S F) = 1; F 65 is the first F at which a lane of
             g2k_joint_rows_kernel (lane 0) adds two frames.
  kd1-wave   (64, 32, 4, K 5): S F = 2048 is the first with KD 1 at Nmax <= 64;
             P <= 4: groups of 16 lanes, seven items on four groups, two passes.

Tolerances and comparison forms, the project's, unchanged: close() <= 1e-4 for
the sampled figures; indices by "the checker's error at the kernel's index
attains the checker's minimum" (1e-4); counts exact; stats moments within
1e-11 of their sum of |term|, sum nll / sum q within 1e-9 max(1, |ref|), counts
inside the checker's bracket at r2 (1 -+ 1e-9) and equal to the checker's, fit
1e-6 (tests/test_head_stats_gpu.py); full-covariance moments and stats 1e-12
max(1, |ref|), counts equal, |fit fit^T - C| <= 1e-4 max|C| and the factor 1e-4
(tests/test_fullcov_gpu.py); joint collision counts of the per-step head inside
the checker's bracket at radius -+ 1e-4, of the full-covariance head inside the
float64 recount of the device's own draws at radius (1 -+ 1e-6), after the caps
(ambiguous couple-draws <= 1e-3 of all and <= 1 % of the collisions) have been
asserted on the checker, and on the recount, alone.  Footprint: guards intact,
every element written, exact zeros for non-pairs, best == pred off the pairs.
Each test prints its worst error as a ratio of its bound before it asserts.

MEASURED on an MI355X, worst error / bound (each test prints its figures
before it asserts); no cell came within 2 x of a bound:
  per-pair, per_ped / sums / draw kA's ADE, per-step head | full covariance;
  every index attains the checker's minimum exactly (0), with and without
  `best` the same bits:
    ks8        0.0035 / 0.0012 / 0.0003  |  0.0052 / 0.0035 / 0.0011
    ks32-fill  0.0029 / 0.0044 / 0.0006  |  0.017  / 0.0089 / 0.0017   (566 pairs)
    ks64       0.0011 / 0.0014 / 0.0002  |  0.0013 / 0.0015 / 0.0004
    ks64-k130  0.0005 / 0.0008 / 0.0002  |  0.0006 / 0.0007 / 0.0004
  stats, per-step head: worst moment / sum nll, sum q / fit; full covariance:
  moments / stats / fit fit^T / factor; every count equal to the checker's:
    w17  (1373 pairs)   0.00033 / 2.0e-6 / 0.053  |  0.00049 / 0.00044 / 0.00056 / 3.2e-5
    w33  (3796 pairs)   0.00079 / 5.0e-6 / 0.040  |  0.00077 / 0.00032 / 0.00056 / 3.3e-5
    cap  (39596 pairs)  0.015   / 1.3e-5 / 0.054  |  0.0013  / 0.00066 / 0.00037 / 3.0e-5
  joint, per_frame / sums, indices 0:
    kd1-waves  per-step 0.0040 / 0.0009, sum col_k 139550 in [139477, 139641]
               (checker: 635664 couple-draws, 139550 collisions, 164 ambiguous);
               full covariance 0.0044 / 0.0009, sampler 0.019, JADE from the
               device's draws 0.0008, sum col_k 144952 in [144952, 144952]
    kd1-wave   per-step 0.0028 / 0.0018, sum col_k 4489 in [4489, 4492] (20800
               couple-draws, 3 ambiguous); full covariance 0.0057 / 0.0019,
               sampler 0.0057, sum col_k 4795 in [4795, 4795]
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib
from tests import eval_cells as ec
from tests import fullcov_joint_ref as fj
from tests import fullcov_ref as fr
from tests.abi_arena import Arena, all_written
from tests.bestk_ref import MASK64, best_of_k_ref, draw_errors
from tests.calib_ref import head_stats_ref, levels_r2
from tests.conftest import close
from tests.joint_ref import joint_eval_ref

pytestmark = pytest.mark.gpu
TOL = 1e-4
REL = 1e-6                                                 # the recount's bracket: radius (1 -/+ REL)
HEADS = ("per_step", "fullcov")
NL = len(ec.LEVELS)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _p(t):
    return None if t is None else t.data_ptr()


def _dims(c):
    return _lib.G2KDims(c.S, c.F, 8, 12, 16, 64, c.Nmax, 8, 0)


def _keep(x, dev, head):
    """The six input pointers' tensors, in the ABI's order."""
    return [_t(x[k], dev) for k in ("pred", "targets", "n_active", "n_frames", "ped_mask", head)]


def report(label, ratios):
    worst = max(ratios, key=ratios.get)
    print(f"{label}: worst error / bound = {ratios[worst]:.3g} ({worst}); "
          + ", ".join(f"{k} {v:.2g}" for k, v in sorted(ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, bad


# ---------------------------------------------------------------------------
# per-pair family
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair_inputs(cid):
    return ec.pair_inputs(next(c for c in ec.PER_PAIR if c.id == cid))


@functools.lru_cache(maxsize=None)
def _pair_reference(cid, which):
    x = _pair_inputs(cid)
    fn, head = (best_of_k_ref, x["head"]) if which == "per_step" else (fr.best_of_k_ref, x["chol"])
    return fn(x["pred"], x["targets"], x["n_active"], head, x["seed"], x["K"], x["n_frames"],
              x["ped_mask"])


def _pair_raw(c, which, dev, want_best):
    lib = _lib.load()
    x = _pair_inputs(c.id)
    d = _dims(c)
    fn = "g2k_best_of_k_f32" if which == "per_step" else "g2k_fullcov_best_of_k_f32"
    ar = Arena(dev)
    per = ar.alloc((c.S, c.F, c.Nmax, 4), name="per_ped")
    best = ar.alloc((c.S, c.F, 24, c.Nmax), name="best") if want_best else None
    out = ar.alloc((c.S, 8), name="out")
    need = int(getattr(lib, fn.replace("_f32", "_workspace_bytes"))(ctypes.byref(d)))
    ws = ar.alloc(need, torch.uint8, "workspace")
    keep = _keep(x, dev, "head" if which == "per_step" else "chol")
    rc = getattr(lib, fn)(ctypes.byref(d), *(_p(t) for t in keep), ctypes.c_uint64(x["seed"]), c.K,
                          _p(per), _p(best), _p(out), _p(ws), need, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.g2k_last_error()
    ar.check_guards()
    assert all_written(per) and all_written(out) and (best is None or all_written(best))
    return per, best, out, keep[0]


@pytest.mark.parametrize("which", HEADS)
@pytest.mark.parametrize("cell", ec.PER_PAIR, ids=lambda c: c.id)
def test_per_pair_cell_matches_checker(gpu, cell, which):
    x, R = _pair_inputs(cell.id), _pair_reference(cell.id, which)
    m = R["pairs"]
    assert int(m.sum()) > 0
    ratios = {}
    first = None
    for want_best in (True, False):
        per_t, best_t, out_t, pred_t = _pair_raw(cell, which, gpu, want_best)
        per, out = per_t.cpu().numpy(), out_t.cpu().numpy()
        assert np.all(np.isfinite(per)) and np.all(np.isfinite(out))   # NaN above the diagonal: not read
        tag = "best" if want_best else "nobest"
        ratios[f"per_ped-{tag}"] = close(per[..., :2], R["per_ped"][..., :2]) / TOL
        ratios[f"sums-{tag}"] = close(out[:, :5], R["out"][:, :5]) / TOL
        np.testing.assert_array_equal(out[:, 2], R["out"][:, 2])       # pairs, exact
        np.testing.assert_array_equal(out[:, 5], R["out"][:, 5])       # K
        assert np.all(out[:, 6:].view(np.int32) == 0)
        assert np.all(per[~m].view(np.int32) == 0)                     # non-pairs: exactly zero, all four
        per64 = per.astype(np.float64)
        for col, errs in ((2, R["ade_k"]), (3, R["fde_k"])):
            k = per64[..., col][m]
            assert np.all(k == np.round(k)) and np.all((k >= 0) & (k < cell.K))
            at = np.take_along_axis(errs, per64[..., col].astype(np.int64)[None], axis=0)[0][m]
            lo = errs.min(axis=0)[m]
            ratios[f"index{col}-{tag}"] = float((np.abs(at - lo) / np.maximum(1.0, np.abs(lo))).max()) / TOL
        if want_best:
            first = (per_t, out_t)
            off = ~torch.from_numpy(m).to(gpu)[:, :, None, :].expand_as(pred_t)
            assert torch.equal(best_t[off], pred_t[off])               # pred off the pairs
            # draw kA itself: its ADE against the targets is the checker's minimum
            ade, _ = draw_errors(best_t.cpu().numpy().astype(np.float64), x["targets"])
            ratios["best-ade"] = close(ade[m], R["per_ped"][..., 0][m]) / TOL
            assert not torch.equal(best_t, pred_t)
        else:                                                          # `best` changes no other output
            assert torch.equal(per_t, first[0]) and torch.equal(out_t, first[1])
    report(f"{cell.id} {which} ({int(m.sum())} pairs)", ratios)


# ---------------------------------------------------------------------------
# stats family
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stats_inputs(cid):
    return ec.stats_inputs(next(c for c in ec.STATS if c.id == cid))


@functools.lru_cache(maxsize=None)
def _stats_reference(cid, which):
    x = _stats_inputs(cid)
    a = (x["pred"], x["targets"], x["n_active"])
    kw = dict(n_frames=x["n_frames"], ped_mask=x["ped_mask"])
    if which == "per_step":
        return head_stats_ref(*a, head=x["head"], r2=levels_r2(ec.LEVELS), **kw)
    return fr.stats_ref(*a, chol=x["chol"], r2=fr.levels_r2(ec.LEVELS), **kw)


def _stats_raw(c, which, dev, with_head):
    """float64 / int64 outputs are float32 / int32 payloads of twice the
    length, viewed.  -> dict of tensors."""
    lib = _lib.load()
    x = _stats_inputs(c.id)
    d = _dims(c)
    nl = NL if with_head else 0
    ar = Arena(dev)
    o = {}
    if which == "per_step":
        fn, hk, r2 = "g2k_head_stats_f32", "head", levels_r2(ec.LEVELS)
        o["stats"] = ar.alloc(2 * 96, torch.float32, "stats")
        shapes = dict(stats=(12, 8), inside=(12, NL))
        o["fit"] = ar.alloc((3, 12), torch.float32, "fit")
    else:
        fn, hk, r2 = "g2k_fullcov_stats_f32", "chol", fr.levels_r2(ec.LEVELS)
        o["moments"] = ar.alloc(2 * 25 * 24, torch.float32, "moments")
        o["stats"] = ar.alloc(2 * 12 * 4, torch.float32, "stats")
        shapes = dict(moments=(25, 24), stats=(12, 4), inside=(13, NL))
        o["fit"] = ar.alloc((24, 24), torch.float32, "fit")
    if nl:
        o["inside"] = ar.alloc(2 * int(np.prod(shapes["inside"])), torch.int32, "inside")
    need = int(getattr(lib, fn.replace("_f32", "_workspace_bytes"))(ctypes.byref(d), nl))
    assert need > 0                                                     # several workgroups: the rows kernel
    ws = ar.alloc(need, torch.uint8, "workspace")
    keep = _keep(x, dev, hk)
    if not with_head:
        keep[5] = None
    r2t = _t(r2, dev) if nl else None
    outs = [o[k] for k in (("moments", "stats") if which == "fullcov" else ("stats",))]
    rc = getattr(lib, fn)(ctypes.byref(d), *(_p(t) for t in keep), _p(r2t), nl, *(_p(t) for t in outs),
                          _p(o.get("inside")), _p(o["fit"]), _p(ws), need, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.g2k_last_error()
    ar.check_guards()
    for k, t in o.items():
        assert all_written(t), k
    res = dict(fit=o["fit"].cpu().numpy())
    for k in ("moments", "stats"):
        if k in o:
            res[k] = o[k].view(torch.float64).view(shapes[k]).cpu().numpy()
    if nl:
        res["inside"] = o["inside"].view(torch.int64).view(shapes["inside"]).cpu().numpy()
    return res


def _check_head_stats(x, R, got, with_head, ratios):
    st = got["stats"]
    assert np.all(np.isfinite(st))
    np.testing.assert_array_equal(st[:, 0], np.full(12, x["pairs"], np.float64))
    assert R["pairs"] == x["pairs"]
    for col in range(1, 6):
        err = np.abs(st[:, col] - R["stats"][:, col])
        ratios[f"moment{col}"] = float(np.max(err / (1e-11 * R["abs"][:, col])))
    fit = got["fit"]
    assert fit.dtype == np.float32
    ratios["fit"] = float((np.abs(fit - R["fit"]) / np.maximum(1.0, np.abs(R["fit"]))).max()) / 1e-6
    if not with_head:
        assert np.all(st[:, 6:].view(np.int64) == 0)                    # columns 6, 7 exactly 0
        return
    for col in (6, 7):
        err = np.abs(st[:, col] - R["stats"][:, col]) / np.maximum(1.0, np.abs(R["stats"][:, col]))
        ratios[f"column{col}"] = float(err.max()) / 1e-9
    r2 = levels_r2(ec.LEVELS)
    lo = (R["q"][:, :, None] <= (r2 * (1 - 1e-9))[None, None]).sum(axis=0)
    hi = (R["q"][:, :, None] <= (r2 * (1 + 1e-9))[None, None]).sum(axis=0)
    assert np.array_equal(lo, hi), "no q may lie within 1e-9 of a level's radius"
    ins = got["inside"]
    assert np.all((lo <= ins) & (ins <= hi))
    np.testing.assert_array_equal(ins, R["inside"])


def _check_fullcov_stats(x, R, got, with_head, ratios):
    mo, st, fit = got["moments"], got["stats"], got["fit"]
    n = x["pairs"]
    assert np.all(np.isfinite(mo)) and np.all(np.isfinite(st)) and R["pairs"] == n
    np.testing.assert_array_equal(st[:, 0], np.full(12, n, np.float64))
    np.testing.assert_array_equal(mo[:24], mo[:24].T)
    ratios["moments"] = float(np.max(np.abs(mo - R["moments"]) / np.maximum(1.0, np.abs(R["moments"])))) / 1e-12
    assert np.all(fit[np.triu_indices(24, 1)] == 0) and np.all(np.diag(fit) > 0)
    f64 = fit.astype(np.float64)
    ratios["fit-llt"] = float(np.abs(f64 @ f64.T - R["C"]).max() / np.abs(R["C"]).max()) / 1e-4
    assert n >= 200 and np.linalg.cond(R["C"]) <= 1e3                  # well conditioned: the factor itself
    ratios["fit"] = close(fit, R["fit"]) / TOL
    if not with_head:
        assert np.all(st[:, 1:].view(np.int64) == 0)
        return
    assert np.all(st[:, 3] == 0)
    ratios["stats"] = float(np.max(np.abs(st - R["stats"]) / np.maximum(1.0, np.abs(R["stats"])))) / 1e-12
    r2 = fr.levels_r2(ec.LEVELS)
    qs = np.concatenate([R["q_t"], R["q"][:, None]], axis=1)           # [P, 13]
    rad = np.concatenate([np.repeat(r2[:1], 12, axis=0), r2[1:]], axis=0)
    lo = (qs[:, :, None] <= (rad * (1 - 1e-9))[None]).sum(axis=0)
    hi = (qs[:, :, None] <= (rad * (1 + 1e-9))[None]).sum(axis=0)
    assert np.array_equal(lo, hi), "no q may lie within 1e-9 of a level's radius"
    np.testing.assert_array_equal(got["inside"], R["inside"])


@pytest.mark.parametrize("with_head", [True, False], ids=["head", "nohead"])
@pytest.mark.parametrize("which", HEADS)
@pytest.mark.parametrize("cell", ec.STATS, ids=lambda c: c.id)
def test_stats_cell_matches_checker(gpu, cell, which, with_head):
    x, R = _stats_inputs(cell.id), _stats_reference(cell.id, which)
    got = _stats_raw(cell, which, gpu, with_head)
    ratios = {}
    (_check_head_stats if which == "per_step" else _check_fullcov_stats)(x, R, got, with_head, ratios)
    report(f"{cell.id} {which} {'with' if with_head else 'without'} head ({x['pairs']} pairs)", ratios)


# ---------------------------------------------------------------------------
# joint family
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _joint_inputs(cid):
    return ec.joint_inputs(next(c for c in ec.JOINT if c.id == cid))


def assert_cap(amb, couple_draws, collisions, label):
    """The ambiguous couple-draws are at most 1e-3 of all couple-draws and at
    most 1 % of the collisions: the bracket cannot hide a miscount."""
    print(f"{label}: {couple_draws} couple-draws, {collisions} collisions, {amb} ambiguous")
    assert amb <= 1e-3 * couple_draws and amb <= 0.01 * collisions


@functools.lru_cache(maxsize=None)
def _joint_reference(cid, which):
    x = _joint_inputs(cid)
    fn, head = (joint_eval_ref, x["head"]) if which == "per_step" else (fj.joint_eval_ref, x["chol"])
    R = fn(x["pred"], x["targets"], x["n_active"], head, x["seed"], x["K"], ec.RADIUS, x["n_frames"],
           x["ped_mask"])
    assert_cap(int(R["amb_k"].sum()), x["K"] * int(R["per_frame_i"][..., 1].sum()), int(R["col_k"].sum()),
               f"checker, {cid} {which}")
    return R


def _joint_raw(c, which, dev):
    lib = _lib.load()
    x = _joint_inputs(c.id)
    d = _dims(c)
    fn = "g2k_joint_eval_f32" if which == "per_step" else "g2k_fullcov_joint_eval_f32"
    ar = Arena(dev)
    pf = ar.alloc((c.S, c.F, 4), name="per_frame_f")
    pi = ar.alloc((c.S, c.F, 6), torch.int32, "per_frame_i")
    sf = ar.alloc((c.S, 4), name="sums_f")
    si32 = ar.alloc(2 * c.S * 6, torch.int32, "sums_i")
    need = int(getattr(lib, fn.replace("_f32", "_workspace_bytes"))(ctypes.byref(d)))
    ws = ar.alloc(need, torch.uint8, "workspace")
    keep = _keep(x, dev, "head" if which == "per_step" else "chol")
    rc = getattr(lib, fn)(ctypes.byref(d), *(_p(t) for t in keep), ctypes.c_uint64(x["seed"]), c.K,
                          ctypes.c_float(ec.RADIUS), _p(pf), _p(pi), _p(sf), _p(si32), _p(ws), need, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.g2k_last_error()
    ar.check_guards()
    for t in (pf, pi, sf, si32):
        assert all_written(t)
    return (pf.cpu().numpy().astype(np.float64), pi.cpu().numpy().astype(np.int64),
            sf.cpu().numpy().astype(np.float64), si32.view(torch.int64).view(c.S, 6).cpu().numpy())


def _between(lo, x, hi):
    return bool(np.all(lo <= x) and np.all(x <= hi))


@pytest.mark.parametrize("which", HEADS)
@pytest.mark.parametrize("cell", ec.JOINT, ids=lambda c: c.id)
def test_joint_cell_matches_checker(gpu, cell, which):
    x, R = _joint_inputs(cell.id), _joint_reference(cell.id, which)
    pf, pi, sf, si = _joint_raw(cell, which, gpu)
    K = cell.K
    ratios = dict(per_frame=close(pf[..., :2], R["per_frame_f"][..., :2]) / TOL,
                  sums=close(sf[:, :2], R["sums_f"][:, :2]) / TOL)
    assert np.all(sf[:, 2] == K) and np.all(sf[:, 3] == 0)
    np.testing.assert_array_equal(pi[..., :2], R["per_frame_i"][..., :2])          # P, PP
    np.testing.assert_array_equal(si[:, :2], R["sums_i"][:, :2])
    off = R["per_frame_i"][..., 0] == 0                     # no member: exactly zero, every column
    on = ~off
    assert off.any() and np.all(pf[off] == 0) and np.all(pi[off] == 0)
    np.testing.assert_array_equal(si, pi.sum(axis=1))       # the scene sums are the frames'
    for col, errs in ((2, R["jade_k"]), (3, R["jfde_k"])):
        k = pf[..., col][on]
        assert np.all(k == np.round(k)) and np.all((k >= 0) & (k < K))
        at = np.take_along_axis(errs, pf[..., col].astype(np.int64)[None], axis=0)[0][on]
        best = errs.min(axis=0)[on]
        ratios[f"index{col}"] = float((np.abs(at - best) / np.maximum(1.0, np.abs(best))).max()) / TOL
    kJA = pf[..., 2].astype(np.int64)                       # the KERNEL's index
    # the head-independent columns (the mean's and the targets' collisions): the checker's bracket
    for col, lo, hi in ((2, R["pred_lo"], R["pred_hi"]), (3, R["gt_lo"], R["gt_hi"])):
        assert _between(lo, pi[..., col], hi), col
        assert _between(lo.sum(axis=1), si[:, col], hi.sum(axis=1)), col
    if which == "per_step":
        lo_k, hi_k = R["col_lo"], R["col_hi"]
    else:
        # the device's own draws (the sampler's, bit for bit) recounted in float64
        from multimodaltraj_2_amd.fullcov import FullCovHead
        fc = FullCovHead(device=gpu)
        fc.chol = _t(x["chol"], gpu)
        pred = _t(x["pred"], gpu)
        xs = np.stack([fc.sample(pred, seed=(x["seed"] + k) & MASK64).cpu().numpy() for k in range(K)])
        ratios["sampler"] = close(xs[K - 1], fr.sample(x["pred"], x["chol"], (x["seed"] + K - 1) & MASK64)) / TOL
        lo_k, hi_k, amb = fj.recount(xs, R["members"], ec.RADIUS, REL)
        assert_cap(int(amb.sum()), K * int(pi[..., 1].sum()), int(lo_k.sum()),
                   f"device draws, {cell.id}")
        Pd = np.maximum(R["members"].sum(axis=2), 1)
        jade = np.stack([(draw_errors(xs[k].astype(np.float64), x["targets"])[0] * R["members"]).sum(axis=2) / Pd
                         for k in range(K)])
        ratios["jade-recount"] = close(pf[..., 0], jade.min(axis=0) * on) / TOL
    print(f"{cell.id} {which}: col_pred {pi[..., 2].sum()}, col_gt {pi[..., 3].sum()}, sum col_k "
          f"{pi[..., 4].sum()} in [{lo_k.sum()}, {hi_k.sum()}], col_best {pi[..., 5].sum()}")
    assert _between(lo_k.sum(axis=0), pi[..., 4], hi_k.sum(axis=0))                # per scene-frame
    assert _between(lo_k.sum(axis=(0, 2)), si[:, 4], hi_k.sum(axis=(0, 2)))        # per scene
    blo = np.take_along_axis(lo_k, kJA[None], axis=0)[0]
    bhi = np.take_along_axis(hi_k, kJA[None], axis=0)[0]
    assert _between(blo[on], pi[..., 5][on], bhi[on])
    assert _between((blo * on).sum(axis=1), si[:, 5], (bhi * on).sum(axis=1))
    assert pi[..., 4].sum() > 0                             # there is something to count
    report(f"{cell.id} {which} ({int(R['per_frame_i'][..., 0].sum())} members)", ratios)
