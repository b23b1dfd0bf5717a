"""GPU: the head calibration (g2k_head_stats_f32, csrc/g2k_calib.hip;
GaussianHead.stats / fit; evaluate.py --fit_head / --calibration) against the
float64 checker tests/calib_ref.py.  PARITY UNPINNED: the reference has no
probabilistic head.  The kernel works in double on exact f32 differences, so
only the summation order differs from the checker: pairs exact, each moment
within 1e-11 of its sum of |term|, sum nll / sum q within 1e-9 max(1, |ref|),
the counts inside the checker's bracket at r2 (1 -+ 1e-9) (which has width 0
on these inputs), the fit within 1e-6 max(1, |ref|) (its f32 rounding).  The
shapes are the smallest that reach every path: one workgroup writing the
outputs itself, several workgroups and the rows kernel, a workgroup's range
that ends inside a scene-frame, Nmax 256, Nmax odd, shared targets, NULL mask
/ n_frames.  Measured on an MI355X: moments within 3.4·10⁻¹⁵ of their sum of
|term|, sum nll / sum q within 3.4·10⁻¹⁵, the fit within 6·10⁻⁸, every count
equal to the checker's.  Every column, frame and masked column that is not a pair holds NaN
in pred and targets: a finite output proves they were never read."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib
from tests.abi_arena import Arena, all_written
from tests.bestk_ref import pair_mask
from tests.calib_ref import head_stats_ref, levels_r2

pytestmark = pytest.mark.gpu
LEVELS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99)
NL = len(LEVELS)
ROW = (96 + 12 * NL) * 8                                  # bytes of one workgroup's row

#        S   F  Nmax n_active        n_frames   mask   shared
CASES = [(3, 2, 9, [0, 5, 9], [2, 1, 2], "one", False),
         (5, 3, 33, [33, 0, 17, 33, 1], [3, 3, 2, 0, 3], "rand", True),
         (2, 1, 256, [256, 130], None, None, False),
         (70, 2, 32, "rand", "rand", "rand", False),
         (61, 2, 9, "rand", "rand", "rand", False)]       # a workgroup's range ends inside a scene-frame
IDS = ["s3f2n9", "n33shared", "n256", "s70", "s61n9"]


@functools.lru_cache(maxsize=None)
def _inputs(i):
    S, F, N, nact, nfr, masked, shared = CASES[i]
    rng = np.random.default_rng(300 + i)
    if isinstance(nact, str):
        nact = rng.integers(0, N + 1, S)
    if isinstance(nfr, str):
        nfr = rng.integers(0, F + 1, S)
    nact = np.asarray(nact, np.int32)
    nfr = None if nfr is None else np.asarray(nfr, np.int32)
    pm = None
    if masked == "one":
        pm = np.ones((S, N), np.uint8)
        pm[:, 2] = 0
    elif masked == "rand":
        pm = (rng.random((S, N)) > 0.2).astype(np.uint8)
    pred = rng.standard_normal((S, F, 24, N)).astype(np.float32)
    Ft = 1 if shared else F
    base = pred[:, :Ft].reshape(S, Ft, 2, 12, N).transpose(0, 1, 4, 3, 2)
    e = rng.standard_normal((S, Ft, N, 12, 2))
    grow = (0.2 + 0.05 * np.arange(12))[None, None, None, :]
    res = np.stack([grow * e[..., 0], 0.5 * grow * (0.6 * e[..., 0] + 0.8 * e[..., 1])], -1)
    tg = np.ascontiguousarray((base + res).astype(np.float32))
    head = np.stack([np.log(0.4) + 0.2 * rng.standard_normal(12),
                     np.log(0.2) + 0.2 * rng.standard_normal(12),
                     0.5 * rng.standard_normal(12)]).astype(np.float32)
    m = pair_mask(S, F, N, nact, nfr, pm)                 # [S, F, N]
    np.transpose(pred, (0, 1, 3, 2))[~m] = np.nan         # a view: pred itself
    if shared:
        tg[:, 0][~m.any(axis=1)] = np.nan
    else:
        tg[~m] = np.nan
    return dict(pred=pred, targets=tg, head=head, n_active=nact, n_frames=nfr, ped_mask=pm,
                shared=shared, pairs=int(m.sum()))


@functools.lru_cache(maxsize=None)
def _reference(i, head="case"):
    c = _inputs(i)
    h = c["head"] if head == "case" else None
    return head_stats_ref(c["pred"], c["targets"], c["n_active"], head=h,
                          r2=levels_r2(LEVELS) if h is not None else (), n_frames=c["n_frames"],
                          ped_mask=c["ped_mask"])


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(i, dev, head="case", levels=LEVELS):
    from multimodaltraj_2_amd.nll import GaussianHead
    c = _inputs(i)
    gh = GaussianHead(device=dev)
    if head is not None:
        gh.head = _t(c["head"], dev) if isinstance(head, str) else head
    r = gh.stats(_t(c["pred"], dev), _t(c["targets"], dev), _t(c["n_active"], dev), levels,
                 n_frames=_t(c["n_frames"], dev), ped_mask=_t(c["ped_mask"], dev),
                 targets_shared=c["shared"], use_head=head is not None)
    torch.cuda.synchronize()
    return r


_CACHE = {}


def _gpu_result(i, dev):
    if i not in _CACHE:
        _CACHE[i] = _run(i, dev)
    return _CACHE[i]


def _ws_bytes(i, nl=NL):
    S, F, N = CASES[i][:3]
    d = _lib.G2KDims(S, F, 8, 12, 16, 64, N, 8, 0)
    return int(_lib.load().g2k_head_stats_workspace_bytes(ctypes.byref(d), nl))


def test_cases_cover_both_reductions():
    """By the kernel's own constants: the small cases are one workgroup (no
    workspace: it writes the outputs itself), s70 is several (rows kernel)."""
    assert [_ws_bytes(i) for i in range(3)] == [0, 0, 0]
    assert _ws_bytes(3) % ROW == 0 and _ws_bytes(3) // ROW >= 2
    S, F, N = CASES[4][:3]
    W = _ws_bytes(4) // ROW
    assert W >= 2 and -(-S * F * N // W) % N != 0         # slots per workgroup: no multiple of Nmax


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_values_match_checker(gpu, i):
    r = _gpu_result(i, gpu)
    R = _reference(i)
    st = r.stats.cpu().numpy()
    assert st.dtype == np.float64 and np.all(np.isfinite(st))
    np.testing.assert_array_equal(st[:, 0], np.full(12, _inputs(i)["pairs"], np.float64))
    assert r.pairs == R["pairs"] == _inputs(i)["pairs"] and r.pairs > 0
    for col in range(1, 6):
        err = np.abs(st[:, col] - R["stats"][:, col])
        print(f"case {IDS[i]} column {col}: max err / sum|term| {np.max(err / R['abs'][:, col]):.3g}")
        assert np.all(err <= 1e-11 * R["abs"][:, col]), col
    for col in (6, 7):
        err = np.abs(st[:, col] - R["stats"][:, col]) / np.maximum(1.0, np.abs(R["stats"][:, col]))
        print(f"case {IDS[i]} column {col}: max rel err {err.max():.3g}")
        assert np.all(err <= 1e-9), col
    # the counts: inside the checker's bracket, which is tight on these inputs
    r2 = levels_r2(LEVELS)
    lo = (R["q"][:, :, None] <= (r2 * (1 - 1e-9))[None, None]).sum(axis=0)
    hi = (R["q"][:, :, None] <= (r2 * (1 + 1e-9))[None, None]).sum(axis=0)
    assert np.array_equal(lo, hi), "no q may lie within 1e-9 of a level's radius"
    ins = r.inside.cpu().numpy()
    assert ins.dtype == np.int64 and ins.shape == (12, NL)
    assert np.all((lo <= ins) & (ins <= hi))
    np.testing.assert_array_equal(ins, R["inside"])
    fit = r.fit.cpu().numpy()
    assert fit.dtype == np.float32
    ferr = np.abs(fit - R["fit"]) / np.maximum(1.0, np.abs(R["fit"]))
    print(f"case {IDS[i]} fit: max rel err {ferr.max():.3g}")
    assert np.all(ferr <= 1e-6)


@pytest.mark.parametrize("i", [0, 3], ids=[IDS[0], IDS[3]])
def test_properties_are_the_definitions(gpu, i):
    r = _gpu_result(i, gpu)
    R = _reference(i)
    n = R["pairs"]
    assert abs(r.nll - R["stats"][:, 6].sum() / n) <= 1e-9 * max(1.0, abs(r.nll))
    np.testing.assert_allclose(r.nll_per_step, R["stats"][:, 6] / n, rtol=1e-9)
    np.testing.assert_array_equal(r.coverage, R["inside"] / n)
    np.testing.assert_array_equal(r.coverage_all, R["inside"].sum(axis=0) / (12 * n))
    assert r.ece == float(np.abs(r.coverage_all - np.asarray(LEVELS)).mean())
    assert abs(r.q_ratio - R["stats"][:, 7].sum() / (24 * n)) <= 1e-9
    np.testing.assert_allclose(r.bias, R["stats"][:, 1:3] / n, rtol=0, atol=1e-11)


@pytest.mark.parametrize("i", [0, 3], ids=[IDS[0], IDS[3]])
def test_agrees_with_the_nll_kernel(gpu, i):
    """sum_t nll_t == g2k_nll_f32's nll (the project's 1e-4 max(1, |ref|)),
    equal pair counts; at head = fit the NLL kernel's head gradient vanishes
    (|dhead| <= 1e-4 pairs) and q_ratio is 1 within 1e-5; with row 0 raised
    by 0.1 it does not (|dhead[0]| >= 0.05 pairs)."""
    from multimodaltraj_2_amd.nll import GaussianHead
    c = _inputs(i)
    r = _gpu_result(i, gpu)
    gh = GaussianHead(device=gpu)
    args = (_t(c["pred"], gpu), _t(c["targets"], gpu), _t(c["n_active"], gpu))
    kw = dict(n_frames=_t(c["n_frames"], gpu), ped_mask=_t(c["ped_mask"], gpu))
    gh.head = _t(c["head"], gpu)
    nll, pairs, _, _ = gh.nll(*args, **kw)
    tot = float(r.stats[:, 6].sum().item())
    print(f"case {IDS[i]}: sum nll {tot:.9g}, g2k_nll_f32 {float(nll):.9g}")
    assert int(pairs.item()) == r.pairs
    assert abs(float(nll) - tot) <= 1e-4 * max(1.0, abs(tot))
    gh.head = r.fit.clone()
    _, _, dhead, _ = gh.nll(*args, **kw)
    worst = float(dhead.abs().max().item())
    at_fit = _run(i, gpu, head=r.fit)
    print(f"case {IDS[i]}: max |dhead| at the fit {worst:.3g} ({r.pairs} pairs), q_ratio {at_fit.q_ratio:.9g}")
    assert worst <= 1e-4 * r.pairs
    assert abs(at_fit.q_ratio - 1.0) <= 1e-5
    gh.head = r.fit.clone()
    gh.head[0] += 0.1
    _, _, dhead, _ = gh.nll(*args, **kw)
    assert bool((dhead[0].abs() >= 0.05 * r.pairs).all())


def test_fit_sets_the_head(gpu):
    from multimodaltraj_2_amd.nll import GaussianHead
    c = _inputs(0)
    gh = GaussianHead(device=gpu)
    hs = gh.fit(_t(c["pred"], gpu), _t(c["targets"], gpu), _t(c["n_active"], gpu),
                n_frames=_t(c["n_frames"], gpu), ped_mask=_t(c["ped_mask"], gpu))
    assert gh.head is hs.fit and torch.equal(hs.fit, _gpu_result(0, gpu).fit)
    assert hs.nll is None and hs.coverage is None and hs.q_ratio is None and hs.inside is None
    assert bool((hs.stats[:, 6:] == 0).all())
    with pytest.raises(ValueError, match="no .* pair"):
        gh.fit(_t(c["pred"], gpu), _t(c["targets"], gpu), torch.zeros(3, dtype=torch.int32, device=gpu))


def _raw(dev, c, S, F, N, head, nl, ar):
    """The raw ABI call into guarded, poisoned outputs: float64 / int64 are
    float32 / int32 payloads of twice the length, viewed."""
    lib = _lib.load()
    d = _lib.G2KDims(S, F, 8, 12, 16, 64, N, 8, _lib.STEP_TARGETS_SHARED if c["shared"] else 0)
    stats32 = ar.alloc(2 * 96, torch.float32, "stats")
    inside32 = ar.alloc(2 * 12 * nl, torch.int32, "inside") if nl else None
    fit = ar.alloc((3, 12), torch.float32, "fit")
    need = int(lib.g2k_head_stats_workspace_bytes(ctypes.byref(d), nl))
    ws = ar.alloc(max(need, 8), torch.uint8, "workspace")
    keep = [_t(c[k], dev) for k in ("pred", "targets", "n_active", "n_frames", "ped_mask")]
    r2 = _t(levels_r2(LEVELS[:nl]), dev) if nl else None
    p = lambda t: None if t is None else t.data_ptr()
    rc = lib.g2k_head_stats_f32(ctypes.byref(d), *(p(t) for t in keep), p(head), p(r2), nl,
                                p(stats32), p(inside32), p(fit), p(ws), need, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.g2k_last_error()
    ar.check_guards()
    return stats32, inside32, fit


@pytest.mark.parametrize("i", [0, 3], ids=[IDS[0], IDS[3]])
def test_write_footprint(gpu, i):
    c = _inputs(i)
    S, F, N = CASES[i][:3]
    ar = Arena(gpu)
    stats32, inside32, fit = _raw(gpu, c, S, F, N, _t(c["head"], gpu), NL, ar)
    assert all_written(stats32) and all_written(inside32) and all_written(fit)
    r = _gpu_result(i, gpu)
    assert torch.equal(stats32.view(torch.float64).view(12, 8), r.stats)
    assert torch.equal(inside32.view(torch.int64).view(12, NL), r.inside)
    assert torch.equal(fit, r.fit)
    # without a head: columns 6, 7 exactly 0, the rest the same bits
    stats32, _, fit = _raw(gpu, c, S, F, N, None, 0, Arena(gpu))
    st = stats32.view(torch.float64).view(12, 8)
    assert all_written(stats32) and all_written(fit)
    assert bool((st[:, 6:] == 0).all()) and torch.equal(st[:, :6], r.stats[:, :6])
    assert torch.equal(fit, r.fit)


def test_no_pair_writes_zeros(gpu):
    c = dict(_inputs(0))
    c.update(pred=c["pred"][:1], targets=c["targets"][:1], n_active=np.zeros(1, np.int32),
             n_frames=c["n_frames"][:1], ped_mask=c["ped_mask"][:1])
    ar = Arena(gpu)
    stats32, inside32, fit = _raw(gpu, c, 1, 2, 9, _t(c["head"], gpu), NL, ar)
    assert all_written(stats32) and all_written(inside32) and all_written(fit)
    for t in (stats32, inside32, fit):
        assert bool((t.view(torch.int32) == 0).all())


@pytest.mark.parametrize("i", [1, 3], ids=[IDS[1], IDS[3]])
def test_repeated_calls_are_bit_identical(gpu, i):
    a, b = _gpu_result(i, gpu), _run(i, gpu)
    assert torch.equal(a.stats.view(torch.int64), b.stats.view(torch.int64))
    assert torch.equal(a.inside, b.inside) and torch.equal(a.fit, b.fit)


def test_evaluation_end_to_end(gpu, tmp_path, data_root):
    """A two-epoch --mode train --loss l2 checkpoint has no head.  Both flags
    off: the two log lines and the seven keys of before.  --fit_head train:
    the head used is GaussianHead.fit on the fold's plan, the CLI's
    CALIB_FIGURES are those of a direct stats call, and minADE_K moves."""
    from multimodaltraj_2_amd import checkpoint, evaluate
    from multimodaltraj_2_amd import train as tr
    from multimodaltraj_2_amd.argParser import ArgsParser
    from multimodaltraj_2_amd.nll import GaussianHead
    argv = ["--data_root", data_root, "--leaveDataset", "2", "--n_max", "32", "--train_scenes", "64",
            "--train_batch", "32", "--num_epochs", "2", "--loss", "l2", "--num_samples", "4",
            "--mode", "train", "--save_dir", str(tmp_path), "--log_dir", str(tmp_path),
            "--device", "cuda:0"]
    args = ArgsParser().parser.parse_args(argv)
    tr.run_train_mode(args, gpu, log=lambda s: None)
    prm = checkpoint.load_params(checkpoint.read_state(str(tmp_path)), device=gpu)
    assert prm.head is None

    # both flags off: exactly the lines and keys of the best-of-K evaluation
    logs, keep = [], {}
    res = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs.append, keep=keep)
    assert list(res) == ["scenes", "pairs", "K", "ade", "fde", "min_ade", "min_fde"]
    assert sorted(keep) == ["head", "joint", "n_frames", "out", "plan", "pred"]
    t = keep["plan"].to_device(gpu, F=1)
    one = torch.ones(keep["plan"].S, dtype=torch.int32, device=gpu)
    bk = GaussianHead(log_sigma=0.0, device=gpu).best_of_k(
        keep["pred"], t["targets"], t["n_active"], 4, seed=0, n_frames=one, ped_mask=t["ped_mask"],
        want_per_ped=False)
    assert res == dict(scenes=keep["plan"].S, pairs=bk.pairs, K=4, ade=bk.ade, fde=bk.fde,
                       min_ade=bk.min_ade, min_fde=bk.min_fde)
    assert logs == ["best-of-K: no head in the parameters, constant log sigma 0.0",
                    f"best-of-4 on dataset 2: {res['scenes']} scenes, {res['pairs']} pairs, "
                    f"ADE {res['ade']:.6g} FDE {res['fde']:.6g} minADE_4 {res['min_ade']:.6g} "
                    f"minFDE_4 {res['min_fde']:.6g}"]

    # --fit_head train
    args.fit_head = "train"
    logs1, keep1 = [], {}
    res1 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs1.append, keep=keep1)
    fplan = evaluate.fold_plan(args, prm.nmax)
    assert fplan.S == 64
    ft, fout, fone = evaluate._fused_step(args, prm, fplan, gpu)
    gh = GaussianHead(device=gpu)
    hs = gh.fit(fout.pred, ft["targets"], ft["n_active"], n_frames=fone, ped_mask=ft["ped_mask"])
    assert torch.equal(keep1["head"], gh.head) and keep1["fitted"].pairs == hs.pairs > 0
    direct = evaluate.calib_figures(gh.stats(keep1["pred"], t["targets"], t["n_active"],
                                             evaluate.CALIB_LEVELS, n_frames=one,
                                             ped_mask=t["ped_mask"]))
    assert tuple(direct) == evaluate.CALIB_FIGURES
    cli = evaluate.main(argv + ["--fit_head", "train"], log=lambda s: None)
    for k in evaluate.CALIB_FIGURES:
        print(f"evaluation {k}: {cli[k]:.8g}")
        assert np.isfinite(cli[k]) and cli[k] == direct[k] == res1[k], k
    assert res1["ade"] == res["ade"] and res1["min_ade"] != res["min_ade"]
    assert len([s for s in logs1 if s.startswith("calibration on dataset 2")]) == 1
    assert any("closed-form fit on 64 scenes" in s for s in logs1)
    # --calibration 1 alone: the constant head's figures, the best-of-K ones unchanged
    args.fit_head, args.calibration = "off", 1
    res2 = evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
    assert {k: res2[k] for k in res} == res and set(res2) == set(res) | set(evaluate.CALIB_FIGURES)
    # --fit_head eval: in-sample, so its NLL is not above any other head's
    args.fit_head = "eval"
    logs3 = []
    res3 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs3.append)
    assert any("in-sample" in s for s in logs3)
    assert res3["nll"] <= res1["nll"] + 1e-9 and res3["nll"] <= res2["nll"] + 1e-9
    assert abs(res3["q_ratio"] - 1.0) <= 1e-5
