"""GPU: the fused rank-histogram calibration (g2k_sample_ranks_f32,
g2k_fullcov_sample_ranks_f32, g2k_mix_sample_ranks_f32, csrc/g2k_ranks.hip; the
three heads' ``sample_ranks``; evaluate.py) against the float64 checker
tests/ranks_ref.py fed with the DEVICE's own draws (the head's sampler called K
times at seeds seed + k), so that the comparison sees the kernel's arithmetic
and not the draws'.  PARITY UNPINNED against the reference (it has no
probabilistic head).  A rank is an integer that compares fp32 sums: it must lie
in the checker's interval [r_lo, r_hi] (margins M and A of tests/ranks_ref.py)
for every pair and row, and the intervals wider than one rank stay below
WIDE_CAP of a case; hist and tot are exactly the sums of the device's own
per_ped.  The cases (tests/ranks_cases.py) are the smallest that reach each
path."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ranks_cases as rc
from tests import ranks_ref as rr
from tests.abi_arena import Arena, all_written
from tests.bestk_ref import MASK64, SEED_A

pytestmark = pytest.mark.gpu
ALL = [(i, w) for i in range(len(rc.CASES)) for w in rc.HEADS]
ALL_IDS = [f"{rc.IDS[i]}-{w}" for i, w in ALL]
STEMS = {"per_step": "g2k_sample_ranks", "fullcov": "g2k_fullcov_sample_ranks", "mix": "g2k_mix_sample_ranks"}
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
        c = rc.inputs(i)
        t = {k: _t(c[k], dev) for k in ("pred", "targets", "n_active", "n_frames", "ped_mask")}
        _DEV[(i, which)] = (_head(which, c, dev), t)
    return _DEV[(i, which)]


def _key(i, which, seed):
    """The caches' key: the case's own seed (None), or another."""
    return (i, which) if seed is None else (i, which, seed)


def _run(i, which, dev, want_per_ped=True, seed=None):
    c = rc.inputs(i)
    h, t = _device_inputs(i, which, dev)
    r = h.sample_ranks(t["pred"], t["targets"], t["n_active"], c["K"], c["B"],
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
    """The float64 checker over the device's own K draws (computed once)."""
    key = _key(i, which, seed)
    if key not in _REF:
        c = rc.inputs(i)
        h, t = _device_inputs(i, which, dev)
        s0 = c["seed"] if seed is None else seed
        draws = np.stack([h.sample(t["pred"], seed=(s0 + k) & MASK64).cpu().numpy()
                          for k in range(c["K"])])
        _REF[key] = rr.sample_ranks_ref(draws, c["targets"], c["pairs"])
    return _REF[key]


def _check_against(per, hist, tot, R, K, B, label):
    """per_ped inside the checker's intervals, degenerate steps agreeing
    outside the open ones, hist / tot the sums of per_ped and between the sums
    of the interval ends."""
    m = R["pairs"]
    assert np.isfinite(per).all()
    r = np.rint(per[..., :13]).astype(np.int64)
    assert np.all(per[..., :13] == r) and np.all(per[~m] == 0) and np.all(per[..., 14:] == 0)
    deg = r[..., :L] < 0
    settled = m[..., None] & ~R["deg_open"]
    opened = np.argwhere(m[..., None] & R["deg_open"])
    print(f"{label}: {int(m.sum())} pairs, degenerate steps {int(deg[m].sum())}, open to either outcome "
          f"{len(opened)}{': ' + str(opened.tolist()) if len(opened) else ''}")
    np.testing.assert_array_equal(deg[settled], R["deg"][settled])
    assert np.all(r[..., :L][deg] == -1)
    np.testing.assert_array_equal(per[..., 13][m], deg[m].sum(axis=-1))
    both = np.concatenate([m[..., None] & ~deg & ~R["deg"], m[..., None]], axis=-1)   # rows with an interval
    wide = float((R["r_hi"] > R["r_lo"])[both].mean()) if both.any() else 0.0
    outside = both & ((r < R["r_lo"]) | (r > R["r_hi"]))
    print(f"{label}: wide intervals {wide:.4f}, ranks off the float64 rank {int((r != R['r'])[both].sum())} of "
          f"{int(both.sum())}, outside their interval {int(outside.sum())}")
    assert wide <= rr.WIDE_CAP
    assert not outside.any(), np.argwhere(outside)[:5]
    # hist and tot: exactly the sums of the device's own per_ped
    want_h, want_t = rr.hist_tot(per, m, K, B)
    np.testing.assert_array_equal(hist, want_h)
    np.testing.assert_array_equal(tot, want_t)
    # ... and between the sums of the interval ends (rows both sides rank)
    lo, hi = np.where(both, R["r_lo"], 0), np.where(both, R["r_hi"], 0)
    rb = np.where(both, r, 0)
    assert lo[..., :L].sum() <= rb[..., :L].sum() <= hi[..., :L].sum()
    assert lo[..., L].sum() <= tot[:, 3].sum() <= hi[..., L].sum()
    w = (K + 1) // B
    for i in range(13):
        for b in range(1, B):                               # ranks below each bin edge
            got = int((rb[..., i][both[..., i]] < b * w).sum())
            assert int((hi[..., i][both[..., i]] < b * w).sum()) <= got <= int((lo[..., i][both[..., i]] < b * w).sum())


def _parity(dev, i, which, seed=None, label=""):
    c = rc.inputs(i)
    r, R = _result(i, which, dev, seed), _recount(i, which, dev, seed)
    per = r.per_ped.cpu().numpy().astype(np.float64)
    hist, tot = r.hist.cpu().numpy().astype(np.int64), r.tot.cpu().numpy()
    _check_against(per, hist, tot, R, c["K"], c["B"], f"case {rc.IDS[i]} {which}{label}")
    # the result class's figures are the counts'
    assert r.k == c["K"] and r.bins == c["B"] and r.pairs == int(c["pairs"].sum())
    if c["pairs"].any():
        hs = hist.sum(axis=0)
        np.testing.assert_allclose(r.hist_traj, hs[L] / hs[L].sum(), rtol=0, atol=1e-15)
        np.testing.assert_allclose(r.hist_pooled, hs[:L].sum(axis=0) / hs[:L].sum(), rtol=0, atol=1e-15)
        assert r.mean_traj == pytest.approx((tot[:, 3].sum() + 0.5 * r.pairs) / ((c["K"] + 1) * r.pairs))
        assert r.degenerate_share == 0.0 and 0.0 <= r.dev <= 1.0 and 0.0 <= r.dev_traj <= 1.0
    else:
        assert np.isnan(r.dev)


@pytest.mark.parametrize("i,which", ALL, ids=ALL_IDS)
def test_ranks_inside_the_checkers_intervals(gpu, i, which):
    _parity(gpu, i, which)


@pytest.mark.parametrize("which", rc.HEADS)
def test_seed_whose_low_word_carries(gpu, which):
    """Case k4 with the same assertions at seed A = 2^32 - 1, where draw 1's
    seed carries out of the low word: the launcher's split of the seed and
    drawn_lane's lo / hi arithmetic (csrc/g2k_drawn.h) against the samplers' at
    (seed + k) mod 2^64.  tests/test_sample_ranks.py: the checker's ranks
    change when the carry is dropped."""
    _parity(gpu, rc.IDS.index("k4"), which, SEED_A, " seed A")


def _raw_call(i, which, dev, per_ped, hist, tot, t=None, ws=None):
    """The entry point itself, on caller-made buffers."""
    from multimodaltraj_2_amd import _lib, ranks
    from multimodaltraj_2_amd.frame_step import _ptr
    lib = ranks.load()
    c = rc.inputs(i)
    h, t0 = _device_inputs(i, which, dev)
    t = t or dict(t0, params=_params(h, which))
    d = h._dims(t0["pred"])
    if c["shared"]:
        d.flags = _lib.STEP_TARGETS_SHARED
    need = int(lib.g2k_sample_ranks_workspace_bytes(ctypes.byref(d), c["B"]))
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc_ = getattr(lib, STEMS[which] + "_f32")(ctypes.byref(d), _ptr(t["pred"]), _ptr(t["targets"]),
                                              _ptr(t["n_active"]), _ptr(t["n_frames"]), _ptr(t["ped_mask"]),
                                              _ptr(t["params"]), ctypes.c_uint64(c["seed"]), c["K"], c["B"],
                                              _ptr(per_ped), _ptr(hist), _ptr(tot), _ptr(ws), need, None)
    torch.cuda.synchronize()
    assert rc_ == 0, lib.g2k_last_error()
    return need


FOOT = [rc.IDS.index(n) for n in ("k20", "passes", "tail")]


@pytest.mark.parametrize("which", rc.HEADS)
@pytest.mark.parametrize("i", FOOT, ids=[rc.IDS[i] for i in FOOT])
def test_determinism_and_footprint(gpu, i, which):
    """Guarded, poisoned outputs: every element written, nothing outside; the
    bits of a second call and of the Python path; per_ped NULL leaves hist's
    and tot's bits alone; non-pairs exactly zero."""
    c = rc.inputs(i)
    S, F, _, N = c["pred"].shape
    B = c["B"]
    ar = Arena(gpu)
    per = ar.alloc((S, F, N, 16), name="per_ped")
    hist, tot = ar.alloc((S, 13, B), torch.int32, name="hist"), ar.alloc((S, 4), torch.int64, name="tot")
    hist2, tot2 = ar.alloc((S, 13, B), torch.int32, name="hist2"), ar.alloc((S, 4), torch.int64, name="tot2")
    _raw_call(i, which, gpu, per, hist, tot)
    ar.check_guards()
    assert all_written(per) and all_written(hist) and all_written(tot)
    r = _result(i, which, gpu)
    assert torch.equal(per, r.per_ped) and torch.equal(hist, r.hist) and torch.equal(tot, r.tot)
    again = _run(i, which, gpu)
    assert torch.equal(again.per_ped, r.per_ped) and torch.equal(again.hist, r.hist) and torch.equal(again.tot, r.tot)
    _raw_call(i, which, gpu, None, hist2, tot2)
    ar.check_guards()
    assert all_written(hist2) and all_written(tot2) and torch.equal(hist2, hist) and torch.equal(tot2, tot)
    no = _run(i, which, gpu, want_per_ped=False)
    assert no.per_ped is None and torch.equal(no.hist, r.hist) and torch.equal(no.tot, r.tot)
    assert bool((per[~_t(c["pairs"], gpu)] == 0).all())
    assert not bool(torch.isnan(per).any())                                 # the poisoned columns were never read


def test_no_frames_writes_zeros(gpu):
    """F = 0 with S > 0: hist and tot are written, all zero."""
    from multimodaltraj_2_amd import _lib, ranks
    from multimodaltraj_2_amd.frame_step import _ptr
    lib = ranks.load()
    d = _lib.G2KDims(3, 0, 8, 12, 16, 64, 16, 8, 0)
    some = torch.zeros(64, device=gpu)                      # pred, targets, head: named, never read
    n_active = torch.full((3,), 16, dtype=torch.int32, device=gpu)
    ar = Arena(gpu)
    hist, tot = ar.alloc((3, 13, 7), torch.int32, name="hist"), ar.alloc((3, 4), torch.int64, name="tot")
    need = int(lib.g2k_sample_ranks_workspace_bytes(ctypes.byref(d), 7))
    ws = ar.alloc((need,), torch.uint8, name="workspace")
    for stem in STEMS.values():
        rc_ = getattr(lib, stem + "_f32")(ctypes.byref(d), _ptr(some), _ptr(some), _ptr(n_active), None, None,
                                          _ptr(some), ctypes.c_uint64(1), 20, 7, None, _ptr(hist), _ptr(tot),
                                          _ptr(ws), need, None)
        torch.cuda.synchronize()
        assert rc_ == 0, lib.g2k_last_error()
        ar.check_guards()
        assert not bool(hist.any()) and not bool(tot.any())
        hist.fill_(5)
        tot.fill_(5)


@pytest.mark.parametrize("which", ("per_step", "fullcov"))
def test_identical_draws_are_degenerate(gpu, which):
    """sigma = 0 (log sigma = -200; a zero factor): the K draws are the
    prediction itself, every step's pooled points lie on a line: 12 degenerate
    steps a pair, rows 0..11 of hist empty, r_traj = K."""
    from multimodaltraj_2_amd.fullcov import FullCovHead
    from multimodaltraj_2_amd.nll import GaussianHead
    K, B, N = 20, 21, 6
    if which == "per_step":
        h = GaussianHead(log_sigma=-200.0, device=gpu)
    else:
        h = FullCovHead(device=gpu)
        h.chol = torch.zeros((24, 24), device=gpu)
    rng = np.random.default_rng(17)
    pred = rng.integers(-3, 4, (1, 1, 24, N)).astype(np.float32)
    tg = rr.band_to_xy(pred).astype(np.float32).copy()
    tg[..., 0:5, 0] += 2.0
    tg[..., 5:10, 1] -= 3.0
    r = h.sample_ranks(_t(pred, gpu), _t(tg, gpu), torch.full((1,), N, dtype=torch.int32, device=gpu), K, B,
                       want_per_ped=True)
    per = r.per_ped.cpu().numpy()
    assert np.all(per[..., :12] == -1) and np.all(per[..., 12] == K) and np.all(per[..., 13] == 12)
    hist = r.hist.cpu().numpy()
    assert not hist[:, :12].any() and hist[0, 12, 20] == N
    assert r.tot.cpu().tolist() == [[N, 12 * N, 0, K * N]] and r.degenerate_share == 1.0


@pytest.mark.parametrize("which", rc.HEADS)
def test_at_minimum_alignment(gpu, which):
    """Each entry point at the weakest pointer alignment its header line
    states (targets 8, per_ped 16, hist 4, tot 8, workspace 8) and every other
    pointer at its element's own (4; the mask 1): the bits of the aligned
    call."""
    i = rc.IDS.index("shared")
    c = rc.inputs(i)
    S, F, _, N = c["pred"].shape
    h, _ = _device_inputs(i, which, gpu)
    ar = Arena(gpu)
    t = dict(pred=ar.put(c["pred"], "pred", 4), targets=ar.put(c["targets"], "targets", 8),
             n_active=ar.put(c["n_active"], "n_active", 4), n_frames=ar.put(c["n_frames"], "n_frames", 4),
             ped_mask=ar.put(c["ped_mask"], "ped_mask", 1),
             params=ar.put(_params(h, which).cpu().numpy(), "params", 4))
    assert t["targets"].data_ptr() % 16 == 8 and t["pred"].data_ptr() % 16 == 4
    per = ar.alloc((S, F, N, 16), name="per_ped")
    hist = ar.alloc((S, 13, c["B"]), torch.int32, name="hist", offset=4)
    tot = ar.alloc((S, 4), torch.int64, name="tot", offset=8)
    from multimodaltraj_2_amd import ranks
    need = ranks.load().g2k_sample_ranks_workspace_bytes(ctypes.byref(h._dims(_t(c["pred"], "cpu"))), c["B"])
    ws = ar.alloc((need,), torch.uint8, name="workspace", offset=8)
    assert hist.data_ptr() % 8 == 4 and tot.data_ptr() % 16 == 8 and ws.data_ptr() % 16 == 8
    assert _raw_call(i, which, gpu, per, hist, tot, t=t, ws=ws) == need
    ar.check_guards()
    r = _result(i, which, gpu)
    assert torch.equal(per, r.per_ped) and torch.equal(hist, r.hist) and torch.equal(tot, r.tot)


@pytest.mark.parametrize("which", rc.HEADS)
def test_exchangeability_on_the_device(gpu, which):
    """Targets = head.sample(pred, seed + K) re-laid as targets: the K + 1
    trajectories are exchangeable, step 11's rank and the trajectory's are
    uniform over the 21 bins (Pearson's chi^2 below the 0.999 quantile at 20
    degrees of freedom; fixed seeds, so deterministic); the same targets under a
    head three times too wide are not."""
    S, F, N, K, B, seed = 4, 4, 128, 20, 21, 777
    c = rc.inputs(rc.IDS.index("k20"))
    rng = np.random.default_rng(5)
    pred = _t(rng.standard_normal((S, F, 24, N)).astype(np.float32), gpu)
    n_active = torch.full((S,), N, dtype=torch.int32, device=gpu)
    h = _head(which, c, gpu)
    y = h.sample(pred, seed=seed + K)                                       # [S, F, 24, N]
    tg = torch.stack([y[:, :, :L], y[:, :, L:]], dim=-1).permute(0, 1, 3, 2, 4).contiguous()
    quant = rr.chi2_quantile(0.999, B - 1)
    r = h.sample_ranks(pred, tg, n_active, K, B, seed=seed)
    counts = r.counts()
    x11, xt = rr.chi2(counts[L - 1]), rr.chi2(counts[L])
    print(f"{which}: {r.pairs} pairs, chi^2 step 11 {x11:.2f} trajectory {xt:.2f} (quantile {quant:.2f}), "
          f"distance from uniform {r.dev:.4f} / {r.dev_traj:.4f}, mean rank {r.mean:.4f} / {r.mean_traj:.4f}")
    assert r.pairs == S * F * N and x11 < quant and xt < quant
    assert abs(r.mean - 0.5) < 0.01 and abs(r.mean_traj - 0.5) < 0.03
    wide = _head(which, rc.scaled(which, c, 3.0), gpu)
    rw = wide.sample_ranks(pred, tg, n_active, K, B, seed=seed)
    cw = rw.counts()
    print(f"{which}, three times too wide: chi^2 step 11 {rr.chi2(cw[L - 1]):.2f} trajectory {rr.chi2(cw[L]):.2f}, "
          f"mean rank {rw.mean:.4f} / {rw.mean_traj:.4f}")
    assert rr.chi2(cw[L - 1]) > quant and rr.chi2(cw[L]) > quant and rw.mean < 0.45


def test_python_argument_checks(gpu):
    for which in rc.HEADS:
        h, t = _device_inputs(0, which, gpu)
        for k in (3, 256):
            with pytest.raises(ValueError, match="4..255"):
                h.sample_ranks(t["pred"], t["targets"], t["n_active"], k)
        with pytest.raises(ValueError, match="a divisor of k \\+ 1"):
            h.sample_ranks(t["pred"], t["targets"], t["n_active"], 20, 4)
        with pytest.raises(ValueError, match="targets must be"):
            h.sample_ranks(t["pred"], t["targets"][:, :1], t["n_active"], 4)
        with pytest.raises(ValueError, match="n_active must be"):
            h.sample_ranks(t["pred"], t["targets"], t["n_active"][:1], 4)


def test_evaluation_end_to_end(gpu, tmp_path, data_root):
    """The recipe of tests/test_sample_scores_gpu.py::test_evaluation_end_to_end
    with --num_samples 20 --sample_ranks 1, without and with --fullcov_head
    train and --mixture_head train: the new keys at the end of each head's
    block, finite and equal to a direct call on ``keep``'s tensors; the old keys
    and values unchanged, one more log line per head; without the flag the
    parent's keys; K = 3 with the flag raises."""
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
    assert args.sample_ranks == 0 and args.rank_bins == 0
    tr.run_train_mode(args, gpu, log=lambda s: None)
    prm = checkpoint.load_params(checkpoint.read_state(str(tmp_path)), device=gpu)
    logs0, keep0 = [], {}
    res0 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs0.append, keep=keep0)
    assert list(res0) == ["scenes", "pairs", "K"] + list(evaluate.FIGURES)
    assert "ranks" not in keep0 and not any("sample ranks" in s for s in logs0)

    args.sample_ranks = 1
    logs1, keep1 = [], {}
    res1 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs1.append, keep=keep1)
    assert list(res1) == list(res0) + list(evaluate.RANK_FIGURES)
    assert {k: res1[k] for k in res0} == res0 and logs1[:len(logs0)] == logs0 and len(logs1) == len(logs0) + 1
    assert logs1[-1].startswith("sample ranks of the 20 draws on dataset 2: 21 bins,")
    t = keep1["plan"].to_device(gpu, F=1)
    one = torch.ones(keep1["plan"].S, dtype=torch.int32, device=gpu)
    gh = GaussianHead(device=gpu)
    gh.head = keep1["head"]
    kw = dict(seed=args.sample_seed, n_frames=one, ped_mask=t["ped_mask"])
    direct = gh.sample_ranks(keep1["pred"], t["targets"], t["n_active"], 20, **kw)
    want = evaluate.rank_figures(direct)
    for k in evaluate.RANK_FIGURES:
        print(f"evaluation {k}: {res1[k]:.8g}")
        assert np.isfinite(res1[k]) and res1[k] == want[k], k
    assert torch.equal(keep1["ranks"].hist, direct.hist) and torch.equal(keep1["ranks"].tot, direct.tot)
    assert direct.pairs == res1["pairs"] and keep1["ranks"].per_ped is not None and direct.bins == 21
    assert res1["rank_nom50"] == 10 / 21 and res1["rank_nom90"] == 18 / 21
    assert f"{res1['rank_dev']:.4f}" in logs1[-1]

    # --rank_bins; with both other heads; the flag off first: the parent's keys
    args.rank_bins = 7
    res7 = evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
    assert res7["rank_nom50"] == 3 / 7 and res7["rank_mean"] == res1["rank_mean"]
    args.sample_ranks, args.rank_bins, args.fullcov_head, args.mixture_head = 0, 0, "train", "train"
    logs_off = []
    res_off = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs_off.append)
    assert list(res_off) == list(res0) + list(evaluate.FULLCOV_FIGURES) + list(evaluate.MIX_FIGURES)
    args.sample_ranks = 1
    logs2, keep2 = [], {}
    res2 = evaluate.evaluate_best_of_k(args, prm, gpu, log=logs2.append, keep=keep2)
    assert list(res2) == (list(res1) + list(evaluate.FULLCOV_FIGURES) + list(evaluate.FULLCOV_RANK_FIGURES)
                          + list(evaluate.MIX_FIGURES) + list(evaluate.MIX_RANK_FIGURES))
    assert {k: res2[k] for k in res1} == res1 and {k: res2[k] for k in res_off} == res_off
    assert len(logs2) == len(logs_off) + 3
    assert [s for s in logs2 if "sample ranks" not in s] == logs_off
    assert sum(s.startswith("full-covariance sample ranks of the 20 draws on dataset 2:") for s in logs2) == 1
    assert logs2[-1].startswith("mixture sample ranks of the 20 draws on dataset 2:")
    fc = FullCovHead(device=gpu)
    fc.chol = keep2["fullcov_chol"]
    fwant = evaluate.rank_figures(fc.sample_ranks(keep2["pred"], t["targets"], t["n_active"], 20, **kw), "fullcov_")
    mdirect = keep2["mixture"]["head"].sample_ranks(keep2["pred"], t["targets"], t["n_active"], 20, **kw)
    mwant = evaluate.rank_figures(mdirect, "mix_")
    for k, v in list(fwant.items()) + list(mwant.items()):
        print(f"evaluation {k}: {res2[k]:.8g}")
        assert np.isfinite(res2[k]) and res2[k] == v, k
    assert torch.equal(keep2["mixture"]["ranks"].hist, mdirect.hist)
    assert keep2["fullcov"]["ranks"].pairs == mdirect.pairs == res2["pairs"]
    # the CLI, and K outside 4..255
    cli = evaluate.main(argv + ["--sample_ranks", "1", "--fullcov_head", "train", "--mixture_head", "train"],
                        log=lambda s: None)
    assert list(cli) == list(res2) and [cli[k] for k in res2] == [res2[k] for k in res2]
    for k in (3, 256):
        args.num_samples = k
        with pytest.raises(ValueError, match="4 <= K <= 255"):
            evaluate.evaluate_best_of_k(args, prm, gpu, log=lambda s: None)
