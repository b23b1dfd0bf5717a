"""GPU: the fixed-frame forward build (g2k_scene_kernel<..., FX = 20>) over the
whole range of Nmax it serves — the cases of tests/step_fixed_cases.py: 3 to 7
prediction tiles over the four producer waves, the position window filling the
As ring it is aliased onto (Nmax 93 / 94), the window of its own from Nmax 95
to N_LAST, the three TPW builds at those widths, both pred layouts, scenes that
stop mid-chain, a mask in the first and the last tile.

Part 1, outputs (every case): pred, h and the run frames' attn / cost are bit
for bit those of the same inputs' launch without G2K_STEP_CORESIDENT (the
12-producer build: another kernel, another layout, the same per-frame
arithmetic; its metric sums group the producers' partials differently: 1e-4),
and pred / h / metrics match the float64 oracle at tests/test_step_gpu.py's
tolerances (pred, metrics: close() <= 1e-4; h: close_h).  The pedestrian-major
pred starts as NaN: what the kernel does not own stays NaN.

Part 2, one target set for every frame at stride 1 (G2K_STEP_TARGETS_SHARED:
the one field of the layout the kernel takes from the host) against the same
set replicated over the frames, and a pos buffer with rows past the window
(W = 30: W is a runtime value of this build) against the window alone.

Part 3, across launches at the widest aliased window (Nmax 94, and 95 beside
it): a plan run again on changed inputs computes what a fresh plan computes,
and launches in flight on four streams compute what each computes alone."""
import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import frame_step as fs
from multimodaltraj_2_amd.synthetic import make_batch
from tests import step_fixed_cases as cases
from tests.conftest import close, close_h

TOL = 1e-4
F, S = cases.F, cases.S
pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    """Bit for bit (NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def assert_bits(a, b, what):
    if not same_bits(a, b):                       # (no tensor dump: say how much differs)
        n = int((bits(a) != bits(b)).sum()) if a.shape == b.shape else -1
        raise AssertionError(f"{what}: {n} of {a.numel()} words differ")


def device_inputs(case, gpu):
    """The case's inputs on the device (copies: the cached host arrays stay as
    they are) and its oracle outputs."""
    b, want = cases.reference(case.key)
    t = {k: torch.tensor(getattr(b, k), device=gpu)
         for k in ("pos", "vislet", "G", "targets", "n_active", "h0")}
    t["ped_mask"] = torch.tensor(case.mask().astype(np.uint8), device=gpu)
    nf = case.n_frames
    t["n_frames"] = None if nf is None else torch.tensor(nf, dtype=torch.int32, device=gpu)
    return b, t, want


def fresh_out(case, gpu):
    """Outputs the launch writes into: pred zero in the band layout (as
    step_fused allocates it), NaN in the pedestrian-major one."""
    shape = fs.pred_shape(S, F, case.Nmax, case.layout)
    pred = (torch.zeros(shape, device=gpu) if case.layout == "band"
            else torch.full(shape, float("nan"), device=gpu))
    return fs.StepOutputs(pred=pred, h=torch.empty((S, fs.HIDDEN_LEN, case.H), device=gpu),
                          metrics=torch.empty((S, 8), device=gpu),
                          attn=torch.empty((S, F, fs.HIDDEN_LEN, fs.HIDDEN_LEN), device=gpu),
                          cost=torch.empty((S, F, fs.OBS_LEN, fs.OBS_LEN), device=gpu))


def launch(case, gpu, t, *, coresident=True, pos=None, targets=None, shared=False):
    params = fs.init_params(case.Nmax, seed=0, device=gpu)
    return fs.step_fused(params, t["pos"] if pos is None else pos, t["vislet"], t["G"],
                         t["targets"] if targets is None else targets, t["n_active"], t["h0"],
                         n_frames=t["n_frames"], ped_mask=t["ped_mask"], pred_layout=case.layout,
                         out=fresh_out(case, gpu), targets_shared=shared, frames=F if shared else None,
                         coresident=coresident)


def assert_same_launch(case, got, base, *, metrics_bitwise):
    """pred, h, the run frames' attn and cost bit for bit; the metrics bit for
    bit or within 1e-4 -> their close() distance."""
    assert_bits(got.pred, base.pred, "pred")
    assert_bits(got.h, base.h, "h")
    for s, nf in enumerate(case.frames):
        assert_bits(got.attn[s, :nf], base.attn[s, :nf], s)
        assert_bits(got.cost[s, :nf], base.cost[s, :nf], s)
    if metrics_bitwise:
        assert_bits(got.metrics, base.metrics, "metrics")
    d = close(got.metrics.cpu().numpy(), base.metrics.cpu().numpy())
    assert d <= TOL
    return d


def assert_oracle(case, out, want):
    """pred / h / metrics against the float64 oracle and the write footprint
    -> the worst errors (h in units of its bound)."""
    worst = dict(pred=0.0, metrics=0.0, h=0.0)
    raw = out.pred.cpu().numpy()
    pred = fs.pred_band(out.pred, case.layout).cpu().numpy()
    hh, met = out.h.cpu().numpy(), out.metrics.cpu().numpy()
    for s in range(S):
        n = case.n_active[s]
        pr, h, m, nf = want[s]
        assert nf == case.frames[s] and pr.shape == (nf, 2, 12, n)
        worst["pred"] = max(worst["pred"], close(pred[s, :nf, :, :n].reshape(nf, 2, 12, n), pr))
        worst["metrics"] = max(worst["metrics"], close(met[s, :6], m[:6]))
        worst["h"] = max(worst["h"], float((np.abs(hh[s] - h) / (1e-5 * np.abs(h) + 1e-8)).max()))
        assert close_h(hh[s], h), (s, worst)
        assert met[s, 5] == nf and met[s, 1] == m[1], (s, met[s], m)
        if case.layout == "band":                 # [S, F, 2L, Nmax]: as allocated, zero
            assert np.all(raw[s, nf:] == 0) and np.all(raw[s, :, :, n:] == 0), s
        else:                                     # [S, F, Nmax, L, 2]: as allocated, NaN
            assert np.isnan(raw[s, nf:]).all() and np.isnan(raw[s, :, n:]).all(), s
            assert not np.isnan(raw[s, :nf, :n]).any(), s
    assert worst["pred"] <= TOL and worst["metrics"] <= TOL, worst
    return worst


def report(case, worst):
    print(f"{case.id} ({case.tiles} tiles, {'aliased' if case.aliased else 'own'} window, "
          f"{case.wgs_per_cu} per CU): " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
          + " (bounds: 1e-4; h in units of its bound, 1)")


@pytest.mark.parametrize("case", cases.OUTPUT_CASES, ids=lambda c: c.id)
def test_fixed_build_outputs_over_its_nmax_range(gpu, case):
    g = cases.fixed_geometry(case)
    assert g["frames"] == F and g["workgroups_per_cu"] == case.wgs_per_cu
    assert cases.fixed_geometry(case, coresident=False)["frames"] == 0
    assert fs.step_geometry(S, F, case.H, case.Nmax, pred_layout=case.layout)["np"] == 12
    b, t, want = device_inputs(case, gpu)
    out = launch(case, gpu, t)
    base = launch(case, gpu, t, coresident=False)
    torch.cuda.synchronize()
    worst = dict(metrics_vs_base=assert_same_launch(case, out, base, metrics_bitwise=False))
    worst.update(assert_oracle(case, out, want))
    report(case, worst)


@pytest.mark.parametrize("case", cases.SHARED_CASES, ids=lambda c: c.id)
def test_shared_targets_at_stride_1_equal_replicated(gpu, case):
    """targets [S, 1, Nmax, L, 2] for every frame: the fixed build with a
    target stride of 0 (not the loop-invariant kernel, which needs stride 0
    of the window as well)."""
    assert cases.fixed_geometry(case)["frames"] == F                        # shared
    assert fs.step_fixed_geometry(S, F, case.H, case.Nmax, coresident=True,
                                  pred_layout=case.layout)["frames"] == F   # replicated
    assert fs.step_geometry(S, F, case.H, case.Nmax, coresident=True, targets_shared=True,
                            pred_layout=case.layout)["variant"] == "general"
    b, t, want = device_inputs(case, gpu)
    first = t["targets"][:, :1].contiguous()
    assert torch.equal(t["targets"], first.expand_as(t["targets"]))
    got = launch(case, gpu, t, targets=first, shared=True)
    rep = launch(case, gpu, t)
    torch.cuda.synchronize()
    worst = dict(metrics_vs_replicated=assert_same_launch(case, got, rep, metrics_bitwise=False))
    worst.update(assert_oracle(case, got, want))
    report(case, worst)
    print(f"{case.id}: metrics bitwise equal to the replicated launch's: "
          f"{same_bits(got.metrics, rep.metrics)}")


@pytest.mark.parametrize("case", cases.LONG_POS_CASES, ids=lambda c: c.id)
def test_rows_of_pos_past_the_window_are_not_read(gpu, case):
    """W = 30: three rows of 1e30 after each scene's window (they shift every
    later scene's rows in the buffer).  Every output is bit for bit the
    W = 27 launch's."""
    assert cases.fixed_geometry(case) == cases.fixed_geometry(cases.plain_twin(case))
    b, t, want = device_inputs(case, gpu)
    long_pos = torch.full((S, case.W, case.Nmax, 2), 1e30, device=gpu)
    long_pos[:, :cases.W_PLAIN] = t["pos"]
    assert long_pos.shape[1] == 30 and t["pos"].shape[1] == 27
    got = launch(case, gpu, t, pos=long_pos)
    plain = launch(case, gpu, t)
    torch.cuda.synchronize()
    assert_same_launch(case, got, plain, metrics_bitwise=True)
    report(case, assert_oracle(case, got, want))


# ---------------------------------------------------------------------------
# across launches, at the widest aliased window
# ---------------------------------------------------------------------------
H_WIDE = 64


def wide_batch(gpu, S_, Nmax, seed):
    t = make_batch(S_, Nmax, H_WIDE, seed=seed, h0_scale=1.0).to_device(gpu)
    return (t["pos"], t["vislet"], t["G"], t["targets"], t["n_active"], t["h0"])


@pytest.mark.parametrize("Nmax", [94, 95])
def test_plan_rerun_on_changed_inputs_at_the_widest_window(gpu, Nmax):
    """A plan's second run, on another batch in the same buffers, equals a
    fresh plan's run on that batch: at Nmax 94 the first run's ring content
    lies under all but 44 floats of the second run's window."""
    S_ = 16
    assert fs.step_fixed_geometry(S_, F, H_WIDE, Nmax, coresident=True, pred_layout="ped")["frames"] == F
    params = fs.init_params(Nmax, seed=0, device=gpu)
    first, second = wide_batch(gpu, S_, Nmax, 70 + Nmax), wide_batch(gpu, S_, Nmax, 170 + Nmax)
    fresh_plans = [fs.StepPlan(params, *x, pred_layout="ped", coresident=True) for x in (first, second)]
    fresh = [p.run() for p in fresh_plans]
    bufs = [x.clone() for x in first]
    plan = fs.StepPlan(params, *bufs, pred_layout="ped", coresident=True)
    plan.run()
    torch.cuda.synchronize()
    for k in ("pred", "h", "metrics"):
        assert_bits(getattr(plan.out, k), getattr(fresh[0], k), k)
    for buf, new in zip(bufs, second):
        buf.copy_(new)
    plan.run()
    torch.cuda.synchronize()
    # (columns past n_active keep the first run's values: compare through n_active)
    for s, n in enumerate(second[4].cpu().numpy()):
        assert_bits(plan.out.pred[s, :, :int(n)], fresh[1].pred[s, :, :int(n)], s)
    assert_bits(plan.out.h, fresh[1].h, "h")
    assert_bits(plan.out.metrics, fresh[1].metrics, "metrics")
    # ... and the fresh run is right, not merely equal: the 12-producer build on the same batch
    base = fs.step_fused(params, *second, pred_layout="ped")
    torch.cuda.synchronize()
    assert_bits(fresh[1].pred, base.pred, "pred vs 12 producers")
    assert_bits(fresh[1].h, base.h, "h vs 12 producers")
    assert close(fresh[1].metrics.cpu().numpy(), base.metrics.cpu().numpy()) <= TOL


def test_launches_in_flight_at_the_widest_window(gpu):
    """Eight S = 256 batches (Nmax 94, H 64) round-robin over four streams,
    three rounds, two workgroups per CU: each plan's outputs are bit for bit
    what its launch computes alone."""
    Nmax, S_, n_flight = 94, 256, 8
    g = fs.step_fixed_geometry(S_, F, H_WIDE, Nmax, coresident=True, pred_layout="ped")
    assert g["frames"] == F and g["workgroups_per_cu"] == 2
    assert fs.step_workgroups_per_cu(S_, F, H_WIDE, Nmax, 27, 1, True) == 2
    params = fs.init_params(Nmax, seed=0, device=gpu)
    streams = [torch.cuda.Stream(device=gpu) for _ in range(4)]
    plans, alone = [], []
    for k in range(n_flight):
        args = wide_batch(gpu, S_, Nmax, 240 + k)
        plans.append(fs.StepPlan(params, *args, stream=streams[k % 4], pred_layout="ped", coresident=True))
        o = fs.step_fused(params, *args, pred_layout="ped", coresident=True)
        torch.cuda.synchronize()
        alone.append(o)
        if k == 0:                                # right, not merely equal
            base = fs.step_fused(params, *args, pred_layout="ped")
            torch.cuda.synchronize()
            assert_bits(o.pred, base.pred, "pred vs 12 producers")
            assert_bits(o.h, base.h, "h vs 12 producers")
            assert close(o.metrics.cpu().numpy(), base.metrics.cpu().numpy()) <= TOL
    for _ in range(3):
        for p in plans:
            p.run()
    torch.cuda.synchronize()
    for k, (p, o) in enumerate(zip(plans, alone)):
        assert_bits(p.out.pred, o.pred, k)
        assert_bits(p.out.h, o.h, k)
        assert_bits(p.out.metrics, o.metrics, k)
