"""GPU: the fixed-frame forward build (g2k_scene_kernel<..., FX = 20>: F, the
chunk length and stride 1 compile-time constants, the position window aliased
onto the As ring, three workgroups per CU at Nmax 32).

Part 1, outputs: pred and h of the fixed build are bit for bit those of the
same inputs' launch without G2K_STEP_CORESIDENT (the unspecialised 12-producer
build: the same per-frame arithmetic; the metric sums add the producers'
partials in another grouping: 1e-4), and pred / h / metrics match the float64
oracle at tests/test_step_gpu.py's tolerances (pred, metrics: close() <= 1e-4;
h: close_h, 1e-5 relative, with h_in drawn N(0, 1)).

Part 2, launches in flight: twelve S = 256 batches round-robin over four
streams compute, bit for bit, what each launch computes alone (the test of the
aliasing and of three workgroups sharing a CU), and a plan run again on
changed inputs computes what a fresh plan computes (nothing a launch leaves in
the ring is ever read as positions)."""
import functools

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import frame_step as fs
from multimodaltraj_2_amd.synthetic import make_batch
from oracle import g2k_ref as ref
from tests.conftest import close, close_h

TOL = 1e-4
F, S = 20, 3
pytestmark = pytest.mark.gpu

N_FRAMES = {"n_frames-0-1-20": (0, 1, 20), "n_frames-none": None}


@functools.lru_cache(maxsize=None)
def case(H, Nmax, frames_id):
    """The inputs of one (H, Nmax, n_frames) case and their oracle outputs,
    shared by both pred layouts: n_active (0, 1, 20) — 20 crosses a tile at
    Nmax 32 and is every pedestrian below it —, one masked pedestrian, h_in
    N(0, 1)."""
    n_active = np.array([0, 1, min(20, Nmax)], np.int32)
    b = make_batch(S, Nmax, H, F=F, seed=31 + Nmax, n_active=n_active, h0_scale=1.0)
    mask = np.ones((S, Nmax), bool)
    mask[2, 5] = False
    n_frames = N_FRAMES[frames_id]
    w = fs.init_params(Nmax, seed=0).numpy()
    want = []
    for s in range(S):
        nf = F if n_frames is None else n_frames[s]
        pr, h, m, _ = ref.scene_step(b.pos[s], b.vislet[s], b.G[s], w, b.targets[s], int(n_active[s]),
                                     b.h0[s], n_frames=nf, stride=1, ped_mask=mask[s])
        want.append((pr, h, m, nf))
    return b, mask, n_frames, want


@pytest.mark.parametrize("frames_id", list(N_FRAMES))
@pytest.mark.parametrize("layout", ["band", "ped"])
@pytest.mark.parametrize("Nmax", [16, 17, 32])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_fixed_build_outputs(gpu, H, Nmax, layout, frames_id):
    """TPW 1, 2, 4; one tile, an odd Nmax (the 4-byte position DMA) and two
    tiles; both pred layouts; empty, one-pedestrian and one-frame scenes."""
    assert fs.step_fixed_geometry(S, F, H, Nmax, coresident=True, pred_layout=layout)["frames"] == F
    assert fs.step_fixed_geometry(S, F, H, Nmax, pred_layout=layout)["frames"] == 0
    b, mask, n_frames, want = case(H, Nmax, frames_id)
    t = b.to_device(gpu)
    params = fs.init_params(Nmax, seed=0, device=gpu)
    kw = dict(n_frames=None if n_frames is None else torch.tensor(n_frames, dtype=torch.int32, device=gpu),
              ped_mask=torch.from_numpy(mask.astype(np.uint8)).to(gpu), pred_layout=layout,
              want_attn=True)
    args = (params, t["pos"], t["vislet"], t["G"], t["targets"], t["n_active"], t["h0"])
    out = fs.step_fused(*args, coresident=True, **kw)
    base = fs.step_fused(*args, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out.pred, base.pred)
    assert torch.equal(out.h, base.h)
    met, bmet = out.metrics.cpu().numpy(), base.metrics.cpu().numpy()
    worst = dict(metrics_vs_base=close(met, bmet), pred=0.0, metrics=0.0, h=0.0)
    pred, hh = fs.pred_band(out.pred, layout).cpu().numpy(), out.h.cpu().numpy()
    for s in range(S):
        n = int(b.n_active[s])
        pr, h, m, nf = want[s]
        # the frames a scene has: A and cost too (the same values, other waves)
        assert torch.equal(out.attn[s, :nf], base.attn[s, :nf])
        assert torch.equal(out.cost[s, :nf], base.cost[s, :nf])
        worst["pred"] = max(worst["pred"], close(pred[s, :nf, :, :n].reshape(nf, 2, 12, n), pr))
        worst["metrics"] = max(worst["metrics"], close(met[s, :6], m[:6]))
        worst["h"] = max(worst["h"], float((np.abs(hh[s] - h) / (1e-5 * np.abs(h) + 1e-8)).max()))
        assert close_h(hh[s], h), (s, worst)
        assert np.all(pred[s, nf:] == 0) and np.all(pred[s, :, :, n:] == 0)
        assert met[s, 5] == nf and met[s, 1] == m[1]
    print(f"H {H} Nmax {Nmax} {layout} {frames_id}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
          + " (bounds 1e-4, 1e-4, 1e-4, 1 [h in units of its bound])")
    assert worst["metrics_vs_base"] <= TOL and worst["pred"] <= TOL and worst["metrics"] <= TOL


N_FLIGHT, S_FLIGHT, NMAX, HID = 12, 256, 32, 128


@pytest.fixture(scope="module")
def flight(gpu):
    """Twelve independent S = 256 batches (Nmax 32, H 128), their plans on four
    streams and each launch's outputs when it runs alone."""
    assert fs.step_workgroups_per_cu(S_FLIGHT, F, HID, NMAX, 27, 1, True) == 3
    params = fs.init_params(NMAX, seed=0, device=gpu)
    streams = [torch.cuda.Stream(device=gpu) for _ in range(4)]
    batches, plans, alone = [], [], []
    for k in range(N_FLIGHT):
        t = make_batch(S_FLIGHT, NMAX, HID, seed=40 + k, h0_scale=1.0).to_device(gpu)
        args = (params, t["pos"], t["vislet"], t["G"], t["targets"], t["n_active"], t["h0"])
        batches.append(args)
        plans.append(fs.StepPlan(*args, stream=streams[k % 4], pred_layout="ped", coresident=True))
        o = fs.step_fused(*args, pred_layout="ped", coresident=True)
        torch.cuda.synchronize()
        alone.append((o.pred.clone(), o.h.clone(), o.metrics.clone()))
    return params, batches, plans, alone


def test_fixed_build_launches_in_flight(gpu, flight):
    params, batches, plans, alone = flight
    # the first batch against the 12-producer build: the launches compared
    # below are right, not merely equal
    base = fs.step_fused(*batches[0], pred_layout="ped")
    torch.cuda.synchronize()
    assert torch.equal(alone[0][0], base.pred) and torch.equal(alone[0][1], base.h)
    assert close(alone[0][2].cpu().numpy(), base.metrics.cpu().numpy()) <= TOL
    for _ in range(3):
        for p in plans:
            p.run()
    torch.cuda.synchronize()
    for k, (p, (pred, h, met)) in enumerate(zip(plans, alone)):
        assert torch.equal(p.out.pred, pred), k
        assert torch.equal(p.out.h, h), k
        assert torch.equal(p.out.metrics, met), k


def test_fixed_build_plan_rerun_on_changed_inputs(gpu, flight):
    """A plan's second run, on other inputs in the same buffers, equals a fresh
    plan's first run on them: the As ring's content of the first run (where
    the position window lands) is not an input of the second."""
    params, batches, plans, alone = flight
    src, dst = batches[1], batches[0]
    bufs = [x.clone() for x in dst[1:]]
    plan = fs.StepPlan(params, *bufs, pred_layout="ped", coresident=True)
    plan.run()
    torch.cuda.synchronize()
    for a, want in zip((plan.out.pred, plan.out.h, plan.out.metrics), alone[0]):
        assert torch.equal(a, want)
    for buf, new in zip(bufs, src[1:]):
        buf.copy_(new)
    plan.run()
    torch.cuda.synchronize()
    # (columns past n_active keep the first run's values: compare through n_active)
    n_active = src[5].cpu().numpy()
    fresh_pred = alone[1][0]
    for s in range(0, S_FLIGHT, 7):
        n = int(n_active[s])
        assert torch.equal(plan.out.pred[s, :, :n], fresh_pred[s, :, :n]), s
    assert torch.equal(plan.out.h, alone[1][1])
    assert torch.equal(plan.out.metrics, alone[1][2])
