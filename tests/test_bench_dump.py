"""bench.py --dump-outputs: after the timed steps the last timed step's
outputs (pred, h, metrics of its batch) are written as DIR/<name>.npy, float32,
within bench.DUMP_LIMIT bytes in all (a larger array as a fixed seeded sample);
a plain run measures nothing beyond its timed steps."""
import json
import types

import numpy as np
import pytest
import torch

import bench
from multimodaltraj_2_amd import frame_step as fs
from multimodaltraj_2_amd.synthetic import make_batch


def _fake_out(seed):
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(pred=torch.randn((4, 5, 6, 12, 2), generator=g),
                                 h=torch.randn((4, 16, 8), generator=g),
                                 metrics=torch.randn((4, 8), generator=g))


def test_dump_whole_and_sampled(tmp_path, monkeypatch):
    out = _fake_out(0)
    bench.dump_outputs(str(tmp_path / "whole"), out)
    for k in ("pred", "h", "metrics"):
        a = np.load(tmp_path / "whole" / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, getattr(out, k).numpy())
    # over the limit: arrays above their share become the same sample in every
    # run, the small ones stay whole, the total stays within the limit
    limit = 3 * 1024
    monkeypatch.setattr(bench, "DUMP_LIMIT", limit)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in ("pred", "h", "metrics")}
    assert sum(a.nbytes for a in got.values()) <= limit
    assert got["pred"].shape == (256,) and got["h"].shape == (256,)
    assert np.array_equal(got["metrics"], out.metrics.numpy())
    assert np.isin(got["pred"], out.pred.numpy()).all()
    for k, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{k}.npy"))
    # another build's outputs are sampled at the same entries
    other = _fake_out(1)
    bench.dump_outputs(str(tmp_path / "c"), other)
    idx = np.flatnonzero(np.isin(out.pred.numpy().reshape(-1), got["pred"]))
    assert np.array_equal(np.load(tmp_path / "c" / "pred.npy"), other.pred.numpy().reshape(-1)[idx])


def _bench_batch(gpu, k, S, Nmax, H, F):
    """bench.py's k-th rotated input batch on rank 0: the seeded batch, and
    for k >= 1 its positions and targets offset by 1e-3 * N(0, 1) drawn in
    turn from one device generator seeded 1234."""
    t = make_batch(S, Nmax, H, F=F, seed=1).to_device(gpu)
    gen = torch.Generator(device=gpu)
    gen.manual_seed(1234)
    for _ in range(k):
        dp = 1e-3 * torch.randn(t["pos"].shape, device=gpu, generator=gen)
        dt = 1e-3 * torch.randn(t["targets"].shape, device=gpu, generator=gen)
    if k:
        t["pos"].add_(dp)
        t["targets"].add_(dt)
    return t


# one warm-up step, two timed steps, two rotated batches.  Replayed from the
# graph the timed steps follow the warm-up step (steps 1, 2): the last is
# batch 0; launched from the host they count from 0 (steps 0, 1): batch 1
@pytest.mark.gpu
@pytest.mark.parametrize("extra,batch", [((), 0), (("--no-graph",), 1)], ids=["graph", "host"])
def test_plain_run_dumps_last_step(gpu, tmp_path, capsys, extra, batch):
    """The dump equals, bit for bit, a launch of the same plan on the last
    timed step's input batch; the line's ADE comes from that batch too, and a
    plain run carries none of the --full measurements."""
    S, Nmax, H, F = 8, 32, 128, 20
    rc = bench.main(["--gpus", "1", "--steps", "2", "--warmup", "1", "--scenes", str(S),
                     "--rotate", "2", "--streams", "1", "--dump-outputs", str(tmp_path), *extra])
    assert rc == 0
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(S * F * 2 / (line["ms_per_step"] * 2e-3))
    assert line["roofline"] is None and line["train_mode"] is None and line["cpu_baseline"] is None

    t = _bench_batch(gpu, batch, S, Nmax, H, F)
    params = fs.init_params(Nmax, seed=0, device=gpu)
    out = fs.StepOutputs(pred=torch.zeros(fs.pred_shape(S, F, Nmax, "ped"), device=gpu),
                         h=torch.empty((S, 16, H), device=gpu),
                         metrics=torch.empty((S, 8), device=gpu))
    fs.StepPlan(params, t["pos"], t["vislet"], t["G"], t["targets"], t["n_active"], t["h0"],
                out=out, pred_layout="ped").run()
    torch.cuda.synchronize()
    for k in ("pred", "h", "metrics"):
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype == np.float32
        assert np.array_equal(a, getattr(out, k).cpu().numpy()), k
    m = np.load(tmp_path / "metrics.npy").astype(np.float64).sum(axis=0)
    assert line["ade_fde_all_ranks"]["ADE"] == pytest.approx(m[0] / max(m[1], 1), rel=1e-12)
