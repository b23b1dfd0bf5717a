"""Time the fused head calibration (g2k_head_stats_f32) against the same
figures composed in torch: residuals, moments, q, nll and one comparison per
level, all in float64.

  python tools/time_head_stats.py [--calls 200] [--warmup 20]

Shapes: eth_hotel_synth (S 256, Nmax 32) and one rank's share of dense_crowd
(S 128 of 1024 over 8 GPUs, Nmax 256), F 20, synthetic.make_batch; pred =
the targets + an anisotropic N(0, .) residual, head sigma of that size, the
levels 0.1 .. 0.9, 0.95, 0.99.  Both paths run in one process, alternating
call by call, each call between its own pair of device events; the figures
are medians, the spread is the 10th..90th percentile.  Prints one JSON line.
Bytes are computed from the shapes: the fused call reads pred and targets
once (its outputs are 2 KiB); torch's temporaries come on top of that, so the
GB/s figure is given for the fused call only.  Needs a GPU: there is no
fallback.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodaltraj_2_amd.nll import DEFAULT_LEVELS, GaussianHead          # noqa: E402
from multimodaltraj_2_amd.synthetic import CONFIGS, FRAMES_PER_SCENE, make_batch   # noqa: E402

SHAPES = {"eth_hotel_synth": dict(S=CONFIGS["eth_hotel_synth"]["S"], Nmax=32),
          "dense_crowd": dict(S=CONFIGS["dense_crowd"]["S"] // 8, Nmax=256)}


def composed(head, pred, targets, pairs, r2):
    """The same figures in torch, float64: -> (stats [12, 8], inside [12, NL])."""
    S, F, _, N = pred.shape
    h = head.double()
    sx, sy, rho = torch.exp(h[0]), torch.exp(h[1]), torch.tanh(h[2])
    c = 1.0 - rho * rho
    p = pred.view(S, F, 2, 12, N).permute(0, 1, 4, 3, 2).double()      # [S, F, N, 12, 2]
    d = (targets.double() - p) * pairs[..., None, None]
    dx, dy = d[..., 0], d[..., 1]                                      # [S, F, N, 12]
    a, b = dx / sx, dy / sy
    q = (a * a + b * b - 2 * rho * a * b) / c
    nll = (math.log(2 * math.pi) + h[0] + h[1] + 0.5 * torch.log(c) + q / 2) * pairs[..., None]
    n = pairs.sum().expand(12)
    cols = [n] + [v.sum(dim=(0, 1, 2)) for v in (dx, dy, dx * dx, dy * dy, dx * dy, nll, q)]
    on = pairs[..., None] > 0
    inside = torch.stack([((q <= r) & on).sum(dim=(0, 1, 2)) for r in r2.unbind()], dim=1)
    return torch.stack(cols, dim=1), inside


def time_shape(name, S, Nmax, calls, warmup, dev):
    F = FRAMES_PER_SCENE
    b = make_batch(S, Nmax, 64, F=F, seed=5)
    rng = np.random.default_rng(6)
    e = rng.standard_normal((2, S, F, 12, Nmax))
    res = np.concatenate([0.3 * e[0], 0.15 * (0.6 * e[0] + 0.8 * e[1])], axis=2)
    pred_h = (np.transpose(b.targets, (0, 1, 4, 3, 2)).reshape(S, F, 24, Nmax) + res).astype(np.float32)
    pred = torch.from_numpy(pred_h).to(dev)
    targets = torch.from_numpy(b.targets).to(dev)
    n_active = torch.from_numpy(b.n_active).to(dev)
    pairs = (torch.arange(Nmax, device=dev)[None, None, :] < n_active[:, None, None]).expand(S, F, Nmax)
    pairs = pairs.to(torch.float64).contiguous()
    gh = GaussianHead(device=dev)
    gh.head[0], gh.head[1], gh.head[2] = math.log(0.3), math.log(0.2), 0.3
    r2 = gh._r2(tuple(DEFAULT_LEVELS), dev)

    def fused():
        r = gh.stats(pred, targets, n_active, DEFAULT_LEVELS)
        return r.stats, r.inside

    def parent():
        return composed(gh.head, pred, targets, pairs, r2)

    (gs, gi), (ws, wi) = fused(), parent()
    torch.cuda.synchronize()
    err = float(((gs - ws).abs() / ws.abs().clamp(min=1.0)).max())
    if err > 1e-9 or not torch.equal(gi, wi):
        raise SystemExit(f"{name}: the two paths disagree ({err:.3g}, counts "
                         f"{int((gi - wi).abs().max())})")
    for _ in range(warmup):
        fused()
        parent()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(calls)]
    for v in ev:                                   # alternating, each call in its own event pair
        v[0].record(); fused(); v[1].record()
        v[2].record(); parent(); v[3].record()
    torch.cuda.synchronize()
    tf = np.array([v[0].elapsed_time(v[1]) for v in ev]) * 1e3      # us
    tp = np.array([v[2].elapsed_time(v[3]) for v in ev]) * 1e3
    n_pairs = int(b.n_active.sum()) * F
    nbytes = pred.numel() * 4 + targets.numel() * 4
    q = lambda a: [round(float(np.percentile(a, p)), 2) for p in (10, 50, 90)]   # noqa: E731
    return dict(S=S, F=F, Nmax=Nmax, levels=len(DEFAULT_LEVELS), pairs=n_pairs, calls=calls,
                fused_us=q(tf)[1], fused_us_p10_p90=[q(tf)[0], q(tf)[2]],
                torch_us=q(tp)[1], torch_us_p10_p90=[q(tp)[0], q(tp)[2]],
                ratio=round(float(np.median(tp) / np.median(tf)), 2),
                fused_bytes=nbytes,
                fused_gb_per_s=round(nbytes / (float(np.median(tf)) * 1e-6) / 1e9, 1),
                paths_max_rel_diff=err)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_head_stats: needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {n: time_shape(n, SHAPES[n]["S"], SHAPES[n]["Nmax"], a.calls, a.warmup, dev)
           for n in a.shapes}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
