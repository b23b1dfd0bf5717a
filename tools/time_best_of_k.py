"""Time the fused best-of-K evaluation (g2k_best_of_k_f32) against the
composition it replaces: K x GaussianHead.sample, then the errors and a
running minimum in torch.

  python tools/time_best_of_k.py [--calls 200] [--warmup 20] [--k 20]

Shapes: eth_hotel_synth (S 256, Nmax 32) and one rank's share of dense_crowd
(S 128 of 1024 over 8 GPUs, Nmax 256), F 20, synthetic.make_batch; pred =
the targets + N(0, 0.05^2), head sigma 0.05.  Both paths run in one process,
alternating call by call, each call between its own pair of device events;
the figures are medians, the spread is the 10th..90th percentile.  Prints one
JSON line.  Bytes are computed from the shapes: the fused call reads pred and
targets once and writes per_ped; the composition moves at least K x (sampler:
read pred, write the draw; errors: read the draw and the targets) — torch's
temporaries come on top, so its figure is a lower bound.  Needs a GPU: there
is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodaltraj_2_amd.nll import GaussianHead          # noqa: E402
from multimodaltraj_2_amd.synthetic import CONFIGS, FRAMES_PER_SCENE, make_batch   # noqa: E402

SHAPES = {"eth_hotel_synth": dict(S=CONFIGS["eth_hotel_synth"]["S"], Nmax=32),
          "dense_crowd": dict(S=CONFIGS["dense_crowd"]["S"] // 8, Nmax=256)}


def unfused(gh, pred, targets, pairs, K, seed):
    """The parent composition: K sampler launches, each followed by the
    errors of its draw and a running minimum; then the scene sums."""
    S, F, _, N = pred.shape
    mn_a = mn_f = None
    for k in range(K):
        x = gh.sample(pred, seed=seed + k)
        d = torch.linalg.vector_norm(x.view(S, F, 2, 12, N).permute(0, 1, 4, 3, 2) - targets, dim=-1)
        a, f = d.mean(dim=-1), d[..., 11]
        mn_a = a if mn_a is None else torch.minimum(mn_a, a)
        mn_f = f if mn_f is None else torch.minimum(mn_f, f)
    return torch.stack([(mn_a * pairs).sum(dim=(1, 2)), (mn_f * pairs).sum(dim=(1, 2))], dim=1)


def time_shape(name, S, Nmax, K, calls, warmup, dev):
    F = FRAMES_PER_SCENE
    b = make_batch(S, Nmax, 64, F=F, seed=5)
    rng = np.random.default_rng(6)
    pred_h = (np.transpose(b.targets, (0, 1, 4, 3, 2)).reshape(S, F, 24, Nmax)
              + 0.05 * rng.standard_normal((S, F, 24, Nmax))).astype(np.float32)
    pred = torch.from_numpy(pred_h).to(dev)
    targets = torch.from_numpy(b.targets).to(dev)
    n_active = torch.from_numpy(b.n_active).to(dev)
    pairs = (torch.arange(Nmax, device=dev)[None, None, :] < n_active[:, None, None]).expand(S, F, Nmax)
    pairs = pairs.to(torch.float32).contiguous()
    gh = GaussianHead(log_sigma=float(np.log(0.05)), device=dev)
    seed = 1234

    def fused():
        return gh.best_of_k(pred, targets, n_active, K, seed=seed).sums

    def parent():
        return unfused(gh, pred, targets, pairs, K, seed)

    got, want = fused()[:, :2], parent()
    torch.cuda.synchronize()
    err = float(((got - want).abs() / want.abs().clamp(min=1.0)).max())
    if err > 1e-4:
        raise SystemExit(f"{name}: the two paths disagree ({err:.3g})")
    for _ in range(warmup):
        fused()
        parent()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(calls)]
    for e in ev:                                   # alternating, each call in its own event pair
        e[0].record(); fused(); e[1].record()
        e[2].record(); parent(); e[3].record()
    torch.cuda.synchronize()
    tf = np.array([e[0].elapsed_time(e[1]) for e in ev]) * 1e3      # us
    tp = np.array([e[2].elapsed_time(e[3]) for e in ev]) * 1e3
    n_pairs = int(b.n_active.sum()) * F
    pred_b, tgt_b = pred.numel() * 4, targets.numel() * 4
    q = lambda a: [round(float(np.percentile(a, p)), 2) for p in (10, 50, 90)]   # noqa: E731
    return dict(S=S, F=F, Nmax=Nmax, K=K, pairs=n_pairs, calls=calls,
                fused_us=q(tf)[1], fused_us_p10_p90=[q(tf)[0], q(tf)[2]],
                unfused_us=q(tp)[1], unfused_us_p10_p90=[q(tp)[0], q(tp)[2]],
                ratio=round(float(np.median(tp) / np.median(tf)), 2),
                draws_per_s=round(n_pairs * K * 12 / (float(np.median(tf)) * 1e-6), 0),
                fused_bytes=pred_b + tgt_b + S * F * Nmax * 16,
                unfused_bytes_at_least=K * (3 * pred_b + tgt_b), paths_max_rel_diff=err)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_best_of_k: needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {n: time_shape(n, SHAPES[n]["S"], SHAPES[n]["Nmax"], a.k, a.calls, a.warmup, dev)
           for n in a.shapes}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
