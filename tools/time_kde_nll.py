"""Time the fused KDE-NLL evaluation (g2k_kde_nll_f32, g2k_fullcov_kde_nll_f32)
against the composition it replaces — K x the head's sampler, then the kernel
density estimate in torch — and against the same head's best_of_k call on the
same shape (one pass over the K draws where the KDE-NLL makes two).

  python tools/time_kde_nll.py [--calls 200] [--warmup 20] [--k 20]

Shapes: eth_hotel_synth (S 256, Nmax 32) and one rank's share of dense_crowd
(S 128 of 1024 over 8 GPUs, Nmax 256), F 20, synthetic.make_batch; pred = the
targets + N(0, 0.05^2).  Heads: the per-step head at sigma 0.05 and a
full-covariance head with the same marginals and AR(1) 0.7 across the steps.
The three paths run in one process, alternating call by call, each call
between its own pair of device events; the figures are medians, the spread is
the 10th..90th percentile.  Prints one JSON line.  The composition keeps the K
draws in memory (K x S x F x 24 x Nmax floats) and forms the bandwidth in
float64 as the kernel does; torch's temporaries come on top.  Needs a GPU:
there is no fallback.
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

from multimodaltraj_2_amd.fullcov import FullCovHead       # noqa: E402
from multimodaltraj_2_amd.nll import GaussianHead          # noqa: E402
from multimodaltraj_2_amd.synthetic import CONFIGS, FRAMES_PER_SCENE, make_batch   # noqa: E402

SHAPES = {"eth_hotel_synth": dict(S=CONFIGS["eth_hotel_synth"]["S"], Nmax=32),
          "dense_crowd": dict(S=CONFIGS["dense_crowd"]["S"] // 8, Nmax=256)}
SIGMA, AR = 0.05, 0.7


def composed(h, pred, targets, pairs, K, seed, floor):
    """K sampler launches, the draws kept, then the KDE of the definition
    (include/g2k_hip.h) in torch -> [S, 2] {sum kde_nll, sum kde_nll_final}."""
    x = torch.stack([h.sample(pred, seed=seed + k) for k in range(K)])     # [K, S, F, 24, N]
    xs, ys = x[:, :, :, :12], x[:, :, :, 12:]                              # [K, S, F, 12, N]
    tx, ty = targets[..., 0].permute(0, 1, 3, 2), targets[..., 1].permute(0, 1, 3, 2)
    dx, dy = xs - xs.mean(dim=0), ys - ys.mean(dim=0)
    f = K ** (-1.0 / 3.0) / (K - 1)
    hxx, hyy, hxy = ((dx * dx).sum(dim=0).double() * f, (dy * dy).sum(dim=0).double() * f,
                     (dx * dy).sum(dim=0).double() * f)
    det = hxx * hyy - hxy * hxy
    ixx, iyy, ixy = (hyy / det).float(), (hxx / det).float(), (-hxy / det).float()
    cst = (-math.log(K) - math.log(2 * math.pi) - 0.5 * torch.log(det)).float()
    ex, ey = tx - xs, ty - ys
    a = -0.5 * (ixx * ex * ex + 2 * ixy * ex * ey + iyy * ey * ey)
    term = torch.clamp(torch.logsumexp(a, dim=0) + cst, min=floor)         # [S, F, 12, N]
    return torch.stack([(-term.mean(dim=2) * pairs).sum(dim=(1, 2)),
                        (-term[:, :, 11] * pairs).sum(dim=(1, 2))], dim=1)


def quantiles(a):
    return [round(float(np.percentile(a, p)), 2) for p in (10, 50, 90)]


def time_head(h, pred, targets, n_active, pairs, K, calls, warmup, floor):
    seed = 1234

    def fused():
        return h.kde_nll(pred, targets, n_active, K, seed=seed, log_floor=floor).out

    def parent():
        return composed(h, pred, targets, pairs, K, seed, floor)

    def bestk():
        return h.best_of_k(pred, targets, n_active, K, seed=seed, want_per_ped=False).sums

    got, want = fused()[:, :2], parent()
    torch.cuda.synchronize()
    err = float(((got - want).abs() / want.abs().clamp(min=1.0)).max())
    if err > 1e-3:
        raise SystemExit(f"the two paths disagree ({err:.3g})")
    for _ in range(warmup):
        fused(), parent(), bestk()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(6)] for _ in range(calls)]
    for e in ev:                                   # alternating, each call in its own event pair
        e[0].record(); fused(); e[1].record()
        e[2].record(); parent(); e[3].record()
        e[4].record(); bestk(); e[5].record()
    torch.cuda.synchronize()
    tf, tp, tb = (np.array([e[i].elapsed_time(e[i + 1]) for e in ev]) * 1e3 for i in (0, 2, 4))   # us
    qf, qp, qb = quantiles(tf), quantiles(tp), quantiles(tb)
    return dict(fused_us=qf[1], fused_us_p10_p90=[qf[0], qf[2]],
                composed_us=qp[1], composed_us_p10_p90=[qp[0], qp[2]],
                best_of_k_us=qb[1], best_of_k_us_p10_p90=[qb[0], qb[2]],
                composed_over_fused=round(qp[1] / qf[1], 2), fused_over_best_of_k=round(qf[1] / qb[1], 2),
                paths_max_rel_diff=err)


def time_shape(S, Nmax, K, calls, warmup, floor, dev):
    F = FRAMES_PER_SCENE
    b = make_batch(S, Nmax, 64, F=F, seed=5)
    rng = np.random.default_rng(6)
    pred_h = (np.transpose(b.targets, (0, 1, 4, 3, 2)).reshape(S, F, 24, Nmax)
              + SIGMA * rng.standard_normal((S, F, 24, Nmax))).astype(np.float32)
    pred = torch.from_numpy(pred_h).to(dev)
    targets = torch.from_numpy(b.targets).to(dev)
    n_active = torch.from_numpy(b.n_active).to(dev)
    pairs = (torch.arange(Nmax, device=dev)[None, None, :] < n_active[:, None, None]).expand(S, F, Nmax)
    pairs = pairs.to(torch.float32).contiguous()
    gh = GaussianHead(log_sigma=float(np.log(SIGMA)), device=dev)
    T = AR ** np.abs(np.subtract.outer(np.arange(12), np.arange(12)))
    fc = FullCovHead(device=dev)
    fc.chol = torch.from_numpy((SIGMA * np.linalg.cholesky(np.kron(T, np.eye(2)))).astype(np.float32)).to(dev)
    out = dict(S=S, F=F, Nmax=Nmax, K=K, pairs=int(b.n_active.sum()) * F, calls=calls,
               draws_bytes=K * pred.numel() * 4)
    out["per_step"] = time_head(gh, pred, targets, n_active, pairs, K, calls, warmup, floor)
    out["fullcov"] = time_head(fc, pred, targets, n_active, pairs, K, calls, warmup, floor)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--floor", type=float, default=-20.0)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_kde_nll: needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {n: time_shape(SHAPES[n]["S"], SHAPES[n]["Nmax"], a.k, a.calls, a.warmup, a.floor, dev)
           for n in a.shapes}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
