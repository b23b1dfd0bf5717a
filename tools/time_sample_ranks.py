"""Time the fused rank-histogram calibration (g2k_sample_ranks_f32 and its
full-covariance and mixture twins, csrc/g2k_ranks.hip) against the composition
it replaces — K x the head's sampler, a stack of the draws with the target,
then the pooled bandwidths, the (K + 1)^2 kernel terms and 24-D distances and
the comparisons in torch on the device — and next to the same head's
sample_scores call on the same shape and K.

  python tools/time_sample_ranks.py [--calls 30] [--warmup 5] [--repeats 3] [--k 20]

Shapes: eth_hotel_synth (S 256, Nmax 32) and one rank's share of dense_crowd
(S 128 of 1024 over 8 GPUs, Nmax 256), F 20, synthetic.make_batch; pred = the
targets + N(0, 0.05^2).  Heads as tools/time_sample_scores.py: the per-step
head at sigma 0.05, a full-covariance head with the same marginals and AR(1)
0.7 across the steps, and a three-component mixture of that factor with
offsets of one sigma.  The three paths run in one process, alternating call by
call, each call between its own pair of device events, the inputs rotating
over four copies of pred (different noise) so that no call finds the previous
call's lines in the caches; the whole measurement is repeated --repeats times.
The figures are the median over the repeats of each repeat's median; the
spread is the 10th..90th percentile over all calls.  Prints one JSON line,
with the arithmetic bound 12 K (K + 1) exp2 per pair as exp2 per second of the
fused call.  The composition keeps the K draws in memory and walks the K + 1
points one by one (a [K + 1, K + 1, ...] tensor of terms would be K + 1 times
the draws again); its bandwidths are float64, its terms float32.  Needs a GPU:
there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodaltraj_2_amd.fullcov import FullCovHead       # noqa: E402
from multimodaltraj_2_amd.mixture import MixtureHead, OFF_B, OFF_L, PITCH, SLOTS   # noqa: E402
from multimodaltraj_2_amd.nll import GaussianHead          # noqa: E402
from multimodaltraj_2_amd.synthetic import CONFIGS, FRAMES_PER_SCENE, make_batch   # noqa: E402

SHAPES = {"eth_hotel_synth": dict(S=CONFIGS["eth_hotel_synth"]["S"], Nmax=32),
          "dense_crowd": dict(S=CONFIGS["dense_crowd"]["S"] // 8, Nmax=256)}
SIGMA, AR = 0.05, 0.7
ROTATE = 4


def composed(h, pred, targets, pairs, K, seed):
    """K sampler launches, the draws kept, then the definition
    (include/g2k_ranks.h) in torch -> [S, 2]: the sums over the pairs of the 12
    steps' ranks and of the trajectory's rank."""
    y = torch.cat([targets[..., 0].permute(0, 1, 3, 2), targets[..., 1].permute(0, 1, 3, 2)], dim=2)
    z = torch.stack([h.sample(pred, seed=seed + k) for k in range(K)] + [y])       # [K + 1, S, F, 24, N]
    zx, zy = z[:, :, :, :12], z[:, :, :, 12:]
    dx, dy = (zx - zx.mean(dim=0)).double(), (zy - zy.mean(dim=0)).double()
    w = (K + 1) ** (-1.0 / 3.0) / K
    hxx, hyy, hxy = (dx * dx).sum(dim=0) * w, (dy * dy).sum(dim=0) * w, (dx * dy).sum(dim=0) * w
    det = hxx * hyy - hxy * hxy
    a, b, c = (-0.5 * hyy / det).float(), (hxy / det).float(), (-0.5 * hxx / det).float()
    rho = []
    for i in range(K + 1):
        ex, ey = zx[i] - zx, zy[i] - zy
        t = torch.exp(a * ex * ex + b * ex * ey + c * ey * ey)
        t[i] = 0.0                                                                  # without the point itself
        t = t.sum(dim=0)
        r =torch.sqrt((ex * ex + ey * ey).sum(dim=-2)).sum(dim=0)
        rho.append(torch.cat([t, r.unsqueeze(-2)], dim=-2))                         # [S, F, 13, N]
    rho = torch.stack(rho)
    rs = (rho[:K, :, :, :12] > rho[K, :, :, :12]).sum(dim=0).sum(dim=-2)            # [S, F, N]
    rt = (rho[:K, :, :, 12] < rho[K, :, :, 12]).sum(dim=0)
    return torch.stack([(rs * pairs).sum(dim=(1, 2)), (rt * pairs).sum(dim=(1, 2))], dim=1)


def quantiles(a):
    return [round(float(np.percentile(a, p)), 2) for p in (10, 50, 90)]


def time_head(h, preds, targets, n_active, pairs, npairs, K, calls, warmup, repeats):
    seed = 1234

    def fused(p):
        return h.sample_ranks(p, targets, n_active, K, seed=seed).tot

    def parent(p):
        return composed(h, p, targets, pairs, K, seed)

    def scores(p):
        return h.sample_scores(p, targets, n_active, K, seed=seed).out

    got, want = fused(preds[0])[:, 2:].double(), parent(preds[0]).double()
    torch.cuda.synchronize()
    err = float(((got - want).abs().sum(dim=0) / want.sum(dim=0).clamp(min=1.0)).max())
    if err > 1e-3:
        raise SystemExit(f"the two paths disagree ({err:.3g})")
    meds, every = [], [[], [], []]
    for _ in range(repeats):
        for i in range(warmup):
            p = preds[i % ROTATE]
            fused(p), parent(p), scores(p)
        torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(6)] for _ in range(calls)]
        for i, e in enumerate(ev):                 # alternating, each call in its own event pair
            p = preds[i % ROTATE]
            e[0].record(); fused(p); e[1].record()
            e[2].record(); parent(p); e[3].record()
            e[4].record(); scores(p); e[5].record()
        torch.cuda.synchronize()
        ts = [np.array([e[i].elapsed_time(e[i + 1]) for e in ev]) * 1e3 for i in (0, 2, 4)]   # us
        meds.append([float(np.median(t)) for t in ts])
        for acc, t in zip(every, ts):
            acc.extend(t.tolist())
    mf, mp, ms = (round(float(np.median([m[i] for m in meds])), 2) for i in range(3))
    qf, qp, qs = (quantiles(a) for a in every)
    return dict(fused_us=mf, fused_us_p10_p90=[qf[0], qf[2]], fused_us_repeats=[round(m[0], 2) for m in meds],
                composed_us=mp, composed_us_p10_p90=[qp[0], qp[2]],
                composed_us_repeats=[round(m[1], 2) for m in meds],
                sample_scores_us=ms, sample_scores_us_p10_p90=[qs[0], qs[2]],
                composed_over_fused=round(mp / mf, 2), fused_over_sample_scores=round(mf / ms, 2),
                exp2_per_s=round(12.0 * K * (K + 1) * npairs / (mf * 1e-6), 0),
                rank_sums_max_rel_diff=err)


def time_shape(S, Nmax, K, calls, warmup, repeats, dev, heads):
    F = FRAMES_PER_SCENE
    b = make_batch(S, Nmax, 64, F=F, seed=5)
    rng = np.random.default_rng(6)
    base = np.transpose(b.targets, (0, 1, 4, 3, 2)).reshape(S, F, 24, Nmax)
    preds = [torch.from_numpy((base + SIGMA * rng.standard_normal((S, F, 24, Nmax))).astype(np.float32)).to(dev)
             for _ in range(ROTATE)]
    targets = torch.from_numpy(b.targets).to(dev)
    n_active = torch.from_numpy(b.n_active).to(dev)
    pairs = (torch.arange(Nmax, device=dev)[None, None, :] < n_active[:, None, None]).expand(S, F, Nmax)
    pairs = pairs.to(torch.int64).contiguous()
    gh = GaussianHead(log_sigma=float(np.log(SIGMA)), device=dev)
    T = AR ** np.abs(np.subtract.outer(np.arange(12), np.arange(12)))
    chol = (SIGMA * np.linalg.cholesky(np.kron(T, np.eye(2)))).astype(np.float32)
    fc = FullCovHead(device=dev)
    fc.chol = torch.from_numpy(chol).to(dev)
    block = np.zeros((SLOTS, PITCH), np.float32)
    for m, w in ((0, 0.5), (2, 0.3), (5, 0.2)):
        block[m, 0] = w
        block[m, OFF_B:OFF_L] = SIGMA * rng.standard_normal(24)
        block[m, OFF_L:] = chol.reshape(-1)
    mx = MixtureHead.from_block(block, device=dev)
    npairs = int(b.n_active.sum()) * F
    out = dict(S=S, F=F, Nmax=Nmax, K=K, pairs=npairs, calls=calls, repeats=repeats,
               draws_bytes=K * preds[0].numel() * 4)
    for name, h in (("per_step", gh), ("fullcov", fc), ("mix", mx)):
        if name in heads:
            out[name] = time_head(h, preds, targets, n_active, pairs, npairs, K, calls, warmup, repeats)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--heads", nargs="*", default=["per_step", "fullcov", "mix"])
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_sample_ranks: needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {n: time_shape(SHAPES[n]["S"], SHAPES[n]["Nmax"], a.k, a.calls, a.warmup, a.repeats, dev, a.heads)
           for n in a.shapes}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
