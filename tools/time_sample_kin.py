"""Time the fused kinematic scores (g2k_sample_kin_f32 and its full-covariance
and mixture twins, csrc/g2k_kin.hip) against the composition it replaces — K x
the head's sampler, a stack of the draws, then the 32 features of the draws and
of the target, the ranks and the three sums m, p, d per group in torch on the
device — and next to the same head's sample_scores call on the same shape and
K.

  python tools/time_sample_kin.py [--calls 30] [--warmup 5] [--repeats 3] [--k 20]

Shapes, heads and method are tools/time_sample_ranks.py's: eth_hotel_synth (S
256, Nmax 32) and one rank's share of dense_crowd (S 128 of 1024 over 8 GPUs,
Nmax 256), F 20, synthetic.make_batch; pred = the targets + N(0, 0.05^2); the
per-step head at sigma 0.05, a full-covariance head with the same marginals and
AR(1) 0.7 across the steps, a three-component mixture of that factor with
offsets of one sigma.  The three paths run in one process, alternating call by
call, each call between its own pair of device events, the inputs rotating over
four copies of pred (different noise); the whole measurement is repeated
--repeats times.  The figures are the median over the repeats of each repeat's
median; the spread is the 10th..90th percentile over all calls.  Prints one JSON
line.  The composition keeps the K draws' features in memory and walks the
couples draw by draw (a [K, K, ...] tensor of differences would be K times the
features again).  Needs a GPU: there is no fallback.
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
GROUPS = (slice(0, 11), slice(11, 21), slice(21, 31), slice(31, 32))


def features(z):
    """z [..., 24, N] (band layout) -> the 32 features [..., 32, N]
    (include/g2k_kin.h), float32."""
    x, y = z[..., :12, :], z[..., 12:, :]
    vx, vy = x[..., 1:, :] - x[..., :-1, :], y[..., 1:, :] - y[..., :-1, :]
    s = torch.sqrt(vx * vx + vy * vy)
    wx, wy = vx[..., 1:, :] - vx[..., :-1, :], vy[..., 1:, :] - vy[..., :-1, :]
    a = torch.sqrt(wx * wx + wy * wy)
    la = s[..., 1:, :] - s[..., :-1, :]
    ex, ey = x[..., 11:, :] - x[..., :1, :], y[..., 11:, :] - y[..., :1, :]
    length = s.sum(dim=-2, keepdim=True)
    st = torch.where(length == 0, torch.ones_like(length), torch.sqrt(ex * ex + ey * ey) / length)
    return torch.cat([s, a, la, st], dim=-2)


def composed(h, pred, targets, pairs, K, seed):
    """K sampler launches, the draws kept, then the definition in torch -> [S,
    16]: per group the sums over the pairs of the ranks, of m, of p and of d
    (unscaled)."""
    y = torch.cat([targets[..., 0].permute(0, 1, 3, 2), targets[..., 1].permute(0, 1, 3, 2)], dim=2)
    fx = features(torch.stack([h.sample(pred, seed=seed + k) for k in range(K)]))   # [K, S, F, 32, N]
    fy = features(y)
    r = (fx < fy).sum(dim=0).to(torch.float32)
    m = (fx - fy).abs().sum(dim=0)
    d = fx.sum(dim=0)
    p = torch.zeros_like(fy)
    for k in range(K - 1):
        p += (fx[k + 1:] - fx[k]).abs().sum(dim=0)
    w = pairs.unsqueeze(-2).to(torch.float32)                                       # [S, F, 1, N]
    out = [torch.nan_to_num(v * w)[:, :, g].sum(dim=(1, 2, 3)) for v in (r, m, p, d) for g in GROUPS]
    return torch.stack(out, dim=1)


def quantiles(a):
    return [round(float(np.percentile(a, p)), 2) for p in (10, 50, 90)]


def time_head(h, preds, targets, n_active, pairs, npairs, K, calls, warmup, repeats):
    seed = 1234

    def fused(p):
        return h.sample_kin(p, targets, n_active, K, seed=seed)

    def parent(p):
        return composed(h, p, targets, pairs, K, seed)

    def scores(p):
        return h.sample_scores(p, targets, n_active, K, seed=seed).out

    f0, want = fused(preds[0]), parent(preds[0]).double()
    torch.cuda.synchronize()
    n = torch.tensor([11.0, 10.0, 10.0, 1.0], dtype=torch.float64, device=want.device)
    got = torch.cat([f0.tot[:, 1:5].double(), f0.sums[:, 0:4].double() * (K * n),
                     f0.sums[:, 4:8].double() * (K * (K - 1) / 2.0 * n), f0.sums[:, 8:12].double() * (K * n)], dim=1)
    err = float(((got - want).abs().sum(dim=0) / want.abs().sum(dim=0).clamp(min=1.0)).max())
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
                pairs_per_s=round(npairs / (mf * 1e-6), 0), sums_max_rel_diff=err)


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
    pairs = pairs.contiguous()
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
        raise SystemExit("time_sample_kin: needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {n: time_shape(SHAPES[n]["S"], SHAPES[n]["Nmax"], a.k, a.calls, a.warmup, a.repeats, dev, a.heads)
           for n in a.shapes}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
