"""Time the fused k-means reduction of the heads' samples (g2k_sample_modes_f32
and its full-covariance and mixture twins, csrc/g2k_modes.hip) against the
composition it replaces — K x the head's sampler, a stack of the draws, then
the same Lloyd loop batched over the pairs in torch float64 on the device —
and next to the same head's sample_scores call at the same K.

  python tools/time_sample_modes.py [--calls 10] [--composed_calls 3] [--warmup 2] [--repeats 3]

Shapes: eth_hotel_synth (S 256, Nmax 32) and one rank's share of dense_crowd
(S 128 of 1024 over 8 GPUs, Nmax 256), F 20, synthetic.make_batch; pred = the
targets + N(0, 0.05^2).  Parameters: K 256, M 20, 10 iterations, and K 64, M 5.
Heads: the per-step head at sigma 0.05, a full-covariance head with the same
marginals and AR(1) 0.7 across the steps, and a three-component mixture of
that factor with offsets of one sigma.  The paths run in one process,
alternating call by call, each call between its own pair of device events, the
inputs rotating over four copies of pred (different noise); the composition,
which is seconds long, is timed over --composed_calls calls of each repeat.
The figures are the median over the repeats of each repeat's median; the spread
is the 10th..90th percentile over all calls.  Prints one JSON line.

The composition keeps the K draws in memory (K x S x F x 24 x Nmax floats: 4 GB
and 16 GB at K 256) and walks the scenes in chunks sized so that the [pairs, K,
M, 24] float64 differences of an assignment stay below --chunk_bytes; the
assignment is the exact sum of squared differences, as the kernel's (the
matrix-product form of the distance would flip near-ties).  Needs a GPU: there
is no fallback."""
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
PARAMS = {"k256_m20": dict(K=256, M=20, iters=10), "k64_m5": dict(K=64, M=5, iters=10)}
SIGMA, AR = 0.05, 0.7
ROTATE = 4


def lloyd(x, y, M, iters):
    """x [P, K, 24] float64 (band order: the 12 x, then the 12 y), y [P, 24]
    -> [P, 8] {cA, cF, (1 - w_mA)^2, (1 - w_mF)^2, cF, inertia, live, 1}: the
    definition (include/g2k_modes.h) batched over the pairs."""
    P, K, _ = x.shape
    c = x[:, :M].clone()
    for it in range(iters + 1):
        d2 = ((x[:, :, None, :] - c[:, None, :, :]) ** 2).sum(dim=-1)      # [P, K, M]
        best, a = d2.min(dim=-1)
        hot = torch.nn.functional.one_hot(a, M).to(x.dtype)                # [P, K, M]
        n = hot.sum(dim=1)                                                 # [P, M]
        if it == iters:
            break
        sums = hot.transpose(1, 2) @ x                                     # [P, M, 24]
        c = torch.where(n[..., None] > 0, sums / n.clamp(min=1)[..., None], c)
    d = c - y[:, None, :]
    dist = torch.sqrt(d[..., :12] ** 2 + d[..., 12:] ** 2)                 # [P, M, 12]
    cA, mA = dist.mean(dim=-1).min(dim=-1)
    cF, mF = dist[..., 11].min(dim=-1)
    w = n / K
    wA, wF = w.gather(1, mA[:, None])[:, 0], w.gather(1, mF[:, None])[:, 0]
    return torch.stack([cA, cF, (1 - wA) ** 2, (1 - wF) ** 2, cF, best.sum(dim=-1) / K,
                        (n > 0).sum(dim=-1).to(x.dtype), torch.ones_like(cA)], dim=1)


def composed(h, pred, targets, pairs, K, M, iters, radius, seed, chunk_bytes):
    """K sampler launches, the draws kept, then ``lloyd`` scene chunk by scene
    chunk -> [S, 8] float64 sums over the pairs (column 4: cF > radius)."""
    x = torch.stack([h.sample(pred, seed=seed + k) for k in range(K)])     # [K, S, F, 24, N]
    S, F, N = pairs.shape
    y = torch.cat([targets[..., 0].permute(0, 1, 3, 2), targets[..., 1].permute(0, 1, 3, 2)], dim=2)
    out = torch.zeros((S, 8), dtype=torch.float64, device=pred.device)
    per_scene = max(1, F * N * K * M * 24 * 8)
    step = max(1, int(chunk_bytes // per_scene))
    for s0 in range(0, S, step):
        m = pairs[s0:s0 + step]                                            # [Sc, F, N] bool
        xs = x[:, s0:s0 + step].permute(1, 2, 4, 0, 3)[m].double()         # [P, K, 24]
        ys = y[s0:s0 + step].permute(0, 1, 3, 2)[m].double()               # [P, 24]
        r = lloyd(xs, ys, M, iters)
        r[:, 4] = (r[:, 4] > radius).to(r.dtype)
        sid = torch.arange(s0, s0 + m.shape[0], device=pred.device)[:, None, None].expand_as(m)[m]
        out.index_add_(0, sid, r)
    return out


def quantiles(a):
    return [round(float(np.percentile(a, p)), 2) for p in (10, 50, 90)]


def time_head(h, preds, targets, n_active, pairs, prm, calls, composed_calls, warmup, repeats,
              chunk_bytes):
    seed, radius = 1234, 0.05
    K, M, iters = prm["K"], prm["M"], prm["iters"]

    def fused(p):
        return h.sample_modes(p, targets, n_active, K, M, iters, seed=seed, miss_radius=radius,
                              want_per_ped=False).out

    def parent(p):
        return composed(h, p, targets, pairs, K, M, iters, radius, seed, chunk_bytes)

    def scores(p):
        return h.sample_scores(p, targets, n_active, K, seed=seed).out

    got, want = fused(preds[0]).double(), parent(preds[0])
    torch.cuda.synchronize()
    err = float(((got - want).abs() / want.abs().clamp(min=1.0)).max())
    if err > 1e-3:
        raise SystemExit(f"the two paths disagree ({err:.3g})")
    meds, every = [], [[], [], []]
    for _ in range(repeats):
        for i in range(warmup):
            p = preds[i % ROTATE]
            fused(p), scores(p)
        parent(preds[0])
        torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(6)] for _ in range(calls)]
        for i, e in enumerate(ev):                 # alternating, each call in its own event pair
            p = preds[i % ROTATE]
            e[0].record(); fused(p); e[1].record()
            e[2].record(); scores(p); e[3].record()
            if i < composed_calls:
                e[4].record(); parent(p); e[5].record()
        torch.cuda.synchronize()
        ts = [np.array([e[i].elapsed_time(e[i + 1]) for e in ev[:n]]) * 1e3                 # us
              for i, n in ((0, calls), (2, calls), (4, composed_calls))]
        meds.append([float(np.median(t)) for t in ts])
        for acc, t in zip(every, ts):
            acc.extend(t.tolist())
    mf, ms, mp = (round(float(np.median([m[i] for m in meds])), 2) for i in range(3))
    qf, qs, qp = (quantiles(a) for a in every)
    return dict(fused_us=mf, fused_us_p10_p90=[qf[0], qf[2]], fused_us_repeats=[round(m[0], 2) for m in meds],
                composed_us=mp, composed_us_p10_p90=[qp[0], qp[2]],
                composed_us_repeats=[round(m[2], 2) for m in meds],
                sample_scores_us=ms, sample_scores_us_p10_p90=[qs[0], qs[2]],
                composed_over_fused=round(mp / mf, 2), fused_over_sample_scores=round(mf / ms, 2),
                paths_max_rel_diff=err)


def time_shape(S, Nmax, a, dev):
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
    out = dict(S=S, F=F, Nmax=Nmax, pairs=int(b.n_active.sum()) * F, calls=a.calls,
               composed_calls=a.composed_calls, repeats=a.repeats)
    for pname in a.params:
        prm = PARAMS[pname]
        out[pname] = dict(prm, draws_bytes=prm["K"] * preds[0].numel() * 4)
        for name, h in (("per_step", gh), ("fullcov", fc), ("mix", mx)):
            if name in a.heads:
                out[pname][name] = time_head(h, preds, targets, n_active, pairs, prm, a.calls,
                                             a.composed_calls, a.warmup, a.repeats, a.chunk_bytes)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--composed_calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk_bytes", type=float, default=2.0 * 2 ** 30)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--params", nargs="*", default=list(PARAMS))
    ap.add_argument("--heads", nargs="*", default=["per_step", "fullcov", "mix"])
    a = ap.parse_args(argv)
    a.composed_calls = min(a.composed_calls, a.calls)
    if not torch.cuda.is_available():
        raise SystemExit("time_sample_modes: needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {n: time_shape(SHAPES[n]["S"], SHAPES[n]["Nmax"], a, dev) for n in a.shapes}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
