"""Time the fused couple-distance scores (g2k_couple_scores_f32 and its
fullcov_ / mix_ twins, csrc/g2k_couples.hip) against the composition they
replace — K sampler launches, the all-against-all distances of every draw, the
ranks, the roots and the two CRPS terms in torch — and next to the same head's
joint_eval call (g2k_joint_eval_f32: the same draws, paired for one threshold).

  python tools/time_couple_scores.py [--calls 100] [--warmup 5] [--k 20] [--head per_step]

Shapes: the real-data evaluation's (F 1, S 384 scenes, Nmax 32, n_active 2..32)
and dense_crowd's (S 64, F 20, Nmax 256), synthetic.make_batch; pred = the
targets + N(0, 0.05^2), head sigma 0.05 (the full-covariance head: the same
marginals, AR(1) 0.7 over the steps; the mixture head: that factor in three
components).  The composition materialises [K, s, F, 12, Nmax, Nmax] distances,
so it runs over chunks of scenes sized to about 1 GiB per temporary.  The three
paths run in one process, alternating call by call, each call between its own
pair of device events; the figures are medians, the spread is the 10th..90th
percentile.  Before timing the fused call and the composition must agree: the
scored couples and the rank sums exactly (torch forms dx dx + dy dy in three
kernels, one rounding each, as the definition has it), the float sums to 1e-4.
Prints one JSON line.  Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodaltraj_2_amd import couples as cp                # noqa: E402
from multimodaltraj_2_amd.fullcov import FullCovHead          # noqa: E402
from multimodaltraj_2_amd.mixture import MixtureHead          # noqa: E402
from multimodaltraj_2_amd.nll import GaussianHead             # noqa: E402
from multimodaltraj_2_amd.synthetic import make_batch         # noqa: E402

SHAPES = {"realdata_eval": dict(S=384, F=1, Nmax=32),
          "dense_crowd": dict(S=64, F=20, Nmax=256)}
CHUNK_BYTES = 1 << 30
SIGMA = 0.05


def make_head(which, dev):
    if which == "per_step":
        return GaussianHead(log_sigma=float(np.log(SIGMA)), device=dev)
    T = 0.7 ** np.abs(np.subtract.outer(np.arange(12), np.arange(12)))
    chol = np.linalg.cholesky(SIGMA * SIGMA * np.kron(T, np.eye(2))).astype(np.float32)
    if which == "fullcov":
        h = FullCovHead(device=dev)
        h.chol = torch.from_numpy(chol).to(dev)
        return h
    block = np.zeros((8, 608), np.float32)
    for m, (w, shift) in enumerate(((0.5, 0.0), (0.3, 0.03), (0.2, -0.03))):
        block[m, 0] = w
        block[m, 8:32] = shift
        block[m, 32:] = chol.reshape(-1)
    return MixtureHead.from_block(block, device=dev)


def _features(x):
    """x [..., 2, 12, N] -> (qmin, qfin) [..., N, N]."""
    dx = x[..., 0, :, :, None] - x[..., 0, :, None, :]
    dy = x[..., 1, :, :, None] - x[..., 1, :, None, :]
    q = dx * dx + dy * dy
    return q.amin(dim=-3), q[..., 11, :, :]


def unfused(head, pred, targets, couples, K, B, seed):
    """K sampler launches, then per chunk of scenes the features of every draw,
    of the targets and of the mean, the ranks, the roots and the CRPS terms.
    -> (sums [S, 8], hist [S, 2, B], tot [S, 3])."""
    S, F, _, N = pred.shape
    dev = pred.device
    draws = torch.stack([head.sample(pred, seed=seed + k) for k in range(K)]).view(K, S, F, 2, 12, N)
    ty = targets.permute(0, 1, 4, 3, 2)                                # [S, F, 2, 12, N]
    sc = int(max(1, min(S, CHUNK_BYTES // max(1, K * F * N * N * 4))))
    coef = (2.0 * torch.arange(K, device=dev, dtype=torch.float32) - (K - 1)).view(K, 1, 1, 1, 1)
    sums = torch.zeros((S, 8), device=dev)
    hist = torch.zeros((S, 2, B), dtype=torch.int64, device=dev)
    tot = torch.zeros((S, 3), dtype=torch.int64, device=dev)
    for s0 in range(0, S, sc):
        sl = slice(s0, min(S, s0 + sc))
        qx = [torch.stack(v) for v in zip(*[_features(draws[k, sl]) for k in range(K)])]   # 2 x [K, s, F, N, N]
        qy = _features(ty[sl])
        on = couples[sl]                                               # every couple: reach = +inf
        w = on.to(torch.float32)
        tot[sl, 0] = on.sum(dim=(1, 2, 3))
        for g in range(2):
            r = (qx[g] < qy[g]).sum(dim=0)
            sx, sy = qx[g].sqrt(), qy[g].sqrt()
            m = (sx - sy).abs().mean(dim=0)
            p = (coef * sx.sort(dim=0).values).sum(dim=0) * (2.0 / (K * (K - 1)))
            d = sx.mean(dim=0)
            for j, v in ((g, m), (2 + g, p), (4 + g, d), (6 + g, sy)):
                sums[sl, j] = (v * w).sum(dim=(1, 2, 3))
            tot[sl, 1 + g] = (r * on).sum(dim=(1, 2, 3))
            hist[sl, g].scatter_add_(1, (r * B // (K + 1)).flatten(1), on.flatten(1).to(torch.int64))
    return sums, hist, tot


def time_shape(name, which, S, F, Nmax, K, calls, warmup, dev):
    b = make_batch(S, Nmax, 64, F=F, seed=5)
    rng = np.random.default_rng(6)
    pred_h = (np.transpose(b.targets, (0, 1, 4, 3, 2)).reshape(S, F, 24, Nmax)
              + SIGMA * rng.standard_normal((S, F, 24, Nmax))).astype(np.float32)
    pred = torch.from_numpy(pred_h).to(dev)
    targets = torch.from_numpy(b.targets).to(dev)
    n_active = torch.from_numpy(b.n_active).to(dev)
    mem = (torch.arange(Nmax, device=dev)[None, None, :] < n_active[:, None, None]).expand(S, F, Nmax)
    couples = (mem[:, :, :, None] & mem[:, :, None, :]
               & torch.ones((Nmax, Nmax), dtype=torch.bool, device=dev).triu(1)).contiguous()
    head = make_head(which, dev)
    B = cp.auto_bins(K)
    seed = 1234

    def fused():
        return head.couple_scores(pred, targets, n_active, K, B, seed=seed)

    def joint():
        return head.joint_eval(pred, targets, n_active, K, SIGMA, seed=seed, want_per_frame=False)

    def parent():
        return unfused(head, pred, targets, couples, K, B, seed)

    got, want = fused(), parent()
    torch.cuda.synchronize()
    err = float(((got.sums - want[0]).abs() / want[0].abs().clamp(min=1.0)
                 / got.tot[:, :1].clamp(min=1).to(torch.float32)).max())
    same = torch.equal(got.tot[:, :3], want[2]) and torch.equal(got.hist.to(torch.int64), want[1])
    if err > 1e-4 or not same:
        raise SystemExit(f"{name}: the two paths disagree (sums {err:.3g} a couple, counts equal: {same})")
    for _ in range(warmup):
        fused()
        joint()
        parent()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(6)] for _ in range(calls)]
    for e in ev:                                   # alternating, each call in its own event pair
        e[0].record(); fused(); e[1].record()
        e[2].record(); joint(); e[3].record()
        e[4].record(); parent(); e[5].record()
    torch.cuda.synchronize()
    tf, tj, tp = (np.array([e[i].elapsed_time(e[i + 1]) for e in ev]) * 1e3 for i in (0, 2, 4))   # us
    q = lambda a: [round(float(np.percentile(a, p)), 2) for p in (10, 50, 90)]   # noqa: E731
    n = got.couples
    return dict(S=S, F=F, Nmax=Nmax, K=K, B=B, head=which, couples=n, calls=calls,
                geometry=cp.couple_scores_geometry(S, F, Nmax, K),
                fused_us=q(tf)[1], fused_us_p10_p90=[q(tf)[0], q(tf)[2]],
                unfused_us=q(tp)[1], unfused_us_p10_p90=[q(tp)[0], q(tp)[2]],
                joint_eval_us=q(tj)[1], joint_eval_us_p10_p90=[q(tj)[0], q(tj)[2]],
                ratio=round(float(np.median(tp) / np.median(tf)), 2),
                over_joint_eval=round(float(np.median(tf) / np.median(tj)), 2),
                couple_steps_per_s=round(n * (K + 2) * 12 / (float(np.median(tf)) * 1e-6), 0),
                crps_min=got.crps("min"), crps_fin=got.crps("fin"), dev_min=got.dev("min"),
                dev_fin=got.dev("fin"), paths_max_rel_diff=err)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--head", choices=("per_step", "fullcov", "mix"), default="per_step")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_couple_scores: needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {n: time_shape(n, a.head, SHAPES[n]["S"], SHAPES[n]["F"], SHAPES[n]["Nmax"], a.k, a.calls, a.warmup,
                         dev) for n in a.shapes}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
