"""Time the fused joint best-of-K evaluation of the full-covariance head
(g2k_fullcov_joint_eval_f32) against (a) the composition it replaces —
K x FullCovHead.sample, the draws' errors averaged over a scene-frame's members
with a running minimum, and the pairwise distances of every draw in torch —
and (b) the per-step head's fused call (g2k_joint_eval_f32) at the same shape
and K.

  python tools/time_fullcov_joint.py [--calls 50] [--warmup 5] [--runs 3] [--k 20] [--radius 0.05]

Shapes: those of tools/time_joint_eval.py — the real-data evaluation's (F 1,
S 384 scenes, Nmax 32, n_active 2..32) and dense_crowd's (S 64, F 20, Nmax
256), synthetic.make_batch; pred = the targets + N(0, 0.05^2); the factor is a
random walk's whose last step has standard deviation 0.05, the per-step head of
(b) has that walk's marginals.  The composition materialises [k, S, F, 12,
Nmax, Nmax] distances, so it runs over chunks of k sized to about 1 GiB per
temporary (one k at a time at dense_crowd: 4 GiB).  The paths of a comparison
run in one process, alternating call by call, each call between its own pair
of device events ((a) takes a fifth of the calls: its composition is slow);
per run the median and the 10th..90th percentile, and the reported figure is
the median of the runs'.  Before timing the two paths of (a) must agree: the
JADE / JFDE sums to 1e-4, the collision totals to 1e-3 (torch squares without
the kernel's fmaf, so a couple at the threshold may fall either side).  Prints
one JSON line.  Needs a GPU: there is no fallback.
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
from multimodaltraj_2_amd.nll import GaussianHead          # noqa: E402
from multimodaltraj_2_amd.synthetic import make_batch       # noqa: E402

SHAPES = {"realdata_eval": dict(S=384, F=1, Nmax=32),
          "dense_crowd": dict(S=64, F=20, Nmax=256)}
CHUNK_BYTES = 1 << 30
SIGMA = 0.05                                               # the walk's last step


def unfused(fc, pred, targets, members, couples, K, radius, seed):
    """K sampler launches; per chunk of draws the errors, their member means
    and the pairwise minimum distances in torch.  -> (sum_f P minJADE [S],
    sum_f P minJFDE [S], sum_k col_k [S])."""
    S, F, _, N = pred.shape
    P = members.sum(dim=2)                                             # [S, F]
    Pd = P.clamp(min=1.0)
    kc = int(max(1, min(K, CHUNK_BYTES // max(1, S * F * 12 * N * N * 4))))
    r2 = radius * radius
    mn_a = mn_f = None
    col = torch.zeros(S, dtype=torch.int64, device=pred.device)
    for k0 in range(0, K, kc):
        x = torch.stack([fc.sample(pred, seed=seed + k) for k in range(k0, min(K, k0 + kc))])
        xy = x.view(-1, S, F, 2, 12, N)
        d = torch.linalg.vector_norm(xy.permute(0, 1, 2, 5, 4, 3) - targets, dim=-1)   # [k, S, F, N, 12]
        ja = ((d.mean(dim=-1) * members).sum(dim=-1) / Pd).amin(dim=0)
        jf = ((d[..., 11] * members).sum(dim=-1) / Pd).amin(dim=0)
        mn_a = ja if mn_a is None else torch.minimum(mn_a, ja)
        mn_f = jf if mn_f is None else torch.minimum(mn_f, jf)
        dx = xy[:, :, :, 0, :, :, None] - xy[:, :, :, 0, :, None, :]   # [k, S, F, 12, N, N]
        dy = xy[:, :, :, 1, :, :, None] - xy[:, :, :, 1, :, None, :]
        hit = ((dx * dx + dy * dy).amin(dim=3) < r2) & couples
        col += hit.sum(dim=(0, 2, 3, 4))
    return (P * mn_a).sum(dim=1), (P * mn_f).sum(dim=1), col


def alternate(fns, calls, warmup):
    """-> one array of microseconds per function: alternating, each call
    between its own pair of device events."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns]
          for _ in range(calls)]
    for row in ev:
        for f, (a, b) in zip(fns, row):
            a.record(); f(); b.record()
    torch.cuda.synchronize()
    return [np.array([row[i][0].elapsed_time(row[i][1]) for row in ev]) * 1e3 for i in range(len(fns))]


def summary(runs):
    """runs: one array per run -> median of the runs' medians, the widest 10th..90th."""
    med = [float(np.median(a)) for a in runs]
    p10 = min(float(np.percentile(a, 10)) for a in runs)
    p90 = max(float(np.percentile(a, 90)) for a in runs)
    return round(float(np.median(med)), 2), [round(p10, 2), round(p90, 2)]


def time_shape(name, S, F, Nmax, K, radius, calls, warmup, runs, dev):
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
    members = mem.to(torch.float32).contiguous()
    step = SIGMA / np.sqrt(12.0)
    Lw = np.zeros((24, 24), np.float32)
    for t in range(12):
        for u in range(t + 1):
            Lw[2 * t, 2 * u] = Lw[2 * t + 1, 2 * u + 1] = step
    fc = FullCovHead(device=dev)
    fc.chol = torch.from_numpy(Lw).to(dev)
    gh = GaussianHead(device=dev)
    gh.head[:2] = torch.log(step * torch.sqrt(torch.arange(1, 13, device=dev, dtype=torch.float32)))
    seed = 1234

    def fused():
        return fc.joint_eval(pred, targets, n_active, K, radius, seed=seed, want_per_frame=False)

    def composed():
        return unfused(fc, pred, targets, members, couples, K, radius, seed)

    def perstep():
        return gh.joint_eval(pred, targets, n_active, K, radius, seed=seed, want_per_frame=False)

    # the two paths of (a) agree before they are timed
    got, want, ps = fused(), composed(), perstep()
    torch.cuda.synchronize()
    err = max(float(((got.sums_f[:, i] - want[i]).abs() / want[i].abs().clamp(min=1.0)).max())
              for i in (0, 1))
    cg, cw = int(got.sums_i[:, 4].sum()), int(want[2].sum())
    if err > 1e-4 or abs(cg - cw) > 1e-3 * max(cw, 1):
        raise SystemExit(f"{name}: the two paths disagree (errors {err:.3g}, collisions {cg} / {cw})")
    if not torch.equal(got.sums_i[:, :4], ps.sums_i[:, :4]):
        raise SystemExit(f"{name}: the head-independent columns differ between the two fused calls")

    ta, tb = [[], []], [[], []]
    for _ in range(runs):
        for acc, fns, n, wu in ((ta, (fused, composed), max(5, calls // 5), min(warmup, 2)),
                                (tb, (fused, perstep), calls, warmup)):
            t = alternate(fns, n, wu)
            acc[0].append(t[0])
            acc[1].append(t[1])
    (a0, sa0), (a1, sa1) = summary(ta[0]), summary(ta[1])
    (b0, sb0), (b1, sb1) = summary(tb[0]), summary(tb[1])
    return dict(S=S, F=F, Nmax=Nmax, K=K, radius=radius, pairs=got.pairs, couples=got.ped_pairs,
                calls=calls, runs=runs,
                a=dict(fused_us=a0, fused_us_p10_p90=sa0, sample_torch_us=a1, sample_torch_us_p10_p90=sa1,
                       ratio=round(a1 / a0, 2)),
                b=dict(fullcov_us=b0, fullcov_us_p10_p90=sb0, perstep_us=b1, perstep_us_p10_p90=sb1,
                       ratio=round(b0 / b1, 3)),
                draws_per_s=round(got.pairs * K * 12 / (b0 * 1e-6), 0),
                jade=dict(fullcov=got.jade, perstep=ps.jade),
                collision_rate=dict(fullcov=got.collision_rate, perstep=ps.collision_rate,
                                    mean=got.collision_rate_pred, gt=got.collision_rate_gt),
                collisions_fused=cg, collisions_composed=cw, paths_max_rel_diff=err)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--radius", type=float, default=0.05)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_fullcov_joint: needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {n: time_shape(n, SHAPES[n]["S"], SHAPES[n]["F"], SHAPES[n]["Nmax"], a.k, a.radius, a.calls,
                         a.warmup, a.runs, dev) for n in a.shapes}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
