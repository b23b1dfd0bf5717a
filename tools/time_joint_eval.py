"""Time the fused joint best-of-K evaluation (g2k_joint_eval_f32) against the
composition it replaces: K x GaussianHead.sample, the draws' errors averaged
over a scene-frame's members with a running minimum, and the pairwise
distances of every draw in torch.

  python tools/time_joint_eval.py [--calls 100] [--warmup 10] [--k 20] [--radius 0.05]

Shapes: the real-data evaluation's (F 1, S 384 scenes, Nmax 32, n_active 2..32)
and dense_crowd's (S 64, F 20, Nmax 256), synthetic.make_batch; pred = the
targets + N(0, 0.05^2), head sigma 0.05.  The composition materialises
[k, S, F, 12, Nmax, Nmax] distances, so it runs over chunks of k sized to
about 1 GiB per temporary (one k at a time at dense_crowd: 4 GiB).  Both paths
run in one process, alternating call by call, each call between its own pair
of device events; the figures are medians, the spread is the 10th..90th
percentile.  Before timing the two paths must agree: the JADE / JFDE sums to
1e-4, the collision totals to 1e-3 (torch squares without the kernel's fmaf,
so a couple at the threshold may fall either side).  Prints one JSON line.
Needs a GPU: there is no fallback.
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
from multimodaltraj_2_amd.synthetic import make_batch       # noqa: E402

SHAPES = {"realdata_eval": dict(S=384, F=1, Nmax=32),
          "dense_crowd": dict(S=64, F=20, Nmax=256)}
CHUNK_BYTES = 1 << 30


def unfused(gh, pred, targets, members, couples, K, radius, seed):
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
        x = torch.stack([gh.sample(pred, seed=seed + k) for k in range(k0, min(K, k0 + kc))])
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


def time_shape(name, S, F, Nmax, K, radius, calls, warmup, dev):
    b = make_batch(S, Nmax, 64, F=F, seed=5)
    rng = np.random.default_rng(6)
    pred_h = (np.transpose(b.targets, (0, 1, 4, 3, 2)).reshape(S, F, 24, Nmax)
              + 0.05 * rng.standard_normal((S, F, 24, Nmax))).astype(np.float32)
    pred = torch.from_numpy(pred_h).to(dev)
    targets = torch.from_numpy(b.targets).to(dev)
    n_active = torch.from_numpy(b.n_active).to(dev)
    mem = (torch.arange(Nmax, device=dev)[None, None, :] < n_active[:, None, None]).expand(S, F, Nmax)
    couples = (mem[:, :, :, None] & mem[:, :, None, :]
               & torch.ones((Nmax, Nmax), dtype=torch.bool, device=dev).triu(1)).contiguous()
    members = mem.to(torch.float32).contiguous()
    gh = GaussianHead(log_sigma=float(np.log(0.05)), device=dev)
    seed = 1234

    def fused():
        return gh.joint_eval(pred, targets, n_active, K, radius, seed=seed, want_per_frame=False)

    def parent():
        return unfused(gh, pred, targets, members, couples, K, radius, seed)

    got, want = fused(), parent()
    torch.cuda.synchronize()
    err = max(float(((got.sums_f[:, i] - want[i]).abs() / want[i].abs().clamp(min=1.0)).max())
              for i in (0, 1))
    cg, cw = int(got.sums_i[:, 4].sum()), int(want[2].sum())
    if err > 1e-4 or abs(cg - cw) > 1e-3 * max(cw, 1):
        raise SystemExit(f"{name}: the two paths disagree (errors {err:.3g}, collisions {cg} / {cw})")
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
    q = lambda a: [round(float(np.percentile(a, p)), 2) for p in (10, 50, 90)]   # noqa: E731
    n_pairs, n_couples = got.pairs, got.ped_pairs
    return dict(S=S, F=F, Nmax=Nmax, K=K, radius=radius, pairs=n_pairs, couples=n_couples, calls=calls,
                fused_us=q(tf)[1], fused_us_p10_p90=[q(tf)[0], q(tf)[2]],
                unfused_us=q(tp)[1], unfused_us_p10_p90=[q(tp)[0], q(tp)[2]],
                ratio=round(float(np.median(tp) / np.median(tf)), 2),
                draws_per_s=round(n_pairs * K * 12 / (float(np.median(tf)) * 1e-6), 0),
                couple_steps_per_s=round(n_couples * (K + 2) * 12 / (float(np.median(tf)) * 1e-6), 0),
                collisions_fused=cg, collisions_unfused=cw, collision_rate=got.collision_rate,
                paths_max_rel_diff=err)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--radius", type=float, default=0.05)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_joint_eval: needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {n: time_shape(n, SHAPES[n]["S"], SHAPES[n]["F"], SHAPES[n]["Nmax"], a.k, a.radius, a.calls,
                         a.warmup, dev) for n in a.shapes}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
