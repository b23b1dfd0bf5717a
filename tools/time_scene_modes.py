"""Time the fused k-medoid reduction of joint samples to scene modes
(g2k_scene_modes_f32 and its fullcov_ / mix_ / coupled_ twins,
csrc/g2k_scene_modes.hip) against the composition it replaces — K sampler
launches, then the matrix of summed per-step displacements, PAM BUILD, the
alternating rounds and the scores in torch float64, batched over the
scene-frames — and next to the same head's scene_ranks call at the same K (the
same joint draws and tiles, one root per pair where this one takes a root per
member and step).

  python tools/time_scene_modes.py [--calls 30] [--warmup 2] [--ks 20 64] [--modes 6] [--heads ...]

Shapes: the real-data evaluation's (F 1, S 384 scenes, Nmax 32, n_active 2..32)
and dense_crowd's (S 64, F 20, Nmax 256), synthetic.make_batch; pred = the
targets + N(0, 0.05^2), head sigma 0.05 (the full-covariance head: the same
marginals, AR(1) 0.7 over the steps; the mixture head: that factor in three
components; the scene-coupled head: that law cut in two, share 0.6).  The
composition materialises [s, K + 1, K + 1, Nmax, 12, 2] float64 differences, so
it runs over chunks of scene-frames sized to about 1 GiB per temporary.  The
paths run in one process, alternating call by call, each call between its own
pair of device events; the figures are medians, the spread is the 10th..90th
percentile.  Before timing the fused call and the composition must agree: tot
exactly, the sums to 1e-9.  The one gate: the fused call is faster than the
composition.  Prints one JSON line.  Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multimodaltraj_2_amd import scenemodes as sd                                         # noqa: E402
from multimodaltraj_2_amd.synthetic import make_batch                                     # noqa: E402
from tools.time_scene_ranks import HEADS, SHAPES, SIGMA, make_head                        # noqa: E402

CHUNK_BYTES = 1 << 30
RADIUS = 0.1


def lowest(v, want_max=False):
    """(best value, its lowest index) along the last dimension."""
    b = v.max(dim=-1, keepdim=True).values if want_max else v.min(dim=-1, keepdim=True).values
    idx = torch.arange(v.shape[-1], device=v.device).expand_as(v)
    return b.squeeze(-1), torch.where(v == b, idx, v.shape[-1]).min(dim=-1).values


def unfused(head, pred, targets, mem, K, M, iters, radius, seed):
    """K sampler launches, then include/g2k_scene_modes.h in torch float64,
    batched over the scene-frames -> (sums [S, 8], tot [S, 4])."""
    S, F, _, N = pred.shape
    dev, f64 = pred.device, torch.float64
    B, NI = S * F, K + 1
    draws = torch.stack([head.sample(pred, seed=seed + k) for k in range(K)], dim=2)         # [S, F, K, 24, N]
    xy = torch.stack([draws[:, :, :, :12], draws[:, :, :, 12:]], dim=-1).permute(0, 1, 2, 4, 3, 5)
    Z = torch.cat([xy, targets.view(S, F, 1, N, 12, 2)], dim=2).reshape(B, NI, N, 12, 2).to(f64)
    w = mem.view(B, 1, 1, N, 1).to(f64)
    A = torch.empty((B, NI, NI), dtype=f64, device=dev)
    last = torch.empty((B, K, N), dtype=f64, device=dev)
    sc = int(max(1, min(B, CHUNK_BYTES // (NI * NI * N * 24 * 8))))
    for s0 in range(0, B, sc):
        z = Z[s0:s0 + sc]
        e = (z[:, :, None] - z[:, None]).pow(2).sum(dim=-1).sqrt() * w[s0:s0 + sc]           # [b, NI, NI, N, 12]
        A[s0:s0 + sc] = e.sum(dim=(3, 4))
        last[s0:s0 + sc] = e[:, :K, K, :, 11]
    Fn, Mx = last.sum(dim=2), last.max(dim=2).values
    Pn = mem.view(B, N).sum(dim=1)
    scored = Pn >= 1
    D = A[:, :K, :K]
    ar = torch.arange(B, device=dev)
    # PAM BUILD
    med = torch.zeros((B, M), dtype=torch.long, device=dev)
    med[:, 0] = lowest(D.sum(dim=2))[1]
    dmin = D[ar, :, med[:, 0]]
    chosen = torch.zeros((B, K), dtype=torch.bool, device=dev)
    chosen[ar, med[:, 0]] = True
    for i in range(1, M):
        gain = (dmin[:, None, :] - D).clamp(min=0.0).sum(dim=2)
        med[:, i] = lowest(torch.where(chosen, -torch.inf, gain), want_max=True)[1]
        chosen[ar, med[:, i]] = True
        dmin = torch.minimum(dmin, D[ar, :, med[:, i]])
    # the alternating rounds, every scene-frame until its own first round that changes nothing
    modes = torch.arange(M, device=dev)
    active = torch.ones(B, dtype=torch.bool, device=dev)
    rounds = torch.zeros(B, dtype=torch.long, device=dev)
    assign = lambda: lowest(D.gather(2, med[:, None, :].expand(B, K, M)))                     # noqa: E731
    for _ in range(iters):
        asg = assign()[1]
        c = (D * (asg[:, :, None] == asg[:, None, :])).sum(dim=2)                              # [B, K]
        cm = torch.where(asg[:, None, :] == modes[None, :, None], c[:, None, :], torch.inf)    # [B, M, K]
        best, j = lowest(cm)
        new = torch.where(torch.isinf(best) | ~active[:, None], med, j)
        changed = (new != med).any(dim=1)
        med = new
        rounds += active
        active = active & changed
    dist, asg = assign()
    cnt = (asg[:, :, None] == modes[None, None, :]).sum(dim=1)                                 # [B, M]
    p = Pn.clamp(min=1).to(f64)
    JA, mA = lowest(A[:, :K, K].gather(1, med))
    JF, mF = lowest(Fn.gather(1, med))
    mx = Mx.gather(1, med).min(dim=1).values
    wA, wF = cnt.gather(1, mA[:, None])[:, 0].to(f64) / K, cnt.gather(1, mF[:, None])[:, 0].to(f64) / K
    cost = dist.sum(dim=1) / (12.0 * K * p)
    raw, al = A[:, :M, K].min(dim=1).values / (12 * p), A[:, :K, K].min(dim=1).values / (12 * p)
    live = scored.to(f64)
    rows = torch.stack([JA / 12, JF, (1 - wA) ** 2 * live, (1 - wF) ** 2 * live, cost * p, raw * p, al * p,
                        torch.zeros_like(p)], dim=1) * live[:, None]
    tot = torch.stack([scored, Pn * scored, scored & (mx > radius), rounds * scored], dim=1).long()
    return rows.view(S, F, 8).sum(dim=1), tot.view(S, F, 4).sum(dim=1)


def time_shape(name, which, S, F, Nmax, K, M, iters, calls, warmup, dev):
    b = make_batch(S, Nmax, 64, F=F, seed=5)
    rng = np.random.default_rng(6)
    pred_h = (np.transpose(b.targets, (0, 1, 4, 3, 2)).reshape(S, F, 24, Nmax)
              + SIGMA * rng.standard_normal((S, F, 24, Nmax))).astype(np.float32)
    pred = torch.from_numpy(pred_h).to(dev)
    targets = torch.from_numpy(b.targets).to(dev)
    n_active = torch.from_numpy(b.n_active).to(dev)
    mem = (torch.arange(Nmax, device=dev)[None, None, :] < n_active[:, None, None]).expand(S, F, Nmax).contiguous()
    head = make_head(which, dev)
    seed = 1234
    bins = next(d for d in range(min(32, K + 1), 0, -1) if (K + 1) % d == 0)

    def fused():
        return head.scene_modes(pred, targets, n_active, K, M, iters, RADIUS, seed=seed, want_modes=False)

    def ranks():
        return head.scene_ranks(pred, targets, n_active, K, bins, seed=seed)

    def parent():
        return unfused(head, pred, targets, mem, K, M, iters, float(np.float32(RADIUS)), seed)

    got, want = fused(), parent()
    torch.cuda.synchronize()
    err = float(((got.sums - want[0]).abs() / want[0].abs().clamp(min=1.0)).max())
    same = torch.equal(got.tot, want[1])
    if err > 1e-9 or not same:
        raise SystemExit(f"{name} {which} K {K}: the two paths disagree (sums {err:.3g}, tot equal: {same})")
    paths = [fused, ranks, parent]
    for _ in range(warmup):
        for fn in paths:
            fn()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2 * len(paths))] for _ in range(calls)]
    for e in ev:                                   # alternating, each call in its own event pair
        for j, fn in enumerate(paths):
            e[2 * j].record(); fn(); e[2 * j + 1].record()
    torch.cuda.synchronize()
    t = [np.array([e[2 * j].elapsed_time(e[2 * j + 1]) for e in ev]) * 1e3 for j in range(len(paths))]   # us
    q = lambda a: [round(float(np.percentile(a, p)), 2) for p in (10, 50, 90)]   # noqa: E731
    tf, tr, tp = t
    if not np.median(tf) < np.median(tp):
        raise SystemExit(f"{name} {which} K {K}: the fused call ({q(tf)[1]} us) is not faster than the "
                         f"composition ({q(tp)[1]} us)")
    return dict(S=S, F=F, Nmax=Nmax, K=K, M=M, iters=iters, head=which, frames=got.frames, calls=calls,
                geometry=sd.scene_modes_geometry(S, F, Nmax, K, M),
                fused_us=q(tf)[1], fused_us_p10_p90=[q(tf)[0], q(tf)[2]],
                unfused_us=q(tp)[1], unfused_us_p10_p90=[q(tp)[0], q(tp)[2]],
                scene_ranks_us=q(tr)[1], scene_ranks_us_p10_p90=[q(tr)[0], q(tr)[2]],
                ratio=round(float(np.median(tp) / np.median(tf)), 2),
                over_scene_ranks=round(float(np.median(tf) / np.median(tr)), 2),
                jade=got.jade, raw_jade=got.raw_jade, all_jade=got.all_jade, miss_rate=got.miss_rate,
                rounds=got.rounds, paths_max_rel_diff=err)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ks", type=int, nargs="*", default=[20, 64])
    ap.add_argument("--modes", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--heads", nargs="*", choices=HEADS, default=list(HEADS))
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_scene_modes: needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {}
    for n in a.shapes:
        for k in a.ks:
            for h in a.heads:
                out[f"{n}/K{k}/{h}"] = time_shape(n, h, SHAPES[n]["S"], SHAPES[n]["F"], SHAPES[n]["Nmax"], k,
                                                  a.modes, a.iters, a.calls, a.warmup, dev)
                print(json.dumps({f"{n}/K{k}/{h}": out[f"{n}/K{k}/{h}"]}), file=sys.stderr, flush=True)
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
