"""Time the fused scene-level rank calibration (g2k_scene_ranks_f32 and its
fullcov_ / mix_ / coupled_ twins, csrc/g2k_scene_ranks.hip) against the
composition it replaces — K sampler launches, then the items' distance matrix,
the three features, the ranks and the energy-score terms in torch float64 — and
next to the same head's couple_scores call (the same joint draws, two members
at a time).

  python tools/time_scene_ranks.py [--calls 50] [--warmup 3] [--k 20] [--bins 7] [--heads ...]

Shapes: the real-data evaluation's (F 1, S 384 scenes, Nmax 32, n_active 2..32)
and dense_crowd's (S 64, F 20, Nmax 256), synthetic.make_batch; pred = the
targets + N(0, 0.05^2), head sigma 0.05 (the full-covariance head: the same
marginals, AR(1) 0.7 over the steps; the mixture head: that factor in three
components; the scene-coupled head: that law cut in two, share 0.6).  The
composition materialises [s, K + 1, K + 1, 24 Nmax] float64 differences, so it
runs over chunks of scene-frames sized to about 1 GiB per temporary.  The paths
run in one process, alternating call by call, each call between its own pair of
device events; the figures are medians, the spread is the 10th..90th
percentile.  Before timing the fused call and the composition must agree: the
scored scene-frames, the ranks' sums and the histograms exactly, the float sums
to 1e-9.  The one gate: the fused call is faster than the composition.  Prints
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

from multimodaltraj_2_amd import sceneranks as sn              # noqa: E402
from multimodaltraj_2_amd.coupled import CoupledHead          # noqa: E402
from multimodaltraj_2_amd.fullcov import FullCovHead          # noqa: E402
from multimodaltraj_2_amd.mixture import MixtureHead          # noqa: E402
from multimodaltraj_2_amd.nll import GaussianHead             # noqa: E402
from multimodaltraj_2_amd.synthetic import make_batch         # noqa: E402

SHAPES = {"realdata_eval": dict(S=384, F=1, Nmax=32),
          "dense_crowd": dict(S=64, F=20, Nmax=256)}
HEADS = ("per_step", "fullcov", "mix", "coupled")
CHUNK_BYTES = 1 << 30
SIGMA = 0.05
SHARE = 0.6


def make_head(which, dev):
    if which == "per_step":
        return GaussianHead(log_sigma=float(np.log(SIGMA)), device=dev)
    T = 0.7 ** np.abs(np.subtract.outer(np.arange(12), np.arange(12)))
    chol = np.linalg.cholesky(SIGMA * SIGMA * np.kron(T, np.eye(2))).astype(np.float32)
    if which in ("fullcov", "coupled"):
        h = FullCovHead(device=dev)
        h.chol = torch.from_numpy(chol).to(dev)
        return h if which == "fullcov" else CoupledHead.from_fullcov(h, SHARE)
    block = np.zeros((8, 608), np.float32)
    for m, (w, shift) in enumerate(((0.5, 0.0), (0.3, 0.03), (0.2, -0.03))):
        block[m, 0] = w
        block[m, 8:32] = shift
        block[m, 32:] = chol.reshape(-1)
    return MixtureHead.from_block(block, device=dev)


def unfused(head, pred, targets, mem, K, B, seed):
    """K sampler launches, then per chunk of scene-frames the pooled items'
    distances from differences, the features, the ranks and the energy-score
    terms, float64 -> (sums [S, 6], hist [S, 3, B], tot [S, 4])."""
    S, F, _, N = pred.shape
    dev = pred.device
    draws = torch.stack([head.sample(pred, seed=seed + k) for k in range(K)], dim=2)         # [S, F, K, 24, N]
    ty = targets.permute(0, 1, 4, 3, 2).reshape(S, F, 1, 24, N)                            # band layout
    w = mem.view(S * F, 1, 1, N).to(torch.float64)
    Z = torch.cat([draws, ty], dim=2).view(S * F, K + 1, 24, N).to(torch.float64) * w      # non-members: 0
    R = Z - pred.view(S * F, 1, 24, N).to(torch.float64) * w
    Pn = mem.view(S * F, N).sum(dim=1)
    scored = Pn >= 2
    sc = int(max(1, min(S * F, CHUNK_BYTES // ((K + 1) * (K + 1) * 24 * N * 8))))
    D = torch.empty((S * F, K + 1, K + 1), dtype=torch.float64, device=dev)
    for s0 in range(0, S * F, sc):
        z = Z[s0:s0 + sc].flatten(2)
        d = z[:, :, None] - z[:, None]
        D[s0:s0 + sc] = (d * d).sum(dim=3).sqrt()
    typ = D.sum(dim=2)
    s = R.sum(dim=3)                                                                       # [SF, K + 1, 24]
    q = (R * R).sum(dim=(2, 3))
    loc = (s * s).sum(dim=2) / Pn.clamp(min=1).to(torch.float64)[:, None]
    spr = q - loc
    m = D[:, :K, K].sum(dim=1) / K
    p = 2.0 * torch.triu(D[:, :K, :K], 1).sum(dim=(1, 2)) / (K * (K - 1))
    rows = torch.stack([m, p, loc[:, :K].mean(dim=1), loc[:, K], spr[:, :K].mean(dim=1), spr[:, K]], dim=1)
    rows = rows * scored[:, None].to(torch.float64)
    ranks = torch.stack([(g[:, :K] < g[:, K:]).sum(dim=1) for g in (typ, loc, spr)], dim=1)  # [SF, 3]
    ranks = ranks * scored[:, None]
    sums = rows.view(S, F, 6).sum(dim=1)
    tot = torch.cat([scored.view(S, F).sum(dim=1, keepdim=True), ranks.view(S, F, 3).sum(dim=1)], dim=1)
    hist = torch.zeros((S, 3, B), dtype=torch.int64, device=dev)
    bins = (ranks * B // (K + 1)).view(S, F, 3).permute(0, 2, 1)                            # [S, 3, F]
    hist.scatter_add_(2, bins, scored.view(S, 1, F).expand(S, 3, F).to(torch.int64))
    return sums, hist, tot


def time_shape(name, which, S, F, Nmax, K, B, calls, warmup, dev):
    b = make_batch(S, Nmax, 64, F=F, seed=5)
    rng = np.random.default_rng(6)
    pred_h = (np.transpose(b.targets, (0, 1, 4, 3, 2)).reshape(S, F, 24, Nmax)
              + SIGMA * rng.standard_normal((S, F, 24, Nmax))).astype(np.float32)
    pred = torch.from_numpy(pred_h).to(dev)
    targets = torch.from_numpy(b.targets).to(dev)
    n_active = torch.from_numpy(b.n_active).to(dev)
    mem = (torch.arange(Nmax, device=dev)[None, None, :] < n_active[:, None, None]).expand(S, F, Nmax).contiguous()
    head = make_head(which, dev)
    twin = make_head("fullcov", dev) if which == "coupled" else None
    seed = 1234

    def fused(h=head):
        return h.scene_ranks(pred, targets, n_active, K, B, seed=seed)

    def couple():
        return head.couple_scores(pred, targets, n_active, K, B, seed=seed)

    def parent():
        return unfused(head, pred, targets, mem, K, B, seed)

    got, want = fused(), parent()
    torch.cuda.synchronize()
    err = float(((got.sums - want[0]).abs() / want[0].abs().clamp(min=1.0)).max())
    same = torch.equal(got.tot, want[2]) and torch.equal(got.hist.to(torch.int64), want[1])
    if err > 1e-9 or not same:
        raise SystemExit(f"{name} {which}: the two paths disagree (sums {err:.3g}, counts equal: {same})")
    paths = [fused, couple, parent] + ([lambda: fused(twin)] if twin is not None else [])
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
    tf, tc, tp = t[:3]
    if not np.median(tf) < np.median(tp):
        raise SystemExit(f"{name} {which}: the fused call ({q(tf)[1]} us) is not faster than the composition "
                         f"({q(tp)[1]} us)")
    out = dict(S=S, F=F, Nmax=Nmax, K=K, B=B, head=which, frames=got.frames, calls=calls,
               geometry=sn.scene_ranks_geometry(S, F, Nmax, K),
               fused_us=q(tf)[1], fused_us_p10_p90=[q(tf)[0], q(tf)[2]],
               unfused_us=q(tp)[1], unfused_us_p10_p90=[q(tp)[0], q(tp)[2]],
               couple_scores_us=q(tc)[1], couple_scores_us_p10_p90=[q(tc)[0], q(tc)[2]],
               ratio=round(float(np.median(tp) / np.median(tf)), 2),
               over_couple_scores=round(float(np.median(tf) / np.median(tc)), 2),
               es=got.es, dev={g: got.dev(g) for g in sn.FEATURES}, pit={g: got.pit(g) for g in sn.FEATURES},
               paths_max_rel_diff=err)
    if twin is not None:
        out.update(fullcov_twin_us=q(t[3])[1], fullcov_twin_us_p10_p90=[q(t[3])[0], q(t[3])[2]],
                   over_fullcov_twin=round(float(np.median(tf) / np.median(t[3])), 2))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--bins", type=int, default=7)
    ap.add_argument("--heads", nargs="*", choices=HEADS, default=list(HEADS))
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_scene_ranks: needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {f"{n}/{h}": time_shape(n, h, SHAPES[n]["S"], SHAPES[n]["F"], SHAPES[n]["Nmax"], a.k, a.bins, a.calls,
                                  a.warmup, dev) for n in a.shapes for h in a.heads}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
