"""Time the full-covariance trajectory head's fused calls (csrc/g2k_fullcov.hip)
against their compositions:

  (a) g2k_fullcov_best_of_k_f32 against K g2k_fullcov_sample_f32 launches with
      the errors and the running minimum in torch,
  (b) g2k_fullcov_best_of_k_f32 against g2k_best_of_k_f32 (the per-step head)
      at the same shape and K: what the 24 x 24 triangular product costs,
  (c) g2k_fullcov_stats_f32 with 11 levels against the same figures composed
      in torch float64 (residuals, Gram, triangular solve, q, nll, counts).

  python tools/time_fullcov.py [--calls 50] [--warmup 5] [--runs 3] [--k 20]

Shapes: eth_hotel_synth (S 256, Nmax 32) and one rank's share of dense_crowd
(S 128 of 1024 over 8 GPUs, Nmax 256), F 20, synthetic.make_batch; pred = the
targets + a random-walk residual, the factor that walk's.  The paths of a
comparison run in one process, alternating call by call, each call between its
own pair of device events; a run's figure is its median, the spread its
10th..90th percentile, and the reported figure is the median of the runs'.
Prints one JSON line.  Needs a GPU: there is no fallback.
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

from multimodaltraj_2_amd.fullcov import FullCovHead                        # noqa: E402
from multimodaltraj_2_amd.nll import DEFAULT_LEVELS, GaussianHead           # noqa: E402
from multimodaltraj_2_amd.synthetic import CONFIGS, FRAMES_PER_SCENE, make_batch   # noqa: E402

SHAPES = {"eth_hotel_synth": dict(S=CONFIGS["eth_hotel_synth"]["S"], Nmax=32),
          "dense_crowd": dict(S=CONFIGS["dense_crowd"]["S"] // 8, Nmax=256)}
SIGMA = 0.05


def composed_best_of_k(fc, pred, targets, pairs, K, seed):
    """K sampler launches, the errors and the running minimum in torch ->
    (sum minADE, sum minFDE) over the pairs."""
    S, F, _, N = pred.shape
    tx, ty = targets[..., 0].permute(0, 1, 3, 2), targets[..., 1].permute(0, 1, 3, 2)   # [S, F, 12, N]
    bA = bF = None
    for k in range(K):
        x = fc.sample(pred, seed=seed + k)
        d = torch.sqrt((x[:, :, :12] - tx) ** 2 + (x[:, :, 12:] - ty) ** 2)
        ade, fde = d.mean(dim=2), d[:, :, 11]
        bA = ade if bA is None else torch.minimum(bA, ade)
        bF = fde if bF is None else torch.minimum(bF, fde)
    return (bA * pairs).sum(), (bF * pairs).sum()


def composed_stats(chol, pred, targets, pairs, r2):
    """The stats call's figures in torch, float64 -> (M [24, 24], sum q_t [12],
    sum nll_t [12], inside [13, NL])."""
    S, F, _, N = pred.shape
    Lm = torch.tril(chol.double())
    p = pred.view(S, F, 2, 12, N).permute(0, 1, 4, 3, 2).double()      # [S, F, N, 12, 2]
    r = ((targets.double() - p) * pairs[..., None, None]).reshape(-1, 24)
    M = r.t() @ r
    z = torch.linalg.solve_triangular(Lm, r.t(), upper=False).t()
    qt = (z * z).view(-1, 12, 2).sum(dim=2)
    q = qt.sum(dim=1)
    on = pairs.reshape(-1) > 0
    dg = torch.log(torch.diagonal(Lm)).view(12, 2).sum(dim=1)
    nll = on.sum() * (math.log(2 * math.pi) + dg) + 0.5 * qt.sum(dim=0)
    ins = [((qt <= r2[0, l]) & on[:, None]).sum(dim=0) for l in range(r2.shape[1])]
    insj = torch.stack([((q <= r2[1, l]) & on).sum() for l in range(r2.shape[1])])
    return M, qt.sum(dim=0), nll, torch.cat([torch.stack(ins, dim=1), insj[None]], dim=0)


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


def time_shape(name, S, Nmax, K, calls, warmup, runs, dev):
    F = FRAMES_PER_SCENE
    b = make_batch(S, Nmax, 64, F=F, seed=5)
    rng = np.random.default_rng(6)
    walk = SIGMA * np.cumsum(rng.standard_normal((S, F, 2, 12, Nmax)), axis=3)
    pred_h = (np.transpose(b.targets, (0, 1, 4, 3, 2)).reshape(S, F, 24, Nmax) -
              walk.reshape(S, F, 24, Nmax)).astype(np.float32)
    pred = torch.from_numpy(pred_h).to(dev)
    targets = torch.from_numpy(b.targets).to(dev)
    n_active = torch.from_numpy(b.n_active).to(dev)
    pm = (torch.arange(Nmax, device=dev)[None, None, :] < n_active[:, None, None]).expand(S, F, Nmax)
    pairs32, pairs64 = pm.float().contiguous(), pm.double().contiguous()
    Lw = np.zeros((24, 24), np.float32)
    for t in range(12):
        for u in range(t + 1):
            Lw[2 * t, 2 * u] = Lw[2 * t + 1, 2 * u + 1] = SIGMA
    fc = FullCovHead(device=dev)
    fc.chol = torch.from_numpy(Lw).to(dev)
    gh = GaussianHead(device=dev)
    gh.head[:2] = torch.log(SIGMA * torch.sqrt(torch.arange(1, 13, device=dev, dtype=torch.float32)))
    levels = tuple(DEFAULT_LEVELS)
    r2 = fc._r2(levels, dev)
    seed = 11

    def fused_bk():
        return fc.best_of_k(pred, targets, n_active, K, seed=seed, want_per_ped=False).sums

    def comp_bk():
        return composed_best_of_k(fc, pred, targets, pairs32, K, seed)

    def step_bk():
        return gh.best_of_k(pred, targets, n_active, K, seed=seed, want_per_ped=False).sums

    def fused_st():
        r = fc.stats(pred, targets, n_active, levels)
        return r.moments, r.stats, r.inside

    def comp_st():
        return composed_stats(fc.chol, pred, targets, pairs64, r2)

    # the paths agree before they are timed
    fs, (ca, cf) = fused_bk().double().sum(dim=0), comp_bk()
    e_bk = max(abs(float(fs[0]) - float(ca)) / float(ca), abs(float(fs[1]) - float(cf)) / float(cf))
    (mo, st, ins), (M, sq, snll, cins) = fused_st(), comp_st()
    torch.cuda.synchronize()
    e_st = max(float(((mo[:24] - M).abs() / M.abs().clamp(min=1.0)).max()),
               float(((st[:, 2] - sq).abs() / sq.abs().clamp(min=1.0)).max()),
               float(((st[:, 1] - snll).abs() / snll.abs().clamp(min=1.0)).max()))
    if e_bk > 1e-4 or e_st > 1e-9 or not torch.equal(ins, cins):
        raise SystemExit(f"{name}: the paths disagree (best-of-K {e_bk:.3g}, stats {e_st:.3g}, counts "
                         f"{int((ins - cins).abs().max())})")
    mins = dict(fullcov_min_ade=float(fs[0] / fs[2]), perstep_min_ade=float(
        step_bk().double().sum(dim=0)[0] / fs[2]), ade=float(fs[3] / fs[2]))

    ta, tb, tc = [[], []], [[], []], [[], []]
    for _ in range(runs):
        for acc, fns, n in ((ta, (fused_bk, comp_bk), max(5, calls // 5)), (tb, (fused_bk, step_bk), calls),
                            (tc, (fused_st, comp_st), calls)):
            got = alternate(fns, n, warmup)
            acc[0].append(got[0])
            acc[1].append(got[1])
    out = dict(S=S, F=F, Nmax=Nmax, K=K, pairs=int(b.n_active.sum()) * F, calls=calls, runs=runs, **mins)
    for key, acc, names in (("a", ta, ("fused_us", "sample_torch_us")), ("b", tb, ("fullcov_us", "perstep_us")),
                            ("c", tc, ("fused_us", "torch_us"))):
        (m0, s0), (m1, s1) = summary(acc[0]), summary(acc[1])
        out[key] = {names[0]: m0, names[0] + "_p10_p90": s0, names[1]: m1, names[1] + "_p10_p90": s1,
                    "ratio": round(m1 / m0, 3) if key != "b" else round(m0 / m1, 3)}
    nbytes = pred.numel() * 4 + targets.numel() * 4
    out["c"]["fused_gb_per_s"] = round(nbytes / (out["c"]["fused_us"] * 1e-6) / 1e9, 1)
    out["paths_max_rel_diff"] = dict(best_of_k=e_bk, stats=e_st)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_fullcov: needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {n: time_shape(n, SHAPES[n]["S"], SHAPES[n]["Nmax"], a.k, a.calls, a.warmup, a.runs, dev)
           for n in a.shapes}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
