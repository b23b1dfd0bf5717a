"""Time the scene-coupled head's launches (coupled.CoupledHead;
csrc/g2k_coupled.hip, g2k_joint.hip, g2k_couples.hip):

  stats          g2k_coupled_stats_f32 with a whitener against the same sums in
                 torch float64 (the groups' means, SSW and SSB as two einsums,
                 y = A r and the five sums of the NLLs)
  couple_scores  g2k_coupled_couple_scores_f32 against (a) the composition it
                 replaces, K sampler launches and tools/time_couple_scores.py's
                 torch scoring, and (b) its twin g2k_fullcov_couple_scores_f32
  joint_eval     g2k_coupled_joint_eval_f32 against (a) K sampler launches and
                 tools/time_fullcov_joint.py's torch composition, and (b) its
                 twin g2k_fullcov_joint_eval_f32

  python tools/time_coupled.py [--calls 50] [--warmup 5] [--runs 3] [--k 20] [--radius 0.05]

Shapes: the real-data evaluation's (F 1, S 384 scenes, Nmax 32, n_active 2..32)
and dense_crowd's (S 64, F 20, Nmax 256), synthetic.make_batch; pred = the
targets + N(0, 0.05^2).  The head cuts the full-covariance timing head's law
(sigma 0.05, AR(1) 0.7 over the steps) in two, share 0.6; the twin draws that
law whole.  The paths of a comparison run in one process, alternating call by
call, each call between its own pair of device events (the compositions take a
fifth of the calls: they are slow); per run the median and the 10th..90th
percentile, and the reported figure is the median of the runs'.  Before timing,
the paths of a comparison must agree: the sums to 1e-9 (stats), the counts
exactly and the float sums to 1e-4 (couple scores), the JADE / JFDE sums to 1e-4
and the collision totals to 1e-3 (joint).  Prints one JSON line.  Needs a GPU:
there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from multimodaltraj_2_amd import couples as cp               # noqa: E402
from multimodaltraj_2_amd.coupled import CoupledHead         # noqa: E402
from multimodaltraj_2_amd.fullcov import FullCovHead         # noqa: E402
from multimodaltraj_2_amd.synthetic import make_batch        # noqa: E402
from time_couple_scores import unfused as unfused_couples    # noqa: E402
from time_fullcov_joint import alternate, summary            # noqa: E402
from time_fullcov_joint import unfused as unfused_joint      # noqa: E402

SHAPES = {"realdata_eval": dict(S=384, F=1, Nmax=32),
          "dense_crowd": dict(S=64, F=20, Nmax=256)}
SIGMA, SHARE = 0.05, 0.6


def torch_stats(pred, targets, mem, A, lam):
    """The stats launch's sums in torch float64 -> (within, between, [q_within,
    independent, q_between, logs])."""
    S, F, _, N = pred.shape
    mu = torch.stack([pred[:, :, :12], pred[:, :, 12:]], dim=-1).permute(0, 1, 3, 2, 4)   # [S, F, N, 12, 2]
    w = mem.to(torch.float64)[..., None]
    r = (targets.double() - mu.double()).reshape(S, F, N, 24) * w
    P = w.sum(dim=2)                                                     # [S, F, 1]
    rbar = r.sum(dim=2) / P.clamp(min=1.0)                                 # [S, F, 24]
    e = (r - rbar[:, :, None]) * w
    within = torch.einsum("sfni,sfnj->ij", e, e)
    between = torch.einsum("sfi,sfj->ij", rbar * P, rbar)
    y, yb = e @ A.T, rbar @ A.T
    qw = (y * y).sum()
    qi = (((y + yb[:, :, None]) ** 2 / (1.0 + lam)) * w).sum()
    qb = (P * yb * yb / (1.0 + P * lam)).sum()
    lg = (torch.log1p(P * lam) * (P > 0)).sum()
    return within, between, torch.stack([qw, qi, qb, lg])


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
    T = 0.7 ** np.abs(np.subtract.outer(np.arange(12), np.arange(12)))
    chol = np.linalg.cholesky(SIGMA * SIGMA * np.kron(T, np.eye(2))).astype(np.float32)
    fc = FullCovHead(device=dev)
    fc.chol = torch.from_numpy(chol).to(dev)
    co = CoupledHead.from_fullcov(fc, SHARE)
    A, lam = (torch.from_numpy(v).to(dev) for v in co.whitener())
    B = cp.auto_bins(K)
    seed = 1234
    out = dict(S=S, F=F, Nmax=Nmax, K=K, B=B, radius=radius, calls=calls, runs=runs)

    def timed(fns, slow):
        acc = [[] for _ in fns]
        for _ in range(runs):
            t = alternate(fns, max(5, calls // 5) if slow else calls, min(warmup, 2) if slow else warmup)
            for a, v in zip(acc, t):
                a.append(v)
        return [summary(a) for a in acc]

    # ---- stats ----
    def st_fused():
        return co.stats(pred, targets, n_active)

    def st_torch():
        return torch_stats(pred, targets, mem, A, lam)
    got, want = st_fused(), st_torch()
    torch.cuda.synchronize()
    rel = lambda a, w: float(((a - w).abs() / w.abs().clamp(min=1.0)).max())   # noqa: E731
    err = max(rel(got.within, want[0]), rel(got.between, want[1]), rel(got.stats[2], want[2][0]),
              rel(got.stats[3], want[2][2]), rel(got.stats[4], want[2][3]))
    if err > 1e-9:
        raise SystemExit(f"{name}: the stats launch and torch disagree ({err:.3g})")
    (f0, fs), (t0, ts) = timed((st_fused, st_torch), False)
    out["stats"] = dict(fused_us=f0, fused_us_p10_p90=fs, torch_us=t0, torch_us_p10_p90=ts,
                        ratio=round(t0 / f0, 2), pairs=got.pairs, groups=got.groups, nll_gain=got.nll_gain,
                        paths_max_rel_diff=err)

    # ---- couple scores ----
    def cs_fused():
        return co.couple_scores(pred, targets, n_active, K, B, seed=seed)

    def cs_twin():
        return fc.couple_scores(pred, targets, n_active, K, B, seed=seed)

    def cs_parent():
        return unfused_couples(co, pred, targets, couples, K, B, seed)
    got, want = cs_fused(), cs_parent()
    torch.cuda.synchronize()
    err = float(((got.sums - want[0]).abs() / want[0].abs().clamp(min=1.0)
                 / got.tot[:, :1].clamp(min=1).to(torch.float32)).max())
    same = torch.equal(got.tot[:, :3], want[2]) and torch.equal(got.hist.to(torch.int64), want[1])
    if err > 1e-4 or not same:
        raise SystemExit(f"{name}: couple scores: the two paths disagree (sums {err:.3g}, counts equal: {same})")
    (a0, sa0), (a1, sa1) = timed((cs_fused, cs_parent), True)
    (b0, sb0), (b1, sb1) = timed((cs_fused, cs_twin), False)
    out["couple_scores"] = dict(fused_us=b0, fused_us_p10_p90=sb0, fullcov_twin_us=b1, fullcov_twin_us_p10_p90=sb1,
                                over_twin=round(b0 / b1, 3), fused_next_to_unfused_us=a0,
                                fused_next_to_unfused_us_p10_p90=sa0, unfused_us=a1, unfused_us_p10_p90=sa1,
                                ratio=round(a1 / a0, 2), couples=got.couples, dev_fin=got.dev("fin"),
                                geometry=cp.couple_scores_geometry(S, F, Nmax, K), paths_max_rel_diff=err)

    # ---- joint evaluation ----
    def je_fused():
        return co.joint_eval(pred, targets, n_active, K, radius, seed=seed, want_per_frame=False)

    def je_twin():
        return fc.joint_eval(pred, targets, n_active, K, radius, seed=seed, want_per_frame=False)

    def je_parent():
        return unfused_joint(co, pred, targets, members, couples, K, radius, seed)
    got, want = je_fused(), je_parent()
    torch.cuda.synchronize()
    err = max(float(((got.sums_f[:, i] - want[i]).abs() / want[i].abs().clamp(min=1.0)).max()) for i in (0, 1))
    cg, cw = int(got.sums_i[:, 4].sum()), int(want[2].sum())
    if err > 1e-4 or abs(cg - cw) > 1e-3 * max(cw, 1):
        raise SystemExit(f"{name}: joint: the two paths disagree (errors {err:.3g}, collisions {cg} / {cw})")
    (a0, sa0), (a1, sa1) = timed((je_fused, je_parent), True)
    (b0, sb0), (b1, sb1) = timed((je_fused, je_twin), False)
    out["joint_eval"] = dict(fused_us=b0, fused_us_p10_p90=sb0, fullcov_twin_us=b1, fullcov_twin_us_p10_p90=sb1,
                             over_twin=round(b0 / b1, 3), fused_next_to_unfused_us=a0,
                             fused_next_to_unfused_us_p10_p90=sa0, unfused_us=a1, unfused_us_p10_p90=sa1,
                             ratio=round(a1 / a0, 2), pairs=got.pairs, jade=got.jade,
                             collision_rate=got.collision_rate, collisions_fused=cg, collisions_composed=cw,
                             paths_max_rel_diff=err)
    return out


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
        raise SystemExit("time_coupled: needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {n: time_shape(n, SHAPES[n]["S"], SHAPES[n]["F"], SHAPES[n]["Nmax"], a.k, a.radius, a.calls,
                         a.warmup, a.runs, dev) for n in a.shapes}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
