"""Time the Gaussian-mixture head's fused joint best-of-K and KDE-NLL
(g2k_mix_joint_eval_f32, g2k_mix_kde_nll_f32) against (a) the composition each
replaces — K x MixtureHead.sample and the same figures in torch (the
compositions of tools/time_fullcov_joint.py and tools/time_kde_nll.py) — and
(b) the full-covariance head's fused call at the same shape and K.

  python tools/time_mixture_eval.py [--calls 50] [--warmup 5] [--runs 3] [--k 20]
                                    [--slots 3 8] [--what joint kde] [--shapes ...]

Shapes: joint — tools/time_fullcov_joint.py's (realdata_eval: S 384, F 1, Nmax
32; dense_crowd: S 64, F 20, Nmax 256); KDE — tools/time_kde_nll.py's
(eth_hotel_synth: S 256, F 20, Nmax 32; dense_crowd: S 128, F 20, Nmax 256) and
realdata_eval.  synthetic.make_batch; pred = the targets + N(0, 0.05^2).  The
mixture has ``slots`` live components (the first ones) with weights U(0.2, 1),
b = 1.5 x 0.05 N(0, 1) and, as every factor, the full-covariance head's of (b):
the random walk of tools/time_fullcov_joint.py for the joint figures, the
AR(1) 0.7 factor of tools/time_kde_nll.py for the KDE.  The paths of a
comparison run in one process, alternating call by call, each call between its
own pair of device events ((a) takes a fifth of the calls: its composition is
slow); per run the median and the 10th..90th percentile, and the reported
figure is the median of the runs' medians with the widest 10th..90th range.
Before timing the two paths of (a) must agree (JADE / JFDE sums and the KDE
sums to 1e-3, collision totals to 1e-3).  Prints one JSON line.  Needs a GPU:
there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_fullcov_joint import alternate, summary, unfused            # noqa: E402
from time_kde_nll import composed as kde_composed                      # noqa: E402
from multimodaltraj_2_amd.fullcov import FullCovHead                   # noqa: E402
from multimodaltraj_2_amd.mixture import OFF_B, OFF_L, PITCH, SLOTS, MixtureHead   # noqa: E402
from multimodaltraj_2_amd.synthetic import make_batch                  # noqa: E402

JOINT_SHAPES = {"realdata_eval": dict(S=384, F=1, Nmax=32), "dense_crowd": dict(S=64, F=20, Nmax=256)}
KDE_SHAPES = {"eth_hotel_synth": dict(S=256, F=20, Nmax=32), "dense_crowd": dict(S=128, F=20, Nmax=256),
              "realdata_eval": dict(S=384, F=1, Nmax=32)}
SIGMA, AR = 0.05, 0.7


def walk_factor():
    step = SIGMA / np.sqrt(12.0)
    Lw = np.zeros((24, 24), np.float32)
    for t in range(12):
        for u in range(t + 1):
            Lw[2 * t, 2 * u] = Lw[2 * t + 1, 2 * u + 1] = step
    return Lw


def ar_factor():
    T = AR ** np.abs(np.subtract.outer(np.arange(12), np.arange(12)))
    return (SIGMA * np.linalg.cholesky(np.kron(T, np.eye(2)))).astype(np.float32)


def mixture_of(chol, slots, dev):
    rng = np.random.default_rng(7 + slots)
    p = np.zeros((SLOTS, PITCH), np.float32)
    p[:slots, 0] = rng.uniform(0.2, 1.0, slots)
    p[:slots, OFF_B:OFF_L] = 1.5 * SIGMA * rng.standard_normal((slots, 24))
    p[:slots, OFF_L:] = np.tril(chol).reshape(-1)
    return MixtureHead.from_block(p, device=dev)


def batch(S, F, Nmax, dev):
    b = make_batch(S, Nmax, 64, F=F, seed=5)
    rng = np.random.default_rng(6)
    pred_h = (np.transpose(b.targets, (0, 1, 4, 3, 2)).reshape(S, F, 24, Nmax)
              + SIGMA * rng.standard_normal((S, F, 24, Nmax))).astype(np.float32)
    pred = torch.from_numpy(pred_h).to(dev)
    n_active = torch.from_numpy(b.n_active).to(dev)
    mem = (torch.arange(Nmax, device=dev)[None, None, :] < n_active[:, None, None]).expand(S, F, Nmax)
    return pred, torch.from_numpy(b.targets).to(dev), n_active, mem


def compare(fused, composed, other, calls, warmup, runs):
    """-> the two comparisons' summaries: (a) fused vs composed, (b) fused vs
    the other head's fused call."""
    ta, tb = [[], []], [[], []]
    for _ in range(runs):
        for acc, fns, n, wu in ((ta, (fused, composed), max(5, calls // 5), min(warmup, 2)),
                                (tb, (fused, other), calls, warmup)):
            t = alternate(fns, n, wu)
            acc[0].append(t[0])
            acc[1].append(t[1])
    (a0, sa0), (a1, sa1) = summary(ta[0]), summary(ta[1])
    (b0, sb0), (b1, sb1) = summary(tb[0]), summary(tb[1])
    return dict(a=dict(fused_us=a0, fused_us_p10_p90=sa0, sample_torch_us=a1, sample_torch_us_p10_p90=sa1,
                       ratio=round(a1 / a0, 2)),
                b=dict(mixture_us=b0, mixture_us_p10_p90=sb0, fullcov_us=b1, fullcov_us_p10_p90=sb1,
                       ratio=round(b0 / b1, 3)))


def time_joint(name, S, F, Nmax, slots, K, radius, calls, warmup, runs, dev):
    pred, targets, n_active, mem = batch(S, F, Nmax, dev)
    couples = (mem[:, :, :, None] & mem[:, :, None, :]
               & torch.ones((Nmax, Nmax), dtype=torch.bool, device=dev).triu(1)).contiguous()
    members = mem.to(torch.float32).contiguous()
    fc = FullCovHead(device=dev)
    fc.chol = torch.from_numpy(walk_factor()).to(dev)
    mx = mixture_of(walk_factor(), slots, dev)
    seed = 1234

    def fused():
        return mx.joint_eval(pred, targets, n_active, K, radius, seed=seed, want_per_frame=False)

    def composed():
        return unfused(mx, pred, targets, members, couples, K, radius, seed)

    def fullcov():
        return fc.joint_eval(pred, targets, n_active, K, radius, seed=seed, want_per_frame=False)

    got, want, other = fused(), composed(), fullcov()
    torch.cuda.synchronize()
    err = max(float(((got.sums_f[:, i] - want[i]).abs() / want[i].abs().clamp(min=1.0)).max())
              for i in (0, 1))
    cg, cw = int(got.sums_i[:, 4].sum()), int(want[2].sum())
    if err > 1e-3 or abs(cg - cw) > 1e-3 * max(cw, 1):
        raise SystemExit(f"{name}: the two paths disagree (errors {err:.3g}, collisions {cg} / {cw})")
    if not torch.equal(got.sums_i[:, :4], other.sums_i[:, :4]):
        raise SystemExit(f"{name}: the head-independent columns differ between the two fused calls")
    out = dict(S=S, F=F, Nmax=Nmax, K=K, slots=slots, radius=radius, pairs=got.pairs,
               couples=got.ped_pairs, calls=calls, runs=runs)
    out.update(compare(fused, composed, fullcov, calls, warmup, runs))
    out.update(jade=dict(mixture=got.jade, fullcov=other.jade),
               collision_rate=dict(mixture=got.collision_rate, fullcov=other.collision_rate),
               paths_max_rel_diff=err)
    return out


def time_kde(name, S, F, Nmax, slots, K, floor, calls, warmup, runs, dev):
    pred, targets, n_active, mem = batch(S, F, Nmax, dev)
    pairs = mem.to(torch.float32).contiguous()
    fc = FullCovHead(device=dev)
    fc.chol = torch.from_numpy(ar_factor()).to(dev)
    mx = mixture_of(ar_factor(), slots, dev)
    seed = 1234

    def fused():
        return mx.kde_nll(pred, targets, n_active, K, seed=seed, log_floor=floor).out

    def composed():
        return kde_composed(mx, pred, targets, pairs, K, seed, floor)

    def fullcov():
        return fc.kde_nll(pred, targets, n_active, K, seed=seed, log_floor=floor).out

    got, want, other = fused(), composed(), fullcov()
    torch.cuda.synchronize()
    err = float(((got[:, :2] - want).abs() / want.abs().clamp(min=1.0)).max())
    if err > 1e-3:
        raise SystemExit(f"{name}: the two paths disagree ({err:.3g})")
    n = float(got[:, 2].sum())
    out = dict(S=S, F=F, Nmax=Nmax, K=K, slots=slots, pairs=int(n), calls=calls, runs=runs)
    out.update(compare(fused, composed, fullcov, calls, warmup, runs))
    out.update(kde_nll=dict(mixture=float(got[:, 0].double().sum()) / n,
                            fullcov=float(other[:, 0].double().sum()) / n), paths_max_rel_diff=err)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--radius", type=float, default=0.05)
    ap.add_argument("--floor", type=float, default=-20.0)
    ap.add_argument("--slots", type=int, nargs="*", default=[3, 8])
    ap.add_argument("--what", nargs="*", default=["joint", "kde"])
    ap.add_argument("--shapes", nargs="*", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_mixture_eval: needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {}
    for what, shapes, fn, extra in (("joint", JOINT_SHAPES, time_joint, a.radius),
                                    ("kde", KDE_SHAPES, time_kde, a.floor)):
        if what not in a.what:
            continue
        for name, sh in shapes.items():
            if a.shapes is not None and name not in a.shapes:
                continue
            for slots in a.slots:
                out[f"{what}/{name}/slots{slots}"] = fn(name, sh["S"], sh["F"], sh["Nmax"], slots, a.k, extra,
                                                        a.calls, a.warmup, a.runs, dev)
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
