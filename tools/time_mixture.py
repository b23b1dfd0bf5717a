"""Time the Gaussian-mixture trajectory head's fused calls (csrc/g2k_mix.hip,
the MixHead policy of csrc/g2k_head_draw.h) against their compositions, to
tools/time_fullcov.py's protocol:

  (a) one EM iteration (g2k_mix_em_f32: E-step and M-step, three launches)
      against the same step composed in torch float64 (residuals, a triangular
      solve per live component, logsumexp, the weighted Grams, the Cholesky),
  (b) g2k_mix_best_of_k_f32 against K g2k_mix_sample_f32 launches with the
      errors and the running minimum in torch,
  (c) g2k_mix_best_of_k_f32 against g2k_fullcov_best_of_k_f32 at the same shape
      and K: what the per-lane factor reads (and the selector) cost.

  python tools/time_mixture.py [--calls 50] [--warmup 5] [--runs 3] [--k 20] [--live 3 8]

Shapes: eth_hotel_synth (S 256, Nmax 32) and one rank's share of dense_crowd
(S 128 of 1024 over 8 GPUs, Nmax 256), F 20, synthetic.make_batch; pred = the
targets + a random-walk residual around one of the components' offsets.  The
paths of a comparison run in one process, alternating call by call, each call
between its own pair of device events; a run's figure is its median, the
spread its 10th..90th percentile, and the reported figure is the median of the
runs'.  Prints one JSON line.  Needs a GPU: there is no fallback.
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
from multimodaltraj_2_amd.mixture import OFF_B, OFF_L, PITCH, SLOTS, MixtureHead   # noqa: E402
from multimodaltraj_2_amd.synthetic import CONFIGS, FRAMES_PER_SCENE, make_batch   # noqa: E402
from tools.time_fullcov import alternate, summary                           # noqa: E402

SHAPES = {"eth_hotel_synth": dict(S=CONFIGS["eth_hotel_synth"]["S"], Nmax=32),
          "dense_crowd": dict(S=CONFIGS["dense_crowd"]["S"] // 8, Nmax=256)}
SIGMA = 0.05


def composed_best_of_k(mx, pred, targets, pairs, K, seed):
    """K sampler launches, the errors and the running minimum in torch ->
    (sum minADE, sum minFDE) over the pairs."""
    tx, ty = targets[..., 0].permute(0, 1, 3, 2), targets[..., 1].permute(0, 1, 3, 2)   # [S, F, 12, N]
    bA = bF = None
    for k in range(K):
        x = mx.sample(pred, seed=seed + k)
        d = torch.sqrt((x[:, :, :12] - tx) ** 2 + (x[:, :, 12:] - ty) ** 2)
        ade, fde = d.mean(dim=2), d[:, :, 11]
        bA = ade if bA is None else torch.minimum(bA, ade)
        bF = fde if bF is None else torch.minimum(bF, fde)
    return (bA * pairs).sum(), (bF * pairs).sum()


def composed_em(params, live, pred, targets, pairs):
    """One EM step in torch, float64 -> (new block [8, 608] float32, sum of the
    log density, N [8])."""
    S, F, _, N = pred.shape
    p = pred.view(S, F, 2, 12, N).permute(0, 1, 4, 3, 2).double()      # [S, F, N, 12, 2]
    on = pairs.reshape(-1) > 0
    r = (targets.double() - p).reshape(-1, 24)[on]
    n = r.shape[0]
    w = params[:, 0].double()
    lms = []
    for m in live:
        Lm = torch.tril(params[m, OFF_L:].view(24, 24).double())
        z = torch.linalg.solve_triangular(Lm, (r - params[m, OFF_B:OFF_L].double()).t(), upper=False)
        lms.append(torch.log(w[m] / w.sum()) - 12 * math.log(2 * math.pi) -
                   torch.log(torch.diagonal(Lm)).sum() - 0.5 * (z * z).sum(dim=0))
    lm = torch.stack(lms, dim=1)
    l = torch.logsumexp(lm, dim=1)
    g = torch.exp(lm - l[:, None])
    out = torch.zeros((SLOTS, PITCH), dtype=torch.float32, device=pred.device)
    Ns = torch.zeros(SLOTS, dtype=torch.float64, device=pred.device)
    eye = torch.eye(24, dtype=torch.float64, device=pred.device)
    for i, m in enumerate(live):
        Nm = g[:, i].sum()
        b = (g[:, i] @ r) / Nm
        C = (r * g[:, i, None]).t() @ r / Nm - torch.outer(b, b)
        C = C + eye * (torch.diagonal(C) * 1e-6 + 1e-12)
        out[m, 0] = (Nm / n).float()
        out[m, OFF_B:OFF_L] = b.float()
        out[m, OFF_L:] = torch.linalg.cholesky(C).float().reshape(-1)
        Ns[m] = Nm
    return out, l.sum(), Ns


def make_block(live, dev):
    """``live`` components: the random walk's factor scaled 0.7 .. 1.3 and
    offsets along the walk's leading direction, weights 1 / M."""
    Lw = np.zeros((24, 24), np.float32)
    for t in range(12):
        for u in range(t + 1):
            Lw[2 * t, 2 * u] = Lw[2 * t + 1, 2 * u + 1] = SIGMA
    M = len(live)
    p = np.zeros((SLOTS, PITCH), np.float32)
    ramp = np.repeat(np.sqrt(np.arange(1, 13, dtype=np.float64)), 2)
    for i, m in enumerate(live):
        p[m, 0] = 1.0 / M
        p[m, OFF_B:OFF_L] = SIGMA * ramp * (2.0 * (i - (M - 1) / 2.0))
        p[m, OFF_L:] = (Lw * (0.7 + 0.6 * i / max(1, M - 1))).reshape(-1)
    return torch.from_numpy(p).to(dev), Lw


def time_shape(name, S, Nmax, K, M, calls, warmup, runs, dev):
    F = FRAMES_PER_SCENE
    b = make_batch(S, Nmax, 64, F=F, seed=5)
    rng = np.random.default_rng(6)
    live = list(range(M))
    block, Lw = make_block(live, dev)
    blk = block.cpu().numpy()
    k = rng.integers(0, M, (S, F, 1, 1, Nmax))
    walk = SIGMA * np.cumsum(rng.standard_normal((S, F, 2, 12, Nmax)), axis=3)
    off = blk[:M, OFF_B:OFF_L].reshape(M, 12, 2).transpose(0, 2, 1)          # [M, 2, 12]
    walk = walk + np.take(off, k[:, :, 0, 0, :], axis=0).transpose(0, 1, 3, 4, 2)
    pred_h = (np.transpose(b.targets, (0, 1, 4, 3, 2)).reshape(S, F, 24, Nmax) -
              walk.reshape(S, F, 24, Nmax)).astype(np.float32)
    pred = torch.from_numpy(pred_h).to(dev)
    targets = torch.from_numpy(b.targets).to(dev)
    n_active = torch.from_numpy(b.n_active).to(dev)
    pm = (torch.arange(Nmax, device=dev)[None, None, :] < n_active[:, None, None]).expand(S, F, Nmax)
    pairs32 = pm.float().contiguous()
    mx = MixtureHead.from_block(block)
    fc = FullCovHead(device=dev)
    fc.chol = torch.from_numpy(Lw).to(dev)
    seed = 11

    def fused_em():
        h = MixtureHead.from_block(block)
        st = h.em_step(pred, targets, n_active)
        return h.params, st

    def comp_em():
        return composed_em(block, live, pred, targets, pairs32)

    def fused_bk():
        return mx.best_of_k(pred, targets, n_active, K, seed=seed, want_per_ped=False).sums

    def comp_bk():
        return composed_best_of_k(mx, pred, targets, pairs32, K, seed)

    def fullcov_bk():
        return fc.best_of_k(pred, targets, n_active, K, seed=seed, want_per_ped=False).sums

    # the paths agree before they are timed
    fs, (ca, cf) = fused_bk().double().sum(dim=0), comp_bk()
    e_bk = max(abs(float(fs[0]) - float(ca)) / float(ca), abs(float(fs[1]) - float(cf)) / float(cf))
    (newp, st), (cp, cl, cN) = fused_em(), comp_em()
    torch.cuda.synchronize()
    e_em = max(abs(float(st.total[1]) - float(cl)) / max(1.0, abs(float(cl))),
               float(((st.resp[:, 0] - cN).abs() / cN.abs().clamp(min=1.0)).max()))
    e_w = float((newp[:, :OFF_L] - cp[:, :OFF_L]).abs().max())
    if e_bk > 1e-4 or e_em > 1e-9 or e_w > 1e-5:
        raise SystemExit(f"{name} M={M}: the paths disagree (best-of-K {e_bk:.3g}, EM {e_em:.3g}, "
                         f"new w / b {e_w:.3g})")
    mins = dict(mix_min_ade=float(fs[0] / fs[2]), fullcov_min_ade=float(
        fullcov_bk().double().sum(dim=0)[0] / fs[2]), ade=float(fs[3] / fs[2]),
        loglik=float(st.total[1] / st.total[0]))

    ta, tb, tc = [[], []], [[], []], [[], []]
    for _ in range(runs):
        for acc, fns, n in ((ta, (fused_em, comp_em), calls), (tb, (fused_bk, comp_bk), max(5, calls // 5)),
                            (tc, (fused_bk, fullcov_bk), calls)):
            got = alternate(fns, n, warmup)
            acc[0].append(got[0])
            acc[1].append(got[1])
    out = dict(S=S, F=F, Nmax=Nmax, K=K, live=M, pairs=int(b.n_active.sum()) * F, calls=calls, runs=runs,
               **mins)
    for key, acc, names in (("a", ta, ("fused_us", "torch_us")), ("b", tb, ("fused_us", "sample_torch_us")),
                            ("c", tc, ("mix_us", "fullcov_us"))):
        (m0, s0), (m1, s1) = summary(acc[0]), summary(acc[1])
        out[key] = {names[0]: m0, names[0] + "_p10_p90": s0, names[1]: m1, names[1] + "_p10_p90": s1,
                    "ratio": round(m1 / m0, 3) if key != "c" else round(m0 / m1, 3)}
    out["paths_max_rel_diff"] = dict(best_of_k=e_bk, em=e_em, new_w_b=e_w)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--live", type=int, nargs="*", default=[3, 8])
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_mixture: needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    out = {f"{n}_m{M}": time_shape(n, SHAPES[n]["S"], SHAPES[n]["Nmax"], a.k, M, a.calls, a.warmup,
                                   a.runs, dev)
           for n in a.shapes for M in a.live}
    out["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
