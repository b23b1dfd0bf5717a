"""The full-covariance trajectory head (csrc/g2k_fullcov.hip): ONE Gaussian
over a pair's whole 24-vector of residuals, coordinate i = 2 t + c (step t,
c = 0 for x, 1 for y), held as the lower Cholesky factor ``chol`` [24, 24] of
the residual covariance.  The per-step head (nll.GaussianHead) is its
block-diagonal special case: it gets every marginal right and draws 12
independent steps, while a draw of this head is a temporally correlated
trajectory.  The build's: the reference has no probabilistic head, so its
parity is unpinned (tests/fullcov_ref.py is the float64 checker).

``stats`` measures a head against the targets in one launch (the residuals'
second moments, the joint NLL, the innovations q_t and their coverage),
``fit`` sets the head to the closed-form maximum-likelihood one, ``sample``
draws one reproducible trajectory per (scene, frame, pedestrian),
``best_of_k`` evaluates K such draws against the targets in one launch,
``kde_nll`` scores the targets under a kernel density estimate of the same
draws (csrc/g2k_kde.hip) and ``joint_eval`` takes them as joint samples of a scene-frame (JADE_K / JFDE_K
and the collision counts, csrc/g2k_joint.hip), also in one launch."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .frame_step import PRED_LEN, _check_dev, _ptr, _stream
from .nll import DEFAULT_LEVELS, MAX_LEVELS, SampledEvals, _check_pairs_inputs

DIM = 2 * PRED_LEN


def chi2_even_quantile(p, dof):
    """The p-quantile of chi^2 with an even number ``dof`` of degrees of
    freedom, float64: bisection on the closed-form CDF
    1 - exp(-x / 2) sum_{j < dof / 2} (x / 2)^j / j!  (dof 2: -2 log1p(-p))."""
    p, dof = float(p), int(dof)
    if dof < 2 or dof % 2:
        raise ValueError(f"dof = {dof}: even and >= 2")
    if not 0.0 < p < 1.0:
        raise ValueError(f"level {p}: 0 < p < 1")
    if dof == 2:
        return -2.0 * math.log1p(-p)
    m = dof // 2

    def tail(x):                                  # 1 - CDF
        h, term, s = 0.5 * x, 1.0, 1.0
        for j in range(1, m):
            term *= h / j
            s += term
        return math.exp(-h) * s
    lo, hi = 0.0, float(dof)
    while tail(hi) > 1.0 - p:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if tail(mid) > 1.0 - p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


@dataclass
class FullCovStats:
    """``FullCovHead.stats``'s outputs (include/g2k_hip.h).  Every property is
    one host read (float64); a figure whose denominator is 0 is NaN, and those
    of a head (nll, coverage, ece_joint, q_ratio) are None when the launch had
    none (``use_head=False``)."""
    moments: torch.Tensor               # [25, 24] float64: M = sum r r^T, then sum r
    stats: torch.Tensor                 # [12, 4] float64 {pairs, S nll_t, S q_t, 0}
    inside: torch.Tensor | None         # [13, NL] int64: q_t <= r2[0][l] per step, then q <= r2[1][l]
    fit_chol: torch.Tensor              # [24, 24] float32: the closed-form factor, written by the device
    levels: tuple = ()
    r2: torch.Tensor | None = None      # [2, NL] float64 on the device
    has_head: bool = True

    def _s(self):
        return self.stats.cpu().numpy()

    @property
    def pairs(self) -> int:
        return int(self.stats[0, 0].item())

    @property
    def fit(self) -> torch.Tensor:
        return self.fit_chol

    @property
    def nll_per_step(self):
        """[12] mean NLL of step t's innovation."""
        if not self.has_head:
            return None
        s = self._s()
        with np.errstate(invalid="ignore", divide="ignore"):
            return s[:, 1] / s[:, 0]

    @property
    def nll(self):
        """The joint NLL per pair (the sum over the 12 steps)."""
        if not self.has_head:
            return None
        s = self._s()
        return float(s[:, 1].sum() / s[0, 0]) if s[0, 0] > 0 else float("nan")

    @property
    def q_ratio(self):
        """sum q / (24 * pairs): 1 under a calibrated head."""
        if not self.has_head:
            return None
        s = self._s()
        return float(s[:, 2].sum() / (DIM * s[0, 0])) if s[0, 0] > 0 else float("nan")

    @property
    def coverage(self):
        """[12, NL]: share of the pairs whose step-t innovation is inside each level."""
        if not self.has_head:
            return None
        n = self._s()[:, :1]
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.inside[:PRED_LEN].cpu().numpy().astype(np.float64) / n

    @property
    def coverage_joint(self):
        """[NL]: share of the pairs whose whole trajectory is inside each level."""
        if not self.has_head:
            return None
        n = self._s()[0, 0]
        tot = self.inside[PRED_LEN].cpu().numpy().astype(np.float64)
        return tot / n if n > 0 else np.full(tot.shape, np.nan)

    @property
    def ece_joint(self):
        """mean over the levels of |coverage_joint - p|."""
        if not self.has_head:
            return None
        if not self.levels:
            return float("nan")
        return float(np.abs(self.coverage_joint - np.asarray(self.levels, np.float64)).mean())

    @property
    def cov(self):
        """[24, 24]: M / pairs, the residuals' uncentred second moments."""
        n = self._s()[0, 0]
        m = self.moments[:DIM].cpu().numpy()
        return m / n if n > 0 else np.full(m.shape, np.nan)

    @property
    def step_corr(self):
        """[12, 12]: correlation of the x-residuals between the steps."""
        c = self.cov[0::2, 0::2]
        d = np.sqrt(np.diag(c))
        with np.errstate(invalid="ignore", divide="ignore"):
            return c / np.outer(d, d)

    @property
    def lag1_corr(self) -> float:
        """Mean correlation of the x-residuals at adjacent steps."""
        return float(np.diag(self.step_corr, 1).mean())


class FullCovHead(SampledEvals):
    """The full-covariance head.  Its sampled evaluations (nll.SampledEvals)
    are GaussianHead's over this head's temporally correlated draws
    ``sample(pred, seed + i)``, i < k: ``best_of_k`` is
    g2k_fullcov_best_of_k_f32, ``kde_nll`` g2k_fullcov_kde_nll_f32,
    ``joint_eval`` g2k_fullcov_joint_eval_f32 (GPU tensors only),
    ``sample_scores`` g2k_fullcov_sample_scores_f32 and ``sample_modes``
    g2k_fullcov_sample_modes_f32."""
    _PREFIX = "g2k_fullcov_"
    _JOINT_GPU_ONLY = True

    def __init__(self, device="cuda"):
        self.chol = torch.eye(DIM, dtype=torch.float32, device=device)

    @classmethod
    def from_gaussian_head(cls, head, device=None):
        """The block-diagonal factor of a per-step head [3, 12] (log sigma_x,
        log sigma_y, atanh rho): blocks {sx, 0; sy rho, sy sqrt(1 - rho^2)},
        formed in float64 on the host and rounded once."""
        h = head.detach().cpu().double().numpy() if isinstance(head, torch.Tensor) else \
            np.asarray(head, np.float64)
        if h.shape != (3, PRED_LEN):
            raise ValueError(f"head must be [3, {PRED_LEN}]")
        sx, sy, rho = np.exp(h[0]), np.exp(h[1]), np.tanh(h[2])
        L = np.zeros((DIM, DIM))
        for t in range(PRED_LEN):
            L[2 * t, 2 * t] = sx[t]
            L[2 * t + 1, 2 * t] = sy[t] * rho[t]
            L[2 * t + 1, 2 * t + 1] = sy[t] * np.sqrt(1.0 - rho[t] * rho[t])
        if device is None:
            device = head.device if isinstance(head, torch.Tensor) else "cuda"
        fc = cls.__new__(cls)
        fc.chol = torch.from_numpy(L.astype(np.float32)).to(device)
        return fc

    def _check_chol(self, dev):
        if tuple(self.chol.shape) != (DIM, DIM):
            raise ValueError(f"chol must be [{DIM}, {DIM}]")
        _check_dev("chol", self.chol, dev, torch.float32)

    def _head_tensor(self, dev):
        self._check_chol(dev)
        return self.chol

    def _r2(self, levels, dev):
        """[2, NL] float64 on ``dev``: the levels' chi^2(2) radii (a step's
        innovation) and chi^2(24) radii (the whole trajectory); formed on the
        host once per set of levels."""
        cache = self.__dict__.setdefault("_r2_cache", {})
        key = (levels, str(dev))
        if key not in cache:
            cache.clear()
            r2 = [[chi2_even_quantile(p, 2) for p in levels],
                  [chi2_even_quantile(p, DIM) for p in levels]]
            cache[key] = torch.tensor(r2, dtype=torch.float64).to(dev)
        return cache[key]

    def stats(self, pred, targets, n_active, levels=DEFAULT_LEVELS, *, n_frames=None, ped_mask=None,
              targets_shared=False, use_head=True, stream=None):
        """One launch (g2k_fullcov_stats_f32): the residuals' second moments
        over the pairs and their closed-form factor (``fit``), and, with
        ``use_head``, this head's joint NLL, the innovations q_t = z[2t]^2 +
        z[2t+1]^2 of z = L^-1 r and the pairs inside the ``levels`` (level p:
        q_t <= the chi^2(2) quantile, q <= the chi^2(24) one) -> FullCovStats."""
        levels = tuple(float(p) for p in levels) if use_head else ()
        if len(levels) > MAX_LEVELS:
            raise ValueError(f"{len(levels)} levels: {MAX_LEVELS} at most")
        for p in levels:
            if not 0.0 < p < 1.0:
                raise ValueError(f"level {p}: 0 < p < 1")
        lib = _lib.load()
        dev = pred.device
        d = self._dims(pred)
        _check_pairs_inputs(d, pred, targets, n_active, n_frames, ped_mask, targets_shared)
        if use_head:
            self._check_chol(dev)
        nl = len(levels)
        r2 = self._r2(levels, dev) if nl else None
        # S = 0 launches nothing: the outputs are the empty launch's (zeros, the identity)
        make = torch.zeros if d.S == 0 else torch.empty
        moments = make((DIM + 1, DIM), dtype=torch.float64, device=dev)
        stats = make((PRED_LEN, 4), dtype=torch.float64, device=dev)
        inside = make((PRED_LEN + 1, nl), dtype=torch.int64, device=dev) if use_head else None
        fit = torch.eye(DIM, dtype=torch.float32, device=dev) if d.S == 0 else \
            torch.empty((DIM, DIM), dtype=torch.float32, device=dev)
        ws = torch.empty(max(8, int(lib.g2k_fullcov_stats_workspace_bytes(ctypes.byref(d), nl))),
                         dtype=torch.uint8, device=dev)
        rc = lib.g2k_fullcov_stats_f32(ctypes.byref(d), _ptr(pred), _ptr(targets), _ptr(n_active),
                                       _ptr(n_frames), _ptr(ped_mask),
                                       _ptr(self.chol) if use_head else None, _ptr(r2), nl,
                                       _ptr(moments), _ptr(stats), _ptr(inside) if nl else None,
                                       _ptr(fit), _ptr(ws), ws.numel(), _stream(stream))
        _lib.check("g2k_fullcov_stats_f32", rc)
        return FullCovStats(moments=moments, stats=stats, inside=inside, fit_chol=fit, levels=levels,
                            r2=r2, has_head=bool(use_head))

    def fit(self, pred, targets, n_active, *, n_frames=None, ped_mask=None, targets_shared=False,
            stream=None):
        """Set ``self.chol`` to the closed-form maximum-likelihood factor of
        the residuals (one stats launch without a head; the device writes the
        factor) -> that launch's FullCovStats.  ValueError when there is no pair."""
        st = self.stats(pred, targets, n_active, (), n_frames=n_frames, ped_mask=ped_mask,
                        targets_shared=targets_shared, use_head=False, stream=stream)
        if st.pairs == 0:
            raise ValueError("fit: no (scene, frame, pedestrian) pair to fit the head on")
        self.chol = st.fit_chol
        return st

    def sample(self, pred, seed=0, stream=None):
        """One correlated draw around pred [S, F, 2L, Nmax] (same layout out)."""
        lib = _lib.load()
        d = self._dims(pred)
        _check_dev("pred", pred, pred.device, torch.float32)
        self._check_chol(pred.device)
        out = torch.empty_like(pred)
        rc = lib.g2k_fullcov_sample_f32(ctypes.byref(d), _ptr(pred), _ptr(self.chol),
                                        ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), _ptr(out),
                                        _stream(stream))
        _lib.check("g2k_fullcov_sample_f32", rc)
        return out
