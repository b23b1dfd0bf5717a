"""The scene-coupled trajectory head (csrc/g2k_coupled.hip;
include/g2k_coupled.h states the definition): the Gaussian whose JOINT draws
share a part among the pedestrians of a scene-frame.  Over the 24-vector
residuals r (time-major, i = 2 t + c, as fullcov.FullCovHead's)

    r_gi = c_g + e_gi,   c_g ~ N(0, B) one per scene-frame,   e_gi ~ N(0, W) one per member

held as ``cpl`` [2, 24, 24] = {Lw, Lb}, the lower Cholesky factors of W and B.
One member's law is N(mu, W + B), a full-covariance head (``marginal()``); B =
0 is that head itself.  The other heads draw every pedestrian independently, so
``joint_eval`` and ``couple_scores`` only ever saw independent joint laws.

``stats`` takes the within- and between-group sums of the residuals in one
launch and, for a fitted head, the exact joint NLL of the groups next to the
NLL of the independent head with the same marginals: their difference is what
the coupling is worth in nats.  ``fit`` is the closed-form method-of-moments
estimate (one stats launch, then a 24 x 24 projection in float64 on the host),
``sample`` draws one reproducible joint trajectory set, and ``joint_eval`` /
``couple_scores`` / ``scene_ranks`` / ``scene_modes`` are nll.SampledEvals' over
this head's joint draws, one call each.  The per-pedestrian evaluations belong to ``marginal()``.

The entry points were added after ABI 11 and are declared in a header of their
own, so this module binds them itself on the handle ``_lib.load()`` returns
(``SYMBOLS`` below must equal include/g2k_coupled.h)."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, couples, scenemodes, sceneranks
from .frame_step import PRED_LEN, _check_dev, _ptr, _stream
from .nll import SampledEvals, _check_pairs_inputs

DIM = 2 * PRED_LEN
SALT = 0x9E3779B97F4A6000               # G2K_COUPLED_SALT
NCOUNTS, NSTATS = 4, 6
RIDGE_REL, RIDGE_ABS = 1e-6, 1e-12      # g2k_fullcov_stats_f32's fit
LOG_2PI = math.log(2.0 * math.pi)

_D = ctypes.POINTER(_lib.G2KDims)
_vp, _i64, _int, _i32, _u64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int32, ctypes.c_uint64
# exported symbol -> (restype, argtypes); must match include/g2k_coupled.h
SYMBOLS = {
    "g2k_coupled_stats_workspace_bytes": (_i64, [_D]),
    "g2k_coupled_stats_f32": (_int, [_D, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "g2k_coupled_sample_f32": (_int, [_D, _vp, _vp, _u64, _vp, _vp]),
    "g2k_coupled_joint_eval_workspace_bytes": (_i64, [_D]),
    "g2k_coupled_joint_eval_f32": (_int, [_D, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _i32, ctypes.c_float, _vp,
                                          _vp, _vp, _vp, _vp, _i64, _vp]),
    "g2k_coupled_couple_scores_f32": couples._CPL,
    "g2k_coupled_scene_ranks_f32": sceneranks._SCN,
    "g2k_coupled_scene_modes_f32": scenemodes._SMD,
}


def load():
    """``_lib.load()``'s handle with this header's symbols bound (once); a
    library without them is an error, there is no fallback."""
    return _lib.bind(_lib.load(), "coupled", SYMBOLS)


def ridged(C):
    """C with the full-covariance fit's ridge on its diagonal (float64)."""
    C = np.array(C, np.float64)
    i = np.arange(C.shape[0])
    C[i, i] = C[i, i] * (1.0 + RIDGE_REL) + RIDGE_ABS
    return C


def project(W, B_raw):
    """The host half of the fit, float64: W [24, 24] (ridged, positive
    definite) and the raw, possibly indefinite B_raw -> (Lw, Lb, A, lam,
    clipped): Lw = chol(W); Lw^-1 B_raw Lw^-T = V diag(l) V^T; lam = max(l, 0),
    ``clipped`` how many l were negative; B = Lw V diag(lam) V^T Lw^T and Lb =
    chol(ridged B), zeros when every lam is 0; A = V^T Lw^-1, so that A W A^T =
    I and A B A^T = diag(lam)."""
    Lw = np.linalg.cholesky(W)
    Li = np.linalg.inv(Lw)
    M = Li @ B_raw @ Li.T
    l, V = np.linalg.eigh(0.5 * (M + M.T))
    clipped = int((l < 0.0).sum())
    lam = np.maximum(l, 0.0)
    if lam.max() > 0.0:
        H = Lw @ V
        Lb = np.linalg.cholesky(ridged((H * lam) @ H.T))
    else:
        Lb = np.zeros_like(Lw)
    return Lw, Lb, V.T @ Li, lam, clipped


def whiten_of(Lw, Lb):
    """(A, lam) of given factors, float64: the projection of B = Lb Lb^T
    (already positive semi-definite: nothing is clipped but rounding)."""
    Lw, Lb = np.tril(np.asarray(Lw, np.float64)), np.tril(np.asarray(Lb, np.float64))
    Li = np.linalg.inv(Lw)
    M = Li @ (Lb @ Lb.T) @ Li.T
    l, V = np.linalg.eigh(0.5 * (M + M.T))
    return V.T @ Li, np.maximum(l, 0.0)


@dataclass
class CoupledStats:
    """``CoupledHead.stats``'s outputs (include/g2k_coupled.h).  Every property
    is one host read (float64); a figure whose denominator is 0 is NaN, and
    those of a head (nll, nll_independent, nll_gain, the q ratios) are None when
    the launch had none (``use_head=False``)."""
    within: torch.Tensor                # [24, 24] float64: SSW
    between: torch.Tensor               # [24, 24] float64: SSB
    counts: torch.Tensor                # [4] int64 {N, G, groups with P >= 2, sum P^2}
    stats: torch.Tensor                 # [6] float64 {S nll, S nll of the independent head, q_within, q_between, logs, 0}
    log_det_lw: float = 0.0
    has_head: bool = True

    def _c(self):
        return [int(v) for v in self.counts.tolist()]

    @property
    def pairs(self) -> int:
        return self._c()[0]

    @property
    def groups(self) -> int:
        return self._c()[1]

    @property
    def W(self):
        """[24, 24]: SSW / (N - G), the members' own covariance (unridged)."""
        n, g = self._c()[:2]
        m = self.within.cpu().numpy()
        return m / (n - g) if n > g else np.full(m.shape, np.nan)

    @property
    def B_raw(self):
        """[24, 24]: (SSB - G W) / N, the shared part's covariance before the
        projection; it may be indefinite."""
        n, g = self._c()[:2]
        m = self.between.cpu().numpy()
        return (m - g * self.W) / n if n > g else np.full(m.shape, np.nan)

    @property
    def share(self) -> float:
        """tr B_raw / tr(W + B_raw): the part of the residual variance that a
        scene-frame's members share."""
        w, b = np.trace(self.W), np.trace(self.B_raw)
        return float(b / (w + b))

    def _per_pair(self, i):
        if not self.has_head:
            return None
        n = self.pairs
        if n == 0:
            return float("nan")
        return float(self.stats[i].item()) / n + PRED_LEN * LOG_2PI + self.log_det_lw

    @property
    def nll(self):
        """The groups' exact joint NLL per pair."""
        return self._per_pair(0)

    @property
    def nll_independent(self):
        """The NLL per pair of the independent head with the same marginals N(0, W + B)."""
        return self._per_pair(1)

    @property
    def nll_gain(self):
        """nll_independent - nll: what the coupling is worth, in nats per pair."""
        if not self.has_head:
            return None
        n = self.pairs
        return float((self.stats[1] - self.stats[0]).item()) / n if n else float("nan")

    @property
    def q_within_ratio(self):
        """q_within / (24 (N - G)): 1 when calibrated."""
        if not self.has_head:
            return None
        n, g = self._c()[:2]
        return float(self.stats[2].item()) / (DIM * (n - g)) if n > g else float("nan")

    @property
    def q_between_ratio(self):
        """q_between / (24 G): 1 when calibrated."""
        if not self.has_head:
            return None
        g = self.groups
        return float(self.stats[3].item()) / (DIM * g) if g else float("nan")


class CoupledHead(SampledEvals):
    """The scene-coupled head.  Of nll.SampledEvals it has the four
    evaluations of JOINT draws, ``joint_eval`` (g2k_coupled_joint_eval_f32),
    ``couple_scores`` (g2k_coupled_couple_scores_f32), ``scene_ranks``
    (g2k_coupled_scene_ranks_f32) and ``scene_modes``
    (g2k_coupled_scene_modes_f32), GPU tensors only; the per-pedestrian ones
    raise: they are ``marginal()``'s."""
    _PREFIX = "g2k_coupled_"
    _JOINT_GPU_ONLY = True

    def __init__(self, device="cuda"):
        cpl = torch.zeros((2, DIM, DIM), dtype=torch.float32, device=device)
        cpl[0] = torch.eye(DIM, dtype=torch.float32, device=device)
        self.cpl = cpl
        self.clipped = 0
        self._white = None              # (the cpl it belongs to, A, lam): float64 host arrays

    @classmethod
    def from_factors(cls, Lw, Lb, device="cuda"):
        """The head with the given lower factors (host arrays [24, 24])."""
        Lw, Lb = np.asarray(Lw, np.float64), np.asarray(Lb, np.float64)
        if Lw.shape != (DIM, DIM) or Lb.shape != (DIM, DIM):
            raise ValueError(f"Lw and Lb must be [{DIM}, {DIM}]")
        h = cls.__new__(cls)
        h.cpl = torch.from_numpy(np.stack([np.tril(Lw), np.tril(Lb)]).astype(np.float32)).to(device)
        h.clipped, h._white = 0, None
        return h

    @classmethod
    def from_fullcov(cls, head, share, device=None):
        """For tests: the full-covariance head's law cut in two, Lw =
        sqrt(1 - share) L, Lb = sqrt(share) L (0 <= share < 1)."""
        share = float(share)
        if not 0.0 <= share < 1.0:
            raise ValueError(f"share = {share}: 0 <= share < 1")
        L = head.chol.detach().cpu().double().numpy() if hasattr(head, "chol") else np.asarray(head, np.float64)
        if device is None:
            device = head.chol.device if hasattr(head, "chol") else "cuda"
        return cls.from_factors(math.sqrt(1.0 - share) * L, math.sqrt(share) * L, device)

    def _check_cpl(self, dev):
        if tuple(self.cpl.shape) != (2, DIM, DIM):
            raise ValueError(f"cpl must be [2, {DIM}, {DIM}]")
        _check_dev("cpl", self.cpl, dev, torch.float32)

    def _head_tensor(self, dev):
        self._check_cpl(dev)
        return self.cpl

    def _bind(self):
        load()

    def _factors(self):
        c = self.cpl.detach().cpu().double().numpy()
        return np.tril(c[0]), np.tril(c[1])

    def whitener(self):
        """(A [24, 24], lam [24]) float64: A W A^T = I, A B A^T = diag(lam);
        the fit's own when the head was fitted, else formed from ``cpl``."""
        key = (self.cpl.data_ptr(), self.cpl._version)
        if self._white is None or self._white[0] != key:
            self._white = (key,) + tuple(whiten_of(*self._factors()))
        return self._white[1:]

    def marginal(self):
        """One member's law N(mu, W + B) as a fullcov.FullCovHead, chol(W + B)
        formed in float64 on the host: the head for the per-pedestrian
        evaluations (best-of-K, KDE-NLL, sample scores, modes, ranks,
        kinematics)."""
        from .fullcov import FullCovHead
        Lw, Lb = self._factors()
        fc = FullCovHead.__new__(FullCovHead)
        fc.chol = torch.from_numpy(np.linalg.cholesky(Lw @ Lw.T + Lb @ Lb.T).astype(np.float32)).to(self.cpl.device)
        return fc

    def stats(self, pred, targets, n_active, *, n_frames=None, ped_mask=None, targets_shared=False,
              use_head=True, stream=None):
        """One launch (g2k_coupled_stats_f32): the residuals' within- and
        between-group sums over the scene-frames and, with ``use_head``, this
        head's exact joint NLL, the independent head's and the two quadratic
        forms -> CoupledStats."""
        lib = load()
        dev = pred.device
        d = self._dims(pred)
        _check_pairs_inputs(d, pred, targets, n_active, n_frames, ped_mask, targets_shared)
        wh, logdet = None, 0.0
        if use_head:
            self._check_cpl(dev)
            A, lam = self.whitener()
            wh = torch.from_numpy(np.concatenate([A, lam[None]], axis=0)).to(dev)
            logdet = float(np.log(np.diag(self._factors()[0])).sum())
        # S = 0 launches nothing: the outputs are the empty launch's zeros
        make = torch.zeros if d.S == 0 else torch.empty
        within = make((DIM, DIM), dtype=torch.float64, device=dev)
        between = make((DIM, DIM), dtype=torch.float64, device=dev)
        counts = make((NCOUNTS,), dtype=torch.int64, device=dev)
        stats = make((NSTATS,), dtype=torch.float64, device=dev)
        ws = torch.empty(max(8, int(lib.g2k_coupled_stats_workspace_bytes(ctypes.byref(d)))),
                         dtype=torch.uint8, device=dev)
        rc = lib.g2k_coupled_stats_f32(ctypes.byref(d), _ptr(pred), _ptr(targets), _ptr(n_active),
                                       _ptr(n_frames), _ptr(ped_mask), _ptr(wh), _ptr(within), _ptr(between),
                                       _ptr(counts), _ptr(stats), _ptr(ws), ws.numel(), _stream(stream))
        _lib.check("g2k_coupled_stats_f32", rc)
        return CoupledStats(within=within, between=between, counts=counts, stats=stats, log_det_lw=logdet,
                            has_head=bool(use_head))

    def fit(self, pred, targets, n_active, *, n_frames=None, ped_mask=None, targets_shared=False,
            stream=None):
        """Set ``self.cpl`` to the closed-form method-of-moments estimate (one
        stats launch without a head, then ``project`` on the host); remembers
        ``clipped`` and the whitener -> that launch's CoupledStats.  ValueError
        when no scene-frame has two members (N == G)."""
        st = self.stats(pred, targets, n_active, n_frames=n_frames, ped_mask=ped_mask,
                        targets_shared=targets_shared, use_head=False, stream=stream)
        if st.pairs == st.groups:
            raise ValueError("fit: no scene-frame with two members to tell the shared part from the own")
        Lw, Lb, A, lam, clipped = project(ridged(st.W), st.B_raw)
        self.cpl = torch.from_numpy(np.stack([Lw, Lb]).astype(np.float32)).to(pred.device)
        self.clipped = clipped
        self._white = ((self.cpl.data_ptr(), self.cpl._version), A, lam)
        return st

    def sample(self, pred, seed=0, stream=None):
        """One JOINT draw around pred [S, F, 2L, Nmax] (same layout out): the
        members of a scene-frame share c = Lb zc."""
        lib = load()
        d = self._dims(pred)
        _check_dev("pred", pred, pred.device, torch.float32)
        self._check_cpl(pred.device)
        out = torch.empty_like(pred)
        rc = lib.g2k_coupled_sample_f32(ctypes.byref(d), _ptr(pred), _ptr(self.cpl),
                                        ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), _ptr(out),
                                        _stream(stream))
        _lib.check("g2k_coupled_sample_f32", rc)
        return out

    def _marginal_only(self, *a, **k):
        raise NotImplementedError("a per-pedestrian evaluation sees one member's law: call it on marginal()")

    best_of_k = kde_nll = sample_scores = sample_modes = sample_ranks = sample_kin = _marginal_only
