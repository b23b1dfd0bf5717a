"""Rank-histogram calibration of a probabilistic head's samples
(csrc/g2k_ranks.hip; include/g2k_ranks.h states the definition): per pair the
target is pooled with the K draws, every one of the K + 1 points gets a scalar
pre-rank — per step a kernel density among the other K points, per trajectory
the sum of the 24-D distances to them — and the target's rank among them is
uniform on 0..K when the target comes from the law of the draws, whatever that
law is (the multivariate rank histogram of Gneiting et al. 2008).  A U-shaped
histogram: the head is too narrow; a hump: too wide.  One launch per head over
the K draws ``sample(pred, seed + i)``, i < k, none of them stored:
``GaussianHead.sample_ranks``, ``FullCovHead.sample_ranks`` and
``MixtureHead.sample_ranks`` all end in ``_sample_ranks`` below.

The entry points were added after ABI 11 and are declared in a header of their
own, so this module binds them itself on the handle ``_lib.load()`` returns
(``SYMBOLS`` below must equal include/g2k_ranks.h)."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .frame_step import PRED_LEN, _ptr, _stream
from .nll import DRAWN_GEOM_FIELDS, _drawn_geometry

KMIN, KMAX, BMAX, ROWS = 4, 255, 64, 13
AUTO_BINS_MAX = 32
GEOM_FIELDS = DRAWN_GEOM_FIELDS

_D = ctypes.POINTER(_lib.G2KDims)
_vp, _i64, _int, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int32
_RANKS = (_int, [_D, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, _i32, _i32, _vp, _vp, _vp, _vp,
                 _i64, _vp])
# exported symbol -> (restype, argtypes); must match include/g2k_ranks.h
SYMBOLS = {
    "g2k_sample_ranks_workspace_bytes": (_i64, [_D, _i32]),
    "g2k_sample_ranks_geometry": (_int, [_D, _i32, ctypes.POINTER(_i32)]),
    "g2k_sample_ranks_f32": _RANKS,
    "g2k_fullcov_sample_ranks_f32": _RANKS,
    "g2k_mix_sample_ranks_f32": _RANKS,
}


def load():
    """``_lib.load()``'s handle with this header's symbols bound (once); a
    library without them is an error, there is no fallback."""
    return _lib.bind(_lib.load(), "ranks", SYMBOLS)


def auto_bins(k) -> int:
    """The largest divisor of k + 1 that is <= 32."""
    return max(b for b in range(1, AUTO_BINS_MAX + 1) if (int(k) + 1) % b == 0)


def _dev(h):
    """Half the L1 distance of the shares h [..., B] from uniform: the
    total-variation distance."""
    return 0.5 * np.abs(h - 1.0 / h.shape[-1]).sum(axis=-1)


@dataclass
class SampleRanks:
    """A ``sample_ranks`` launch's outputs (include/g2k_ranks.h).  Every
    property is one host read (float64); a figure whose denominator is 0 is
    NaN."""
    hist: torch.Tensor              # [S, 13, B] int32: rows 0..11 the steps' ranks, row 12 the trajectory's
    tot: torch.Tensor               # [S, 4] int64 {pairs, degenerate steps, sum r_t, sum r_traj}
    per_ped: torch.Tensor | None    # [S, F, Nmax, 16] {r_0..r_11, r_traj, degenerate steps, 0, 0}
    k: int = 0
    bins: int = 0

    def counts(self):
        """[13, B] float64: the histograms summed over the scenes (one read)."""
        return self.hist.sum(dim=0, dtype=torch.int64).cpu().numpy().astype(np.float64)

    def totals(self):
        """{pairs, degenerate steps, sum r_t, sum r_traj} over all scenes."""
        return [int(v) for v in self.tot.sum(dim=0).tolist()]

    @staticmethod
    def _shares(c):
        n = c.sum(axis=-1, keepdims=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, c / n, np.nan)

    @property
    def pairs(self) -> int:
        return self.totals()[0]

    @property
    def degenerate_share(self) -> float:
        """The share of (pair, step) whose pooled bandwidth is singular."""
        t = self.totals()
        return t[1] / (PRED_LEN * t[0]) if t[0] > 0 else float("nan")

    @property
    def hist_steps(self):
        """[12, B]: each step's histogram as shares of its non-degenerate pairs."""
        return self._shares(self.counts()[:PRED_LEN])

    @property
    def hist_pooled(self):
        """[B]: the 12 steps pooled."""
        return self._shares(self.counts()[:PRED_LEN].sum(axis=0))

    @property
    def hist_traj(self):
        """[B]: the trajectory rank's."""
        return self._shares(self.counts()[PRED_LEN])

    @property
    def dev(self) -> float:
        """1/2 sum_b |share_b - 1 / B| of the pooled steps: 0 when calibrated."""
        return float(_dev(self.hist_pooled))

    @property
    def dev_final(self) -> float:
        return float(_dev(self.hist_steps[PRED_LEN - 1]))

    @property
    def dev_traj(self) -> float:
        return float(_dev(self.hist_traj))

    @property
    def mean(self) -> float:
        """The mean of (r_t + 1/2) / (K + 1) over the non-degenerate steps: 1/2
        when calibrated, above it when the head is too narrow."""
        t = self.totals()
        n = PRED_LEN * t[0] - t[1]
        return (t[2] + 0.5 * n) / ((self.k + 1) * n) if n > 0 else float("nan")

    @property
    def mean_traj(self) -> float:
        t = self.totals()
        return (t[3] + 0.5 * t[0]) / ((self.k + 1) * t[0]) if t[0] > 0 else float("nan")

    def coverage(self, p):
        """-> (nominal, observed): the largest bin edge j / B <= p and the
        pooled share of the steps' ranks below that edge: how many targets are
        among the (nominal) most typical points."""
        j = int(np.floor(float(p) * self.bins + 1e-9))
        j = min(max(j, 0), self.bins)
        return j / self.bins, float(self.hist_pooled[:j].sum())


def sample_ranks_geometry(S, F, Nmax, k) -> dict:
    """The launch geometry of ``sample_ranks`` for these shapes
    (g2k_sample_ranks_geometry: host arithmetic, no HIP call;
    the fields of nll._drawn_geometry)."""
    return _drawn_geometry(load(), "g2k_sample_ranks_geometry", S, F, Nmax, k)


def check_k_bins(k, bins):
    """-> (k, bins) as the entry points take them; ``bins`` None or 0: auto_bins."""
    k = int(k)
    if not KMIN <= k <= KMAX:
        raise ValueError(f"k = {k}: {KMIN}..{KMAX}")
    bins = auto_bins(k) if not bins else int(bins)
    if not 1 <= bins <= BMAX or (k + 1) % bins:
        raise ValueError(f"bins = {bins}: 1..{BMAX}, a divisor of k + 1 = {k + 1}")
    return k, bins


def _sample_ranks(symbol, head, d, pred, targets, n_active, k, bins, seed, n_frames, ped_mask,
                  want_per_ped, stream):
    """The entry point ``symbol`` on checked inputs (nll._check_pairs_inputs);
    ``head`` is that head's parameter tensor -> SampleRanks."""
    lib = load()
    dev = pred.device
    k, bins = check_k_bins(k, bins)
    S, F, Nmax = d.S, d.F, d.Nmax
    # S = 0 launches nothing: the outputs are the empty launch's zeros
    hist = torch.empty((S, ROWS, bins), dtype=torch.int32, device=dev)
    tot = torch.empty((S, 4), dtype=torch.int64, device=dev)
    per_ped = torch.empty((S, F, Nmax, 16), dtype=torch.float32, device=dev) if want_per_ped else None
    need = int(lib.g2k_sample_ranks_workspace_bytes(ctypes.byref(d), bins))
    ws = torch.empty(max(8, need), dtype=torch.uint8, device=dev)
    rc = getattr(lib, symbol)(ctypes.byref(d), _ptr(pred), _ptr(targets), _ptr(n_active), _ptr(n_frames),
                              _ptr(ped_mask), _ptr(head), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), k,
                              bins, _ptr(per_ped), _ptr(hist), _ptr(tot), _ptr(ws), ws.numel(),
                              _stream(stream))
    _lib.check(symbol, rc)
    return SampleRanks(hist=hist, tot=tot, per_ped=per_ped, k=k, bins=bins)
