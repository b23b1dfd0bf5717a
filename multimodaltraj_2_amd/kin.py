"""Kinematic scores of a probabilistic head's samples (csrc/g2k_kin.hip;
include/g2k_kin.h states the definition): 32 scalar features of a trajectory —
11 speeds, 10 accelerations, 10 longitudinal accelerations and the
straightness, in the dataset's units per 0.4 s step — and per group of them the
fair CRPS of the K draws against the target and the target's PIT rank among the
draws' features, uniform on 0..K when the target moves as the head's draws do.
A PIT mean below 1/2: the draws' feature is larger than the target's (the
per-step head's draws accelerate harder than a person does).  One launch per
head over the K draws ``sample(pred, seed + i)``, i < k, none of them stored:
``GaussianHead.sample_kin``, ``FullCovHead.sample_kin`` and
``MixtureHead.sample_kin`` all end in ``_sample_kin`` below.

The entry points were added after ABI 11 and are declared in a header of their
own, so this module binds them itself on the handle ``_lib.load()`` returns
(``SYMBOLS`` below must equal include/g2k_kin.h)."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .frame_step import _ptr, _stream
from .nll import DRAWN_GEOM_FIELDS, _drawn_geometry
from .ranks import _dev

KMIN, KMAX, BMAX, ROWS = 2, 255, 64, 32
COLS, NSUMS, NTOT = 48, 16, 8
AUTO_BINS_MAX = 32
# group -> the rows of hist (and the columns of per_ped) that hold its ranks
GROUPS = {"speed": slice(0, 11), "acc": slice(11, 21), "lacc": slice(21, 31), "straight": slice(31, 32)}
GROUP_NAMES = tuple(GROUPS)
GEOM_FIELDS = DRAWN_GEOM_FIELDS

_D = ctypes.POINTER(_lib.G2KDims)
_vp, _i64, _int, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int32
_KIN = (_int, [_D, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, _i32, _i32, _vp, _vp, _vp, _vp, _vp,
               _i64, _vp])
# exported symbol -> (restype, argtypes); must match include/g2k_kin.h
SYMBOLS = {
    "g2k_sample_kin_workspace_bytes": (_i64, [_D, _i32]),
    "g2k_sample_kin_geometry": (_int, [_D, _i32, ctypes.POINTER(_i32)]),
    "g2k_sample_kin_f32": _KIN,
    "g2k_fullcov_sample_kin_f32": _KIN,
    "g2k_mix_sample_kin_f32": _KIN,
}


def load():
    """``_lib.load()``'s handle with this header's symbols bound (once); a
    library without them is an error, there is no fallback."""
    return _lib.bind(_lib.load(), "kin", SYMBOLS)


def auto_bins(k) -> int:
    """The largest divisor of k + 1 that is <= 32."""
    return max(b for b in range(1, AUTO_BINS_MAX + 1) if (int(k) + 1) % b == 0)


def _group(g) -> int:
    if g not in GROUPS:
        raise ValueError(f"group {g!r}: one of {', '.join(GROUP_NAMES)}")
    return GROUP_NAMES.index(g)


@dataclass
class SampleKin:
    """A ``sample_kin`` launch's outputs (include/g2k_kin.h).  Every method is
    one host read (float64) and takes a group, one of ``GROUPS``; a figure
    whose denominator is 0 is NaN."""
    sums: torch.Tensor              # [S, 16] f32: the pairs' m_g, p_g, d_g, y_g summed
    hist: torch.Tensor              # [S, 32, B] int32: row j the ranks of feature j
    tot: torch.Tensor               # [S, 8] int64 {pairs, sum r per group, 0, 0, 0}
    per_ped: torch.Tensor | None    # [S, F, Nmax, 48] {r_0..r_31, m_g, p_g, d_g, y_g}
    k: int = 0
    bins: int = 0

    def counts(self):
        """[32, B] float64: the histograms summed over the scenes (one read)."""
        return self.hist.sum(dim=0, dtype=torch.int64).cpu().numpy().astype(np.float64)

    def totals(self):
        """{pairs, sum r of speed, acc, lacc, straight, 0, 0, 0} over all scenes."""
        return [int(v) for v in self.tot.sum(dim=0).tolist()]

    def _means(self):
        """[16] float64: the sums over all scenes divided by the pairs."""
        n = self.pairs
        s = self.sums.sum(dim=0, dtype=torch.float64).cpu().numpy()
        return s / n if n > 0 else np.full(NSUMS, np.nan)

    @property
    def pairs(self) -> int:
        return self.totals()[0]

    def crps(self, g) -> float:
        """m_g - p_g / 2, the fair CRPS averaged over the group's rows and the
        pairs, in the feature's unit."""
        i, m = _group(g), self._means()
        return float(m[i] - 0.5 * m[4 + i])

    def draw_mean(self, g) -> float:
        """The mean of the feature over the group's rows, the draws and the pairs."""
        return float(self._means()[8 + _group(g)])

    def target_mean(self, g) -> float:
        """... of the targets."""
        return float(self._means()[12 + _group(g)])

    def pit_mean(self, g) -> float:
        """The mean of (r_j + 1/2) / (K + 1) over the group's rows and the
        pairs: 1/2 when calibrated, below it when the draws' feature is larger
        than the target's."""
        t = self.totals()
        i = _group(g)
        n = (GROUPS[g].stop - GROUPS[g].start) * t[0]
        return (t[1 + i] + 0.5 * n) / ((self.k + 1) * n) if n > 0 else float("nan")

    def dev(self, g) -> float:
        """1/2 sum_b |share_b - 1 / B| of the group's rows pooled: 0 when
        calibrated (ranks.py's definition)."""
        _group(g)
        c = self.counts()[GROUPS[g]].sum(axis=0)
        n = c.sum()
        return float(_dev(c / n)) if n > 0 else float("nan")


def sample_kin_geometry(S, F, Nmax, k) -> dict:
    """The launch geometry of ``sample_kin`` for these shapes
    (g2k_sample_kin_geometry: host arithmetic, no HIP call;
    the fields of nll._drawn_geometry)."""
    return _drawn_geometry(load(), "g2k_sample_kin_geometry", S, F, Nmax, k)


def check_k_bins(k, bins):
    """-> (k, bins) as the entry points take them; ``bins`` None or 0: auto_bins."""
    k = int(k)
    if not KMIN <= k <= KMAX:
        raise ValueError(f"k = {k}: {KMIN}..{KMAX}")
    bins = auto_bins(k) if not bins else int(bins)
    if not 1 <= bins <= BMAX or (k + 1) % bins:
        raise ValueError(f"bins = {bins}: 1..{BMAX}, a divisor of k + 1 = {k + 1}")
    return k, bins


def _sample_kin(symbol, head, d, pred, targets, n_active, k, bins, seed, n_frames, ped_mask,
                want_per_ped, stream):
    """The entry point ``symbol`` on checked inputs (nll._check_pairs_inputs);
    ``head`` is that head's parameter tensor -> SampleKin."""
    lib = load()
    dev = pred.device
    k, bins = check_k_bins(k, bins)
    S, F, Nmax = d.S, d.F, d.Nmax
    # S = 0 launches nothing: the outputs are the empty launch's zeros
    sums = torch.empty((S, NSUMS), dtype=torch.float32, device=dev)
    hist = torch.empty((S, ROWS, bins), dtype=torch.int32, device=dev)
    tot = torch.empty((S, NTOT), dtype=torch.int64, device=dev)
    per_ped = torch.empty((S, F, Nmax, COLS), dtype=torch.float32, device=dev) if want_per_ped else None
    need = int(lib.g2k_sample_kin_workspace_bytes(ctypes.byref(d), bins))
    ws = torch.empty(max(8, need), dtype=torch.uint8, device=dev)
    rc = getattr(lib, symbol)(ctypes.byref(d), _ptr(pred), _ptr(targets), _ptr(n_active), _ptr(n_frames),
                              _ptr(ped_mask), _ptr(head), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), k,
                              bins, _ptr(per_ped), _ptr(sums), _ptr(hist), _ptr(tot), _ptr(ws),
                              ws.numel(), _stream(stream))
    _lib.check(symbol, rc)
    return SampleKin(sums=sums, hist=hist, tot=tot, per_ped=per_ped, k=k, bins=bins)
