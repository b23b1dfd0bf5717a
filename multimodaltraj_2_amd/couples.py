"""Couple-distance scores of a probabilistic head's JOINT samples
(csrc/g2k_couples.hip; include/g2k_couples.h states the definition): per couple
of a scene-frame's members two features of the distance between them over the
12 predicted steps — the closest approach ("min") and the final separation
("fin"), in the dataset's units — and per feature the fair CRPS of the K joint
draws against the targets' and the targets' PIT rank among the draws', uniform
on 0..K when the targets' dependence BETWEEN pedestrians is the head's.  The
collision rate of ``joint_eval`` is one threshold of this distribution.  One
call per head over the K joint draws ``sample(pred, seed + i)``, i < k, none of
them stored: ``GaussianHead.couple_scores``, ``FullCovHead.couple_scores`` and
``MixtureHead.couple_scores`` all end in ``_couple_scores`` below.

The entry points were added after ABI 11 and are declared in a header of their
own, so this module binds them itself on the handle ``_lib.load()`` returns
(``SYMBOLS`` below must equal include/g2k_couples.h)."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .frame_step import OBS_LEN, PRED_LEN, _ptr, _stream
from .kin import auto_bins
from .ranks import _dev

KMIN, KMAX, BMAX = 2, 64, 64
NSUMS, NTOT = 8, 4
FEATURES = ("min", "fin")
GEOM_FIELDS = ("tr", "tc", "cp", "dr", "tiles", "w", "passes", "lds_bytes")

_D = ctypes.POINTER(_lib.G2KDims)
_vp, _i64, _int, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int32
_CPL = (_int, [_D, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, _i32, _i32, ctypes.c_float, _vp, _vp, _vp,
               _vp, _vp, _vp, _vp, _i64, _vp])
# exported symbol -> (restype, argtypes); must match include/g2k_couples.h
SYMBOLS = {
    "g2k_couple_scores_workspace_bytes": (_i64, [_D, _i32, _i32]),
    "g2k_couple_scores_geometry": (_int, [_D, _i32, ctypes.POINTER(_i32)]),
    "g2k_couple_scores_f32": _CPL,
    "g2k_fullcov_couple_scores_f32": _CPL,
    "g2k_mix_couple_scores_f32": _CPL,
}


def load():
    """``_lib.load()``'s handle with this header's symbols bound (once); a
    library without them is an error, there is no fallback."""
    return _lib.bind(_lib.load(), "couples", SYMBOLS)


def _feature(g) -> int:
    if g not in FEATURES:
        raise ValueError(f"feature {g!r}: one of {', '.join(FEATURES)}")
    return FEATURES.index(g)


@dataclass
class CoupleScores:
    """A ``couple_scores`` call's outputs (include/g2k_couples.h).  Every
    method is one host read (float64) and takes a feature, "min" or "fin"; a
    figure whose denominator is 0 is NaN."""
    sums: torch.Tensor                  # [S, 8] f32: the scored couples' m, p, d, y per feature, summed
    hist: torch.Tensor                  # [S, 2, B] int32: row g the ranks of feature g
    tot: torch.Tensor                   # [S, 4] int64 {scored couples, sum r_min, sum r_fin, member couples}
    per_couple: torch.Tensor | None     # [S, F, Nmax, Nmax] int32: 1 + r_min + 256 r_fin, 0 when not scored
    per_frame_f: torch.Tensor | None    # [S, F, 8] the scene-frame's sums
    per_frame_i: torch.Tensor | None    # [S, F, 4] int32, the scene-frame's tot
    k: int = 0
    bins: int = 0
    reach: float = math.inf

    def counts(self):
        """[2, B] float64: the histograms summed over the scenes (one read)."""
        return self.hist.sum(dim=0, dtype=torch.int64).cpu().numpy().astype(np.float64)

    def totals(self):
        """{scored couples, sum r_min, sum r_fin, member couples} over all scenes."""
        return [int(v) for v in self.tot.sum(dim=0).tolist()]

    def _means(self):
        """[8] float64: the sums over all scenes divided by the scored couples."""
        n = self.couples
        s = self.sums.sum(dim=0, dtype=torch.float64).cpu().numpy()
        return s / n if n > 0 else np.full(NSUMS, np.nan)

    @property
    def couples(self) -> int:
        """The scored couples."""
        return self.totals()[0]

    @property
    def member_couples(self) -> int:
        """All member couples, scored or not (``joint_eval``'s ped_pairs)."""
        return self.totals()[3]

    def crps(self, g) -> float:
        """m_g - p_g / 2, the fair CRPS averaged over the scored couples, in
        the dataset's units."""
        i, m = _feature(g), self._means()
        return float(m[i] - 0.5 * m[2 + i])

    def draw_mean(self, g) -> float:
        """The mean of the feature over the draws and the scored couples."""
        return float(self._means()[4 + _feature(g)])

    def target_mean(self, g) -> float:
        """... of the targets."""
        return float(self._means()[6 + _feature(g)])

    def pit_mean(self, g) -> float:
        """The mean of (r_g + 1/2) / (K + 1) over the scored couples: 1/2 when
        calibrated, below it when the draws keep the couples further apart
        than the targets are."""
        t = self.totals()
        n = t[0]
        return (t[1 + _feature(g)] + 0.5 * n) / ((self.k + 1) * n) if n > 0 else float("nan")

    def dev(self, g) -> float:
        """1/2 sum_b |share_b - 1 / B| of the feature's ranks: 0 when
        calibrated (ranks.py's definition)."""
        c = self.counts()[_feature(g)]
        n = c.sum()
        return float(_dev(c / n)) if n > 0 else float("nan")


def couple_scores_geometry(S, F, Nmax, k) -> dict:
    """The launch geometry of ``couple_scores`` for these shapes
    (g2k_couple_scores_geometry: host arithmetic, no HIP call): a pass of a
    workgroup is a tile of tr x tc members (cp couples), its items made dr to a
    round; tiles that hold a couple when every column is a member, dealt to w
    workgroups per scene-frame, passes the most one of them takes; lds_bytes
    the workgroup's without the head's own."""
    lib = load()
    d = _lib.G2KDims(S, F, OBS_LEN, PRED_LEN, 16, 64, Nmax, OBS_LEN, 0)
    out = (ctypes.c_int32 * len(GEOM_FIELDS))()
    _lib.check("g2k_couple_scores_geometry", lib.g2k_couple_scores_geometry(ctypes.byref(d), int(k), out))
    return dict(zip(GEOM_FIELDS, (int(v) for v in out)))


def check_k_bins(k, bins):
    """-> (k, bins) as the entry points take them; ``bins`` None or 0: auto_bins."""
    k = int(k)
    if not KMIN <= k <= KMAX:
        raise ValueError(f"k = {k}: {KMIN}..{KMAX}")
    bins = auto_bins(k) if not bins else int(bins)
    if not 1 <= bins <= BMAX or (k + 1) % bins:
        raise ValueError(f"bins = {bins}: 1..{BMAX}, a divisor of k + 1 = {k + 1}")
    return k, bins


def check_reach(reach) -> float:
    """-> reach as the entry points take it; None: +inf, every couple."""
    reach = math.inf if reach is None else float(reach)
    if not reach > 0.0:
        raise ValueError(f"reach = {reach}: > 0, or None / inf for every couple")
    return reach


def _couple_scores(symbol, head, d, pred, targets, n_active, k, bins, seed, reach, n_frames, ped_mask,
                   want_per_couple, want_per_frame, stream):
    """The entry point ``symbol`` on checked inputs (nll._check_pairs_inputs);
    ``head`` is that head's parameter tensor -> CoupleScores."""
    lib = load()
    dev = pred.device
    k, bins = check_k_bins(k, bins)
    reach = check_reach(reach)
    S, F, Nmax = d.S, d.F, d.Nmax
    # S = 0 launches nothing: the outputs are the empty launch's zeros
    sums = torch.empty((S, NSUMS), dtype=torch.float32, device=dev)
    hist = torch.empty((S, 2, bins), dtype=torch.int32, device=dev)
    tot = torch.empty((S, NTOT), dtype=torch.int64, device=dev)
    pc = torch.empty((S, F, Nmax, Nmax), dtype=torch.int32, device=dev) if want_per_couple else None
    pf = torch.empty((S, F, NSUMS), dtype=torch.float32, device=dev) if want_per_frame else None
    pi = torch.empty((S, F, NTOT), dtype=torch.int32, device=dev) if want_per_frame else None
    need = int(lib.g2k_couple_scores_workspace_bytes(ctypes.byref(d), k, bins))
    ws = torch.empty(max(4, need), dtype=torch.uint8, device=dev)
    rc = getattr(lib, symbol)(ctypes.byref(d), _ptr(pred), _ptr(targets), _ptr(n_active), _ptr(n_frames),
                              _ptr(ped_mask), _ptr(head), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), k,
                              bins, ctypes.c_float(reach), _ptr(pc), _ptr(pf), _ptr(pi), _ptr(sums),
                              _ptr(hist), _ptr(tot), _ptr(ws), ws.numel(), _stream(stream))
    _lib.check(symbol, rc)
    return CoupleScores(sums=sums, hist=hist, tot=tot, per_couple=pc, per_frame_f=pf, per_frame_i=pi, k=k,
                        bins=bins, reach=reach)
