"""Trajectory-level scores of a probabilistic head's samples
(csrc/g2k_scores.hip; include/g2k_scores.h states the definition): the energy
score with the 24-D norm (``es_traj``, strictly proper for the joint law of a
pedestrian's 12 steps), with the ADE and the FDE (``es_ade``, ``es_fde``:
marginals only), the expected ADE / FDE of a draw, the average pairwise
displacement of the K draws (``apd``) and the variogram score of order 1/2
(``vs``, the one that sees the dependence between steps).  One launch per
head over the K draws ``sample(pred, seed + i)``, i < k, none of them stored:
``GaussianHead.sample_scores``, ``FullCovHead.sample_scores`` and
``MixtureHead.sample_scores`` all end in ``_sample_scores`` below.

The entry points were added after ABI 11 and are declared in a header of their
own, so this module binds them itself on the handle ``_lib.load()`` returns
(``SYMBOLS`` below must equal include/g2k_scores.h)."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from . import _lib
from .nll import DRAWN_GEOM_FIELDS, _drawn_geometry, _launch

KMIN, KMAX = 2, 256
GEOM_FIELDS = DRAWN_GEOM_FIELDS

_D = ctypes.POINTER(_lib.G2KDims)
_vp, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
_SCORES = (_int, [_D, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, ctypes.c_int32, _vp, _vp, _vp,
                  _i64, _vp])
# exported symbol -> (restype, argtypes); must match include/g2k_scores.h
SYMBOLS = {
    "g2k_sample_scores_workspace_bytes": (_i64, [_D]),
    "g2k_sample_scores_geometry": (_int, [_D, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
    "g2k_sample_scores_f32": _SCORES,
    "g2k_fullcov_sample_scores_f32": _SCORES,
    "g2k_mix_sample_scores_f32": _SCORES,
}


def load():
    """``_lib.load()``'s handle with this header's symbols bound (once); a
    library without them is an error, there is no fallback."""
    return _lib.bind(_lib.load(), "scores", SYMBOLS)


@dataclass
class SampleScores:
    """A ``sample_scores`` launch's outputs (include/g2k_scores.h).  Every
    property is one host read (float64), a mean over the pairs; a figure whose
    denominator is 0 is NaN."""
    out: torch.Tensor               # [S, 8] sums of {mA, mF, mR, pA, pF, pR, vs} and the pair count
    per_ped: torch.Tensor | None    # [S, F, Nmax, 8] {mA, mF, mR, pA, pF, pR, vs, 0}
    k: int = 0

    def totals(self):
        """The sums over all scenes, on the host (one read, float64)."""
        return self.out.double().sum(dim=0).tolist()

    def _mean(self, i, j=None):
        t = self.totals()
        if not t[7] > 0:
            return float("nan")
        return (t[i] - (0.5 * t[j] if j is not None else 0.0)) / t[7]

    @property
    def pairs(self) -> int:
        return int(self.totals()[7])

    @property
    def es_traj(self) -> float:
        """The fair energy score with the norm over all 24 coordinates."""
        return self._mean(2, 5)

    @property
    def es_ade(self) -> float:
        """The mean of the 12 per-step energy scores."""
        return self._mean(0, 3)

    @property
    def es_fde(self) -> float:
        """The last step's energy score."""
        return self._mean(1, 4)

    @property
    def mean_ade(self) -> float:
        """The expected ADE of a draw."""
        return self._mean(0)

    @property
    def mean_fde(self) -> float:
        return self._mean(1)

    @property
    def apd(self) -> float:
        """The average pairwise displacement (ADE) of the K draws."""
        return self._mean(3)

    @property
    def vs(self) -> float:
        """The variogram score of order 1/2 over the 66 step pairs."""
        return self._mean(6)


def sample_scores_geometry(S, F, Nmax, k) -> dict:
    """The launch geometry of ``sample_scores`` for these shapes
    (g2k_sample_scores_geometry: host arithmetic, no HIP call;
    the fields of nll._drawn_geometry)."""
    return _drawn_geometry(load(), "g2k_sample_scores_geometry", S, F, Nmax, k)


def _sample_scores(symbol, head, d, pred, targets, n_active, k, seed, n_frames, ped_mask,
                   want_per_ped, stream):
    """The entry point ``symbol`` on checked inputs (nll._check_pairs_inputs);
    ``head`` is that head's parameter tensor -> SampleScores."""
    lib = load()
    dev = pred.device
    k = int(k)
    if not KMIN <= k <= KMAX:
        raise ValueError(f"k = {k}: {KMIN}..{KMAX}")
    S, F, Nmax = d.S, d.F, d.Nmax
    # S = 0 launches nothing: the outputs are the empty launch's zeros
    out = torch.empty((S, 8), dtype=torch.float32, device=dev)
    per_ped = torch.empty((S, F, Nmax, 8), dtype=torch.float32, device=dev) if want_per_ped else None
    _launch(lib, symbol, d, pred, targets, n_active, n_frames, ped_mask, head, seed, stream, k, per_ped,
            out, size="g2k_sample_scores_workspace_bytes")
    return SampleScores(out=out, per_ped=per_ped, k=k)
