"""K-means reduction of a probabilistic head's samples to M modes
(csrc/g2k_modes.hip; include/g2k_modes.h states the definition): the K draws
``sample(pred, seed + i)``, i < k, of every pair are clustered to ``modes``
representative trajectories with probabilities by ``iters`` rounds of Lloyd's
algorithm in double precision, and the centres are scored against the target:
minADE_M / minFDE_M of the centres, their Brier variants with the clusters'
weights, the miss rate, the inertia and the number of live clusters.  One
launch per head, no draw ever in memory: ``GaussianHead.sample_modes``,
``FullCovHead.sample_modes`` and ``MixtureHead.sample_modes`` all end in
``_sample_modes`` below.

The entry points were added after ABI 11 and are declared in a header of their
own, so this module binds them itself on the handle ``_lib.load()`` returns
(``SYMBOLS`` below must equal include/g2k_modes.h)."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import torch

from . import _lib
from .frame_step import PRED_LEN
from .nll import DRAWN_GEOM_FIELDS, _drawn_geometry, _launch

MMAX, KMAX, ITERS_MAX = 32, 256, 64
GEOM_FIELDS = DRAWN_GEOM_FIELDS

_D = ctypes.POINTER(_lib.G2KDims)
_vp, _i64, _int, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int32
_MODES = (_int, [_D, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, _i32, _i32, _i32, ctypes.c_float,
                 _vp, _vp, _vp, _vp, _vp, _i64, _vp])
# exported symbol -> (restype, argtypes); must match include/g2k_modes.h
SYMBOLS = {
    "g2k_sample_modes_workspace_bytes": (_i64, [_D]),
    "g2k_sample_modes_geometry": (_int, [_D, _i32, _i32, ctypes.POINTER(_i32)]),
    "g2k_sample_modes_f32": _MODES,
    "g2k_fullcov_sample_modes_f32": _MODES,
    "g2k_mix_sample_modes_f32": _MODES,
}


def load():
    """``_lib.load()``'s handle with this header's symbols bound (once); a
    library without them is an error, there is no fallback."""
    return _lib.bind(_lib.load(), "modes", SYMBOLS)


@dataclass
class SampleModes:
    """A ``sample_modes`` launch's outputs (include/g2k_modes.h).  Every
    property is one host read (float64), a mean over the pairs; NaN when there
    is no pair."""
    out: torch.Tensor               # [S, 8] sums {cA, cF, (1 - w_mA)^2, (1 - w_mF)^2, misses, inertia, live}, pairs
    per_ped: torch.Tensor | None    # [S, F, Nmax, 8] {cA, cF, mA, mF, w_mA, w_mF, inertia, live}
    centres: torch.Tensor | None    # [S, F, M, 2L, Nmax]: each [:, :, m] laid out as pred
    weights: torch.Tensor | None    # [S, F, M, Nmax]
    k: int = 0
    modes: int = 0
    iters: int = 0
    miss_radius: float = 0.0

    def totals(self):
        """The sums over all scenes, on the host (one read, float64)."""
        return self.out.double().sum(dim=0).tolist()

    def _mean(self, i, j=None):
        t = self.totals()
        if not t[7] > 0:
            return float("nan")
        return (t[i] + (t[j] if j is not None else 0.0)) / t[7]

    @property
    def pairs(self) -> int:
        return int(self.totals()[7])

    @property
    def min_ade(self) -> float:
        """minADE_M of the centres."""
        return self._mean(0)

    @property
    def min_fde(self) -> float:
        return self._mean(1)

    @property
    def brier_ade(self) -> float:
        """The mean of cA + (1 - w)^2, w the weight of the centre that attains cA."""
        return self._mean(0, 2)

    @property
    def brier_fde(self) -> float:
        return self._mean(1, 3)

    @property
    def miss_rate(self) -> float:
        """The share of pairs whose best centre ends farther than ``miss_radius`` from the target."""
        return self._mean(4)

    @property
    def inertia(self) -> float:
        """The mean squared 24-D distance of a draw to its centre."""
        return self._mean(5)

    @property
    def live(self) -> float:
        """The mean number of non-empty clusters."""
        return self._mean(6)


def sample_modes_geometry(S, F, Nmax, k, modes) -> dict:
    """The launch geometry of ``sample_modes`` for these shapes
    (g2k_sample_modes_geometry: host arithmetic, no HIP call;
    the fields of nll._drawn_geometry)."""
    return _drawn_geometry(load(), "g2k_sample_modes_geometry", S, F, Nmax, k, modes)


def _sample_modes(symbol, head, d, pred, targets, n_active, k, modes, iters, seed, miss_radius,
                  n_frames, ped_mask, want_per_ped, want_centres, stream):
    """The entry point ``symbol`` on checked inputs (nll._check_pairs_inputs);
    ``head`` is that head's parameter tensor -> SampleModes (``want_centres``:
    the centres and their weights)."""
    lib = load()
    dev = pred.device
    k, modes, iters, miss_radius = int(k), int(modes), int(iters), float(miss_radius)
    if not 1 <= modes <= MMAX:
        raise ValueError(f"modes = {modes}: 1..{MMAX}")
    if not modes <= k <= KMAX:
        raise ValueError(f"k = {k}: modes..{KMAX}")
    if not 0 <= iters <= ITERS_MAX:
        raise ValueError(f"iters = {iters}: 0..{ITERS_MAX}")
    if not (math.isfinite(miss_radius) and miss_radius >= 0):
        raise ValueError(f"miss_radius = {miss_radius}: finite and >= 0")
    S, F, Nmax = d.S, d.F, d.Nmax
    # S = 0 launches nothing: the outputs are the empty launch's zeros
    out = torch.empty((S, 8), dtype=torch.float32, device=dev)
    per_ped = torch.empty((S, F, Nmax, 8), dtype=torch.float32, device=dev) if want_per_ped else None
    centres = weights = None
    if want_centres:
        centres = torch.empty((S, F, modes, 2 * PRED_LEN, Nmax), dtype=torch.float32, device=dev)
        weights = torch.empty((S, F, modes, Nmax), dtype=torch.float32, device=dev)
    _launch(lib, symbol, d, pred, targets, n_active, n_frames, ped_mask, head, seed, stream, k, modes,
            iters, miss_radius, per_ped, centres, weights, out, size="g2k_sample_modes_workspace_bytes")
    return SampleModes(out=out, per_ped=per_ped, centres=centres, weights=weights, k=k, modes=modes,
                       iters=iters, miss_radius=miss_radius)
