"""Scene-level rank calibration of a probabilistic head's JOINT samples
(csrc/g2k_scene_ranks.hip; include/g2k_scene_ranks.h states the definition):
per scene-frame with two members or more, the targets' whole configuration is
pooled with the K joint draws and ranked among them by three pre-rank functions
— typicality ("typ": the sum of an item's distances to the others), common mode
("loc": |the members' summed residual|^2 / P) and within-scene spread ("spr":
the residuals' sum of squares less loc) — uniform on 0..K when the targets come
from the head's JOINT law.  ``sample_ranks`` ranks one pedestrian's draws and
cannot see dependence between pedestrians; here a ``loc`` PIT near 1 (``spr``
near 0) says that the targets move together more than any draw does: the
coupling is too weak.  The same distance matrix gives the fair energy score of
the scene's joint law, ``es``: strictly proper, and known to be nearly blind
to dependence, so it is reported and never gated on.  One call per head over
the K joint draws ``sample(pred, seed + i)``, i < k, none of them stored:
``GaussianHead.scene_ranks``, ``FullCovHead.scene_ranks``,
``MixtureHead.scene_ranks`` and ``CoupledHead.scene_ranks`` all end in
``_scene_ranks`` below.

The entry points were added after ABI 11 and are declared in a header of their
own, so this module binds them itself on the handle ``_lib.load()`` returns
(``SYMBOLS`` below must equal include/g2k_scene_ranks.h)."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .frame_step import OBS_LEN, PRED_LEN, _ptr, _stream
from .kin import auto_bins
from .ranks import _dev

KMIN, KMAX, BMAX = 2, 64, 64
NSUMS, NTOT = 6, 4
FEATURES = ("typ", "loc", "spr")
GEOM_FIELDS = ("tm", "dr", "tiles", "w", "pairs", "apt", "aft", "lds_bytes")

_D = ctypes.POINTER(_lib.G2KDims)
_vp, _i64, _int, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int32
_SCN = (_int, [_D, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
               _i64, _vp])
# exported symbol -> (restype, argtypes); must match include/g2k_scene_ranks.h
SYMBOLS = {
    "g2k_scene_ranks_workspace_bytes": (_i64, [_D, _i32, _i32]),
    "g2k_scene_ranks_geometry": (_int, [_D, _i32, ctypes.POINTER(_i32)]),
    "g2k_scene_ranks_f32": _SCN,
    "g2k_fullcov_scene_ranks_f32": _SCN,
    "g2k_mix_scene_ranks_f32": _SCN,
}


def load():
    """``_lib.load()``'s handle with this header's symbols bound (once); a
    library without them is an error, there is no fallback."""
    return _lib.bind(_lib.load(), "sceneranks", SYMBOLS)


def _feature(g, among=FEATURES) -> int:
    if g not in among:
        raise ValueError(f"feature {g!r}: one of {', '.join(among)}")
    return FEATURES.index(g)


@dataclass
class SceneRanks:
    """A ``scene_ranks`` call's outputs (include/g2k_scene_ranks.h).  Every
    property or method is one host read (float64); a figure whose denominator
    is 0 is NaN."""
    sums: torch.Tensor                  # [S, 6] f64: m, p, mean_k loc_k, loc_K, mean_k spr_k, spr_K, summed
    hist: torch.Tensor                  # [S, 3, B] int32: row g the ranks of feature g
    tot: torch.Tensor                   # [S, 4] int64 {scored scene-frames, sum r_typ, sum r_loc, sum r_spr}
    per_frame_i: torch.Tensor | None    # [S, F, 4] int32 {P if scored else 0, r_typ, r_loc, r_spr}
    per_frame_d: torch.Tensor | None    # [S, F, 6] f64, the scene-frame's sums
    k: int = 0
    bins: int = 0

    def counts(self):
        """[3, B] float64: the histograms summed over the scenes (one read)."""
        return self.hist.sum(dim=0, dtype=torch.int64).cpu().numpy().astype(np.float64)

    def totals(self):
        """{scored scene-frames, sum r_typ, sum r_loc, sum r_spr} over all scenes."""
        return [int(v) for v in self.tot.sum(dim=0).tolist()]

    def _means(self):
        """[6] float64: the sums over all scenes divided by the scored scene-frames."""
        n = self.frames
        s = self.sums.sum(dim=0, dtype=torch.float64).cpu().numpy()
        return s / n if n > 0 else np.full(NSUMS, np.nan)

    @property
    def frames(self) -> int:
        """The scored scene-frames (two members or more)."""
        return self.totals()[0]

    @property
    def es(self) -> float:
        """m - p / 2, the fair energy score of the scene's joint law averaged
        over the scored scene-frames, in the dataset's units."""
        m = self._means()
        return float(m[0] - 0.5 * m[1])

    def pit(self, g) -> float:
        """The mean of (r_g + 1/2) / (K + 1) over the scored scene-frames: 1/2
        when calibrated."""
        t = self.totals()
        n = t[0]
        return (t[1 + _feature(g)] + 0.5 * n) / ((self.k + 1) * n) if n > 0 else float("nan")

    def dev(self, g) -> float:
        """1/2 sum_b |share_b - 1 / B| of the feature's ranks: 0 when
        calibrated (ranks.py's definition)."""
        c = self.counts()[_feature(g)]
        n = c.sum()
        return float(_dev(c / n)) if n > 0 else float("nan")

    def draw(self, g) -> float:
        """The mean of the feature ("loc" or "spr") over the draws and the
        scored scene-frames."""
        return float(self._means()[2 * _feature(g, FEATURES[1:])])

    def target(self, g) -> float:
        """... of the targets."""
        return float(self._means()[2 * _feature(g, FEATURES[1:]) + 1])


def scene_ranks_geometry(S, F, Nmax, k) -> dict:
    """The launch geometry of ``scene_ranks`` for these shapes
    (g2k_scene_ranks_geometry: host arithmetic, no HIP call): one workgroup
    (w = 1) owns a scene-frame and walks its members in tiles of tm, tiles of
    them when every column is a member, a tile's k + 1 items made dr to a
    round; pairs = k (k + 1) / 2 distance accumulators, apt at most to a lane,
    and aft of the 25 (k + 1) residual sums; lds_bytes the workgroup's without
    the head's own."""
    lib = load()
    d = _lib.G2KDims(S, F, OBS_LEN, PRED_LEN, 16, 64, Nmax, OBS_LEN, 0)
    out = (ctypes.c_int32 * len(GEOM_FIELDS))()
    _lib.check("g2k_scene_ranks_geometry", lib.g2k_scene_ranks_geometry(ctypes.byref(d), int(k), out))
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


def _scene_ranks(symbol, head, d, pred, targets, n_active, k, bins, seed, n_frames, ped_mask,
                 want_per_frame, stream):
    """The entry point ``symbol`` on checked inputs (nll._check_pairs_inputs);
    ``head`` is that head's parameter tensor -> SceneRanks."""
    lib = load()
    dev = pred.device
    k, bins = check_k_bins(k, bins)
    if dev.type != "cuda":
        raise ValueError(f"pred: on {dev}, expected a GPU tensor")
    S, F = d.S, d.F
    # S = 0 launches nothing: the outputs are the empty launch's zeros
    sums = torch.empty((S, NSUMS), dtype=torch.float64, device=dev)
    hist = torch.empty((S, 3, bins), dtype=torch.int32, device=dev)
    tot = torch.empty((S, NTOT), dtype=torch.int64, device=dev)
    pi = torch.empty((S, F, NTOT), dtype=torch.int32, device=dev) if want_per_frame else None
    pd = torch.empty((S, F, NSUMS), dtype=torch.float64, device=dev) if want_per_frame else None
    need = int(lib.g2k_scene_ranks_workspace_bytes(ctypes.byref(d), k, bins))
    ws = torch.empty(max(8, need), dtype=torch.uint8, device=dev)
    rc = getattr(lib, symbol)(ctypes.byref(d), _ptr(pred), _ptr(targets), _ptr(n_active), _ptr(n_frames),
                              _ptr(ped_mask), _ptr(head), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), k,
                              bins, _ptr(pi), _ptr(pd), _ptr(sums), _ptr(hist), _ptr(tot), _ptr(ws),
                              ws.numel(), _stream(stream))
    _lib.check(symbol, rc)
    return SceneRanks(sums=sums, hist=hist, tot=tot, per_frame_i=pi, per_frame_d=pd, k=k, bins=bins)
