"""K-medoid reduction of a probabilistic head's JOINT samples to M scene modes
(csrc/g2k_scene_modes.hip; include/g2k_scene_modes.h states the definition):
per scene-frame the K joint draws ``sample(pred, seed + i)``, i < k, are
clustered by their joint displacement distance (PAM BUILD, then up to ``iters``
alternating rounds, all in double precision) to ``modes`` representative joint
futures with probabilities.  ``sample_modes`` reduces one pedestrian's draws to
centres; a mean of joint draws is no coherent scene, so here every mode IS one
of the draws, named by its draw index: the seed regenerates it
(``SceneModes.trajectories``) and nothing is stored.  The modes are scored
against the targets by minJADE_M / minJFDE_M, their Brier variants with the
clusters' weights and a scene-level miss rate (no mode keeps every member
within ``miss_radius`` at the final step), next to what the first M raw draws
give (``raw_jade``) and the floor of all K (``all_jade``).  One call per head:
``GaussianHead.scene_modes``, ``FullCovHead.scene_modes``,
``MixtureHead.scene_modes`` and ``CoupledHead.scene_modes`` all end in
``_scene_modes`` below.

The entry points were added after ABI 11 and are declared in a header of their
own, so this module binds them itself on the handle ``_lib.load()`` returns
(``SYMBOLS`` below must equal include/g2k_scene_modes.h)."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import torch

from . import _lib
from .frame_step import OBS_LEN, PRED_LEN, _ptr, _stream

MMAX, KMIN, KMAX, ITERS_MAX = 32, 2, 64, 32
NSUMS, NTOT = 8, 4
GEOM_FIELDS = ("tm", "dr", "tiles", "w", "pairs", "apt", "row_bytes", "lds_bytes")

_D = ctypes.POINTER(_lib.G2KDims)
_vp, _i64, _int, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int32
_SMD = (_int, [_D, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, _i32, _i32, _i32, ctypes.c_float, _vp, _vp,
               _vp, _vp, _vp, _vp, _vp, _i64, _vp])
# exported symbol -> (restype, argtypes); must match include/g2k_scene_modes.h
SYMBOLS = {
    "g2k_scene_modes_workspace_bytes": (_i64, [_D, _i32, _i32]),
    "g2k_scene_modes_geometry": (_int, [_D, _i32, _i32, ctypes.POINTER(_i32)]),
    "g2k_scene_modes_f32": _SMD,
    "g2k_fullcov_scene_modes_f32": _SMD,
    "g2k_mix_scene_modes_f32": _SMD,
}


def load():
    """``_lib.load()``'s handle with this header's symbols bound (once); a
    library without them is an error, there is no fallback."""
    return _lib.bind(_lib.load(), "scenemodes", SYMBOLS)


@dataclass
class SceneModes:
    """A ``scene_modes`` call's outputs (include/g2k_scene_modes.h).  Every
    property is one host read (float64); a figure whose denominator is 0 is
    NaN."""
    sums: torch.Tensor                  # [S, 8] f64: P cA, P cF, (1 - w_mA)^2, (1 - w_mF)^2, P cost, P raw, P all, 0
    tot: torch.Tensor                   # [S, 4] int64 {scored frames, sum P, missed frames, sum rounds}
    per_frame_i: torch.Tensor | None    # [S, F, 4] int32 {P or 0, mA, mF, rounds}
    per_frame_d: torch.Tensor | None    # [S, F, 8] f64 {cA, cF, w_mA, w_mF, cost, raw, all, min_m Mx}
    medoids: torch.Tensor | None        # [S, F, M] int32: the draw index of each mode
    counts: torch.Tensor | None         # [S, F, M] int32: the draws assigned to each mode
    k: int = 0
    modes: int = 0
    iters: int = 0
    miss_radius: float = 0.0
    seed: int = 0

    def totals(self):
        """{scored frames, sum P, missed frames, sum rounds} over all scenes."""
        return [int(v) for v in self.tot.sum(dim=0).tolist()]

    def _sum(self, i) -> float:
        return float(self.sums[:, i].sum(dtype=torch.float64))

    def _per_member(self, i) -> float:
        n = self.totals()[1]
        return self._sum(i) / n if n > 0 else float("nan")

    def _per_frame(self, v) -> float:
        n = self.frames
        return v / n if n > 0 else float("nan")

    @property
    def frames(self) -> int:
        """The scored scene-frames (one member or more)."""
        return self.totals()[0]

    @property
    def jade(self) -> float:
        """minJADE_M of the modes: sum P cA / sum P, the mean over the members."""
        return self._per_member(0)

    @property
    def jfde(self) -> float:
        """minJFDE_M of the modes."""
        return self._per_member(1)

    @property
    def brier_jade(self) -> float:
        """``jade`` + the mean over the scored frames of (1 - w)^2, w the
        weight of the mode that attains cA."""
        return self.jade + self._per_frame(self._sum(2))

    @property
    def brier_jfde(self) -> float:
        return self.jfde + self._per_frame(self._sum(3))

    @property
    def miss_rate(self) -> float:
        """The share of scored frames in which no mode keeps every member
        within ``miss_radius`` of its target at the final step."""
        return self._per_frame(float(self.totals()[2]))

    @property
    def cost(self) -> float:
        """The mean joint displacement of a draw to its mode, per member and step."""
        return self._per_member(4)

    @property
    def raw_jade(self) -> float:
        """minJADE of the first M draws, unreduced."""
        return self._per_member(5)

    @property
    def all_jade(self) -> float:
        """minJADE_K of all the draws: the floor of ``jade``."""
        return self._per_member(6)

    @property
    def rounds(self) -> float:
        """The mean number of alternating rounds run."""
        return self._per_frame(float(self.totals()[3]))

    def trajectories(self, head, pred, stream=None):
        """[S, F, M, 2L, Nmax] float32: the modes' joint futures, regenerated
        with ``head.sample(pred, seed + index)`` — one launch per distinct
        draw index in use — and gathered in torch (needs ``medoids``; not a
        hot path).  Rows of scene-frames that are not scored are draw 0's."""
        if self.medoids is None:
            raise ValueError("trajectories: the call was made without want_modes")
        S, F, L2, N = pred.shape
        med = self.medoids.long()
        out = torch.empty((S, F, self.modes, L2, N), dtype=pred.dtype, device=pred.device)
        for idx in torch.unique(med).tolist():
            draw = head.sample(pred, (self.seed + int(idx)) & (2 ** 64 - 1), stream=stream)
            sel = (med == idx)[..., None, None]                       # [S, F, M, 1, 1]
            out = torch.where(sel, draw[:, :, None], out)
        return out


def scene_modes_geometry(S, F, Nmax, k, modes) -> dict:
    """The launch geometry of ``scene_modes`` for these shapes
    (g2k_scene_modes_geometry: host arithmetic, no HIP call): one workgroup
    (w = 1) owns a scene-frame and walks its members in tiles of tm, tiles of
    them when every column is a member, a tile's k + 1 items made dr to a
    round; pairs = k (k + 1) / 2 distance accumulators, apt at most to a lane;
    row_bytes the scene-frame's row in the workspace; lds_bytes the
    workgroup's without the head's own."""
    lib = load()
    d = _lib.G2KDims(S, F, OBS_LEN, PRED_LEN, 16, 64, Nmax, OBS_LEN, 0)
    out = (ctypes.c_int32 * len(GEOM_FIELDS))()
    _lib.check("g2k_scene_modes_geometry",
               lib.g2k_scene_modes_geometry(ctypes.byref(d), int(k), int(modes), out))
    return dict(zip(GEOM_FIELDS, (int(v) for v in out)))


def check_args(k, modes, iters, miss_radius):
    """-> (k, modes, iters, miss_radius) as the entry points take them."""
    k, modes, iters, miss_radius = int(k), int(modes), int(iters), float(miss_radius)
    if not 1 <= modes <= MMAX:
        raise ValueError(f"modes = {modes}: 1..{MMAX}")
    if not max(modes, KMIN) <= k <= KMAX:
        raise ValueError(f"k = {k}: {max(modes, KMIN)}..{KMAX}")
    if not 0 <= iters <= ITERS_MAX:
        raise ValueError(f"iters = {iters}: 0..{ITERS_MAX}")
    if not (math.isfinite(miss_radius) and miss_radius >= 0):
        raise ValueError(f"miss_radius = {miss_radius}: finite and >= 0")
    return k, modes, iters, miss_radius


def _scene_modes(symbol, head, d, pred, targets, n_active, k, modes, iters, miss_radius, seed, n_frames,
                 ped_mask, want_per_frame, want_modes, stream):
    """The entry point ``symbol`` on checked inputs (nll._check_pairs_inputs);
    ``head`` is that head's parameter tensor -> SceneModes."""
    lib = load()
    dev = pred.device
    k, modes, iters, miss_radius = check_args(k, modes, iters, miss_radius)
    if dev.type != "cuda":
        raise ValueError(f"pred: on {dev}, expected a GPU tensor")
    S, F = d.S, d.F
    # S = 0 launches nothing: the outputs are the empty launch's zeros
    sums = torch.empty((S, NSUMS), dtype=torch.float64, device=dev)
    tot = torch.empty((S, NTOT), dtype=torch.int64, device=dev)
    pi = torch.empty((S, F, NTOT), dtype=torch.int32, device=dev) if want_per_frame else None
    pd = torch.empty((S, F, NSUMS), dtype=torch.float64, device=dev) if want_per_frame else None
    med = torch.empty((S, F, modes), dtype=torch.int32, device=dev) if want_modes else None
    cnt = torch.empty((S, F, modes), dtype=torch.int32, device=dev) if want_modes else None
    need = int(lib.g2k_scene_modes_workspace_bytes(ctypes.byref(d), k, modes))
    ws = torch.empty(max(8, need), dtype=torch.uint8, device=dev)
    seed = int(seed) & (2 ** 64 - 1)
    rc = getattr(lib, symbol)(ctypes.byref(d), _ptr(pred), _ptr(targets), _ptr(n_active), _ptr(n_frames),
                              _ptr(ped_mask), _ptr(head), ctypes.c_uint64(seed), k, modes, iters,
                              ctypes.c_float(miss_radius), _ptr(pi), _ptr(pd), _ptr(med), _ptr(cnt),
                              _ptr(sums), _ptr(tot), _ptr(ws), ws.numel(), _stream(stream))
    _lib.check(symbol, rc)
    return SceneModes(sums=sums, tot=tot, per_frame_i=pi, per_frame_d=pd, medoids=med, counts=cnt, k=k,
                      modes=modes, iters=iters, miss_radius=miss_radius, seed=seed)
