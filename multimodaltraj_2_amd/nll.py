"""The bivariate-Gaussian NLL head and its sampling path (SURVEY.md §8(f)
row 4; the reference has none, so this is the build's definition and its
parity is unpinned — see csrc/g2k_nll.hip for the formulas and
oracle/g2k_ref.py bivariate_nll / gauss_sample for the checker).

``GaussianHead`` holds the head's parameters [3, 12] (log sigma_x, log
sigma_y, atanh rho per prediction step) around the model's predictions
(pred_path_band as the fused step writes it: [S, F, 2L, Nmax]); ``nll``
returns the summed loss, the pair count, d nll / d head and (optionally)
d nll / d pred; ``sample`` draws one reproducible trajectory per
(step, pedestrian); ``best_of_k`` evaluates K such draws against the targets
in one launch (minADE_K / minFDE_K, csrc/g2k_bestk.hip); ``kde_nll`` fits a
Gaussian kernel density estimate to the same K draws per step and scores the
target under it (the KDE-NLL of Trajectron++, csrc/g2k_kde.hip); ``joint_eval``
scores the same K draws as JOINT samples of a scene-frame (JADE_K / JFDE_K)
and counts collisions between the pedestrians (csrc/g2k_joint.hip);
``stats`` measures the head's calibration against the targets (coverage of
its confidence ellipses, per-step NLL) and ``fit`` sets the head to the
closed-form maximum-likelihood one of the residuals (csrc/g2k_calib.hip)."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .frame_step import OBS_LEN, PRED_LEN, _check_dev, _ptr, _stream


@dataclass
class BestOfK:
    """``GaussianHead.best_of_k``'s outputs (include/g2k_hip.h)."""
    sums: torch.Tensor              # [S, 8] {sum minADE, sum minFDE, pairs, sum ADE, sum FDE, K, 0, 0}
    per_ped: torch.Tensor | None    # [S, F, Nmax, 4] {minADE, minFDE, kA, kF}; zeros for non-pairs
    best: torch.Tensor | None       # [S, F, 2L, Nmax] draw kA for pairs, pred elsewhere

    def totals(self):
        """The sums over all scenes, on the host (one read, float64)."""
        return self.sums.double().sum(dim=0).tolist()

    def _mean(self, i):
        t = self.totals()
        return t[i] / t[2] if t[2] > 0 else float("nan")

    @property
    def pairs(self) -> int:
        return int(self.totals()[2])

    @property
    def min_ade(self) -> float:
        return self._mean(0)

    @property
    def min_fde(self) -> float:
        return self._mean(1)

    @property
    def ade(self) -> float:
        """The mean prediction's ADE (no sampling) over the same pairs."""
        return self._mean(3)

    @property
    def fde(self) -> float:
        return self._mean(4)


@dataclass
class KdeNll:
    """``GaussianHead.kde_nll``'s outputs (include/g2k_hip.h).  Every property
    is one host read (float64); a figure whose denominator is 0 is NaN."""
    out: torch.Tensor               # [S, 8] {sum kde_nll, sum kde_nll_final, pairs, sum clipped, K, floor, 0, 0}
    per_ped: torch.Tensor | None    # [S, F, Nmax, 4] {kde_nll, kde_nll_final, clipped steps, 0}
    k: int = 0
    log_floor: float = -20.0

    def totals(self):
        """The sums over all scenes, on the host (one read, float64)."""
        return self.out.double().sum(dim=0).tolist()

    def _mean(self, i, per=1):
        t = self.totals()
        return t[i] / (t[2] * per) if t[2] > 0 else float("nan")

    @property
    def pairs(self) -> int:
        return int(self.totals()[2])

    @property
    def kde_nll(self) -> float:
        """Per pair: the mean over the 12 steps of -max(log density, floor)."""
        return self._mean(0)

    @property
    def kde_nll_final(self) -> float:
        """Per pair: the last step's."""
        return self._mean(1)

    @property
    def clipped_share(self) -> float:
        """The share of (pair, step) terms that sit on the floor."""
        return self._mean(3, PRED_LEN)


@dataclass
class JointEval:
    """``GaussianHead.joint_eval``'s outputs (include/g2k_hip.h).  Every
    property is one host read (float64 / int); a rate whose denominator is 0
    is NaN."""
    sums_f: torch.Tensor                # [S, 4] {sum_f P minJADE, sum_f P minJFDE, K, 0}
    sums_i: torch.Tensor                # [S, 6] int64: sum_f of the per_frame_i columns
    per_frame_f: torch.Tensor | None    # [S, F, 4] {minJADE, minJFDE, kJA, kJF}
    per_frame_i: torch.Tensor | None    # [S, F, 6] int32 {P, PP, col_pred, col_gt, sum_k col_k, col_best}
    k: int = 0
    radius: float = 0.0

    def _f(self, i):
        return float(self.sums_f[:, i].double().sum().item())

    def _i(self, i):
        return int(self.sums_i[:, i].sum().item())

    def _rate(self, i, scale=1):
        den = self._i(1) * scale
        return self._i(i) / den if den > 0 else float("nan")

    @property
    def pairs(self) -> int:
        """(scene-frame, member) pairs: the denominator of ADE / minADE_K too."""
        return self._i(0)

    @property
    def ped_pairs(self) -> int:
        """Unordered member couples, summed over the scene-frames."""
        return self._i(1)

    @property
    def jade(self) -> float:
        p = self.pairs
        return self._f(0) / p if p > 0 else float("nan")

    @property
    def jfde(self) -> float:
        p = self.pairs
        return self._f(1) / p if p > 0 else float("nan")

    @property
    def collision_rate(self) -> float:
        """Of the K samples: colliding couples per couple and draw."""
        return self._rate(4, self.k)

    @property
    def collision_rate_pred(self) -> float:
        return self._rate(2)

    @property
    def collision_rate_best(self) -> float:
        """Of each scene-frame's best joint sample (draw kJA)."""
        return self._rate(5)

    @property
    def collision_rate_gt(self) -> float:
        return self._rate(3)


@dataclass
class HeadStats:
    """``GaussianHead.stats``'s outputs (include/g2k_hip.h).  Every property
    is one host read (float64); a figure whose denominator is 0 is NaN, and
    those of a head (nll, coverage, ece, q_ratio) are None when the launch had
    none (``use_head=False``)."""
    stats: torch.Tensor                 # [12, 8] float64 {pairs, S dx, S dy, S dx2, S dy2, S dxdy, S nll, S q}
    inside: torch.Tensor | None         # [12, NL] int64: pairs with q_t <= r2[l]
    fit_head: torch.Tensor              # [3, 12] float32: the closed-form head, written by the device
    levels: tuple = ()
    r2: torch.Tensor | None = None      # [NL] float64 on the device
    has_head: bool = True

    def _s(self):
        return self.stats.cpu().numpy()

    @property
    def pairs(self) -> int:
        return int(self.stats[0, 0].item())

    @property
    def fit(self) -> torch.Tensor:
        return self.fit_head

    @property
    def nll_per_step(self):
        """[12] mean NLL of a pair at each step."""
        if not self.has_head:
            return None
        s = self._s()
        with np.errstate(invalid="ignore", divide="ignore"):
            return s[:, 6] / s[:, 0]

    @property
    def nll(self):
        """Per pair, summed over the 12 steps."""
        if not self.has_head:
            return None
        s = self._s()
        return float(s[:, 6].sum() / s[0, 0]) if s[0, 0] > 0 else float("nan")

    @property
    def coverage(self):
        """[12, NL]: share of the pairs inside each level's ellipse, per step."""
        if not self.has_head:
            return None
        n = self._s()[:, :1]
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.inside.cpu().numpy().astype(np.float64) / n

    @property
    def coverage_all(self):
        """[NL]: pooled over the 12 steps."""
        if not self.has_head:
            return None
        n = self._s()[:, 0].sum()
        tot = self.inside.sum(dim=0).cpu().numpy().astype(np.float64)
        return tot / n if n > 0 else np.full(tot.shape, np.nan)

    @property
    def ece(self):
        """mean over the levels of |coverage_all - p|."""
        if not self.has_head:
            return None
        if not self.levels:
            return float("nan")
        return float(np.abs(self.coverage_all - np.asarray(self.levels, np.float64)).mean())

    @property
    def q_ratio(self):
        """sum q / (2 * 12 * pairs): 1 under a calibrated head."""
        if not self.has_head:
            return None
        s = self._s()
        return float(s[:, 7].sum() / (2.0 * PRED_LEN * s[0, 0])) if s[0, 0] > 0 else float("nan")

    @property
    def bias(self):
        """[12, 2]: mean dx, dy per step."""
        s = self._s()
        with np.errstate(invalid="ignore", divide="ignore"):
            return s[:, 1:3] / s[:, :1]


MAX_LEVELS = 32
DEFAULT_LEVELS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99)


def _check_pairs_inputs(d, pred, targets, n_active, n_frames, ped_mask, targets_shared):
    """What every evaluation over the pairs takes, whatever the head: pred,
    targets ([S, 1, ...] when shared: sets the flag in ``d``), n_active and
    the optional n_frames / ped_mask, all on pred's device."""
    dev = pred.device
    S, F, Nmax = d.S, d.F, d.Nmax
    if targets_shared:
        d.flags = _lib.STEP_TARGETS_SHARED
    _check_dev("pred", pred, dev, torch.float32)
    if tuple(n_active.shape) != (S,):
        raise ValueError("n_active must be [S]")
    _check_dev("n_active", n_active, dev, torch.int32)
    tshape = (S, 1 if targets_shared else F, Nmax, PRED_LEN, 2)
    if tuple(targets.shape) != tshape:
        raise ValueError(f"targets must be {list(tshape)}")
    _check_dev("targets", targets, dev, torch.float32)
    if n_frames is not None:
        if tuple(n_frames.shape) != (S,):
            raise ValueError("n_frames must be [S]")
        _check_dev("n_frames", n_frames, dev, torch.int32)
    if ped_mask is not None:
        if tuple(ped_mask.shape) != (S, Nmax):
            raise ValueError("ped_mask must be [S, Nmax]")
        _check_dev("ped_mask", ped_mask, dev, torch.uint8)


def best_of_k_geometry(S, F, Nmax, k) -> dict:
    """The launch geometry of the per-pair sampled evaluations (best-of-K and
    KDE-NLL of either head) for these shapes (g2k_best_of_k_geometry: host
    arithmetic, no HIP call): ks lanes share a pair's draws, fc frames per
    workgroup, c workgroups per scene."""
    lib = _lib.load()
    d = _lib.G2KDims(S, F, OBS_LEN, PRED_LEN, 16, 64, Nmax, OBS_LEN, 0)
    out = (ctypes.c_int32 * len(_lib.BESTK_GEOM_FIELDS))()
    _lib.check("g2k_best_of_k_geometry", lib.g2k_best_of_k_geometry(ctypes.byref(d), int(k), out))
    return dict(zip(_lib.BESTK_GEOM_FIELDS, (int(v) for v in out)))


# the out[] of the drawn-once evaluations' geometry entry points
# (G2K_{SCORES,MODES,RANKS,KIN}_GEOM_*: csrc/g2k_drawn.h holds them equal)
DRAWN_GEOM_FIELDS = ("g", "lanes", "fc", "c", "lds_bytes")


def _drawn_geometry(lib, symbol, S, F, Nmax, *params) -> dict:
    """The launch geometry of a drawn-once sampled evaluation (sample_scores,
    sample_modes, sample_ranks, sample_kin) for these shapes, from its entry
    point ``symbol`` on the handle ``lib`` (host arithmetic, no HIP call):
    g pairs per pass of a workgroup, lanes per pair, fc frames per workgroup,
    c workgroups per scene and the workgroup's LDS bytes without the head's
    own.  ``params``: K, and what else the entry point takes before out."""
    d = _lib.G2KDims(S, F, OBS_LEN, PRED_LEN, 16, 64, Nmax, OBS_LEN, 0)
    out = (ctypes.c_int32 * len(DRAWN_GEOM_FIELDS))()
    _lib.check(symbol, getattr(lib, symbol)(ctypes.byref(d), *(int(v) for v in params), out))
    return dict(zip(DRAWN_GEOM_FIELDS, (int(v) for v in out)))


def _launch(lib, symbol, d, pred, targets, n_active, n_frames, ped_mask, head, seed, stream, *args,
            size=None):
    """The tail of every sampled evaluation: the workspace (``size``, the
    entry point's own ``*_workspace_bytes`` when not named), the seed mod 2^64,
    the call and its check.  ``args`` are what ``symbol`` takes between the
    seed and the workspace; tensors and None go as pointers."""
    size = getattr(lib, size or symbol.replace("_f32", "_workspace_bytes"))
    ws = torch.empty(max(1, int(size(ctypes.byref(d)))), dtype=torch.uint8, device=pred.device)
    mid = [_ptr(a) if a is None or isinstance(a, torch.Tensor) else a for a in args]
    rc = getattr(lib, symbol)(ctypes.byref(d), _ptr(pred), _ptr(targets), _ptr(n_active),
                              _ptr(n_frames), _ptr(ped_mask), _ptr(head),
                              ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), *mid, _ptr(ws), ws.numel(),
                              _stream(stream))
    _lib.check(symbol, rc)


class SampledEvals:
    """The ten sampled evaluations of a probabilistic head, once for the
    heads (GaussianHead below, fullcov.FullCovHead, mixture.MixtureHead;
    coupled.CoupledHead takes the four of JOINT draws): each
    is ONE launch over the K draws ``sample(pred, seed + i)``, i < k, of the
    head it is called on, none of them stored.  A head supplies ``_PREFIX``
    (its entry points are ``_PREFIX`` + best_of_k_f32, ...), ``_head_tensor``
    and, where it refuses host tensors in ``joint_eval``, ``_JOINT_GPU_ONLY``;
    a head whose symbols are bound apart from _lib.SYMBOLS does that in
    ``_bind``."""
    _PREFIX = "g2k_"
    _JOINT_GPU_ONLY = False

    def _head_tensor(self, dev):
        """The head's parameter tensor, checked (shape, dtype, on ``dev``)."""
        raise NotImplementedError

    def _bind(self):
        """Before anything else of an evaluation: the head's own symbols."""

    def _dims(self, pred):
        S, F, L2, Nmax = (int(x) for x in pred.shape)
        if L2 != 2 * PRED_LEN:
            raise ValueError(f"pred must be [S, F, {2 * PRED_LEN}, Nmax]")
        return _lib.G2KDims(S, F, OBS_LEN, PRED_LEN, 16, 64, Nmax, OBS_LEN, 0)

    def _sampled_inputs(self, pred, targets, n_active, n_frames, ped_mask, targets_shared):
        """-> (dims, the head's tensor), everything checked."""
        self._bind()
        d = self._dims(pred)
        _check_pairs_inputs(d, pred, targets, n_active, n_frames, ped_mask, targets_shared)
        return d, self._head_tensor(pred.device)

    def best_of_k(self, pred, targets, n_active, k, seed=0, *, n_frames=None, ped_mask=None,
                  targets_shared=False, want_per_ped=True, want_best=False, stream=None):
        """Best-of-K sampling evaluation in one launch (``_PREFIX`` +
        best_of_k_f32, csrc/g2k_bestk.hip): of the K draws ``sample(pred, seed
        + i)``, i < k, each pair's smallest ADE and FDE and the draws that
        attain them -> BestOfK."""
        d, head = self._sampled_inputs(pred, targets, n_active, n_frames, ped_mask, targets_shared)
        lib = _lib.load()
        dev = pred.device
        k = int(k)
        if not 1 <= k <= 4096:
            raise ValueError(f"k = {k}: 1..4096")
        S, F, Nmax = d.S, d.F, d.Nmax
        sums = torch.empty((S, 8), dtype=torch.float32, device=dev)
        per_ped = torch.empty((S, F, Nmax, 4), dtype=torch.float32, device=dev) if want_per_ped else None
        best = torch.empty_like(pred) if want_best else None
        _launch(lib, self._PREFIX + "best_of_k_f32", d, pred, targets, n_active, n_frames, ped_mask,
                head, seed, stream, k, per_ped, best, sums)
        return BestOfK(sums=sums, per_ped=per_ped, best=best)

    def kde_nll(self, pred, targets, n_active, k, seed=0, *, log_floor=-20.0, n_frames=None,
                ped_mask=None, want_per_ped=False, targets_shared=False, stream=None):
        """KDE-NLL in one launch (``_PREFIX`` + kde_nll_f32, csrc/g2k_kde.hip):
        per pair and step a Gaussian kernel density estimate (Scott's
        bandwidth, as scipy.stats.gaussian_kde) of the K draws ``sample(pred,
        seed + i)``, i < k, and the target's log density under it, floored at
        ``log_floor`` -> KdeNll.  k in 4..4096."""
        d, head = self._sampled_inputs(pred, targets, n_active, n_frames, ped_mask, targets_shared)
        lib = _lib.load()
        dev = pred.device
        k = int(k)
        if not 4 <= k <= 4096:
            raise ValueError(f"k = {k}: 4..4096")
        log_floor = float(log_floor)
        if not math.isfinite(log_floor):
            raise ValueError(f"log_floor = {log_floor}: finite")
        S, F, Nmax = d.S, d.F, d.Nmax
        out = torch.empty((S, 8), dtype=torch.float32, device=dev)
        per_ped = torch.empty((S, F, Nmax, 4), dtype=torch.float32, device=dev) if want_per_ped else None
        _launch(lib, self._PREFIX + "kde_nll_f32", d, pred, targets, n_active, n_frames, ped_mask, head,
                seed, stream, k, log_floor, per_ped, out)
        return KdeNll(out=out, per_ped=per_ped, k=k, log_floor=log_floor)

    def joint_eval(self, pred, targets, n_active, k, radius, seed=0, *, n_frames=None, ped_mask=None,
                   targets_shared=False, want_per_frame=True, stream=None):
        """Joint best-of-K evaluation in one launch (``_PREFIX`` +
        joint_eval_f32, csrc/g2k_joint.hip): draw i < k of EVERY member of a
        scene-frame is ``sample(pred, seed + i)``; per scene-frame the smallest
        mean ADE / FDE over the members (JADE_K / JFDE_K) and the couples that
        come closer than ``radius`` at any of the 12 predicted steps, in the
        draws, the mean prediction and the targets -> JointEval."""
        d, head = self._sampled_inputs(pred, targets, n_active, n_frames, ped_mask, targets_shared)
        lib = _lib.load()
        dev = pred.device
        k = int(k)
        if not 1 <= k <= 4096:
            raise ValueError(f"k = {k}: 1..4096")
        radius = float(radius)
        if not (math.isfinite(radius) and radius >= 0.0):
            raise ValueError(f"radius = {radius}: finite and >= 0")
        # _check_dev only compares devices: the heads that refuse host tensors do it here
        if self._JOINT_GPU_ONLY and dev.type != "cuda":
            raise ValueError(f"pred: on {dev}, expected a GPU tensor")
        S, F = d.S, d.F
        sums_f = torch.empty((S, 4), dtype=torch.float32, device=dev)
        sums_i = torch.empty((S, 6), dtype=torch.int64, device=dev)
        pf = torch.empty((S, F, 4), dtype=torch.float32, device=dev) if want_per_frame else None
        pi = torch.empty((S, F, 6), dtype=torch.int32, device=dev) if want_per_frame else None
        _launch(lib, self._PREFIX + "joint_eval_f32", d, pred, targets, n_active, n_frames, ped_mask,
                head, seed, stream, k, radius, pf, pi, sums_f, sums_i)
        return JointEval(sums_f=sums_f, sums_i=sums_i, per_frame_f=pf, per_frame_i=pi, k=k,
                         radius=radius)

    def sample_scores(self, pred, targets, n_active, k, seed=0, *, n_frames=None, ped_mask=None,
                      want_per_ped=False, targets_shared=False, stream=None):
        """Energy, variogram and diversity scores of the K draws
        ``sample(pred, seed + i)``, i < k, in one launch (``_PREFIX`` +
        sample_scores_f32, csrc/g2k_scores.hip) -> scores.SampleScores.  k in
        2..256."""
        from .scores import _sample_scores
        d, head = self._sampled_inputs(pred, targets, n_active, n_frames, ped_mask, targets_shared)
        return _sample_scores(self._PREFIX + "sample_scores_f32", head, d, pred, targets, n_active, k,
                              seed, n_frames, ped_mask, want_per_ped, stream)

    def sample_modes(self, pred, targets, n_active, k, modes, iters=10, seed=0, *, miss_radius=0.0,
                     n_frames=None, ped_mask=None, want_per_ped=True, want_centres=False,
                     targets_shared=False, stream=None):
        """K-means reduction of the K draws ``sample(pred, seed + i)``, i < k,
        to ``modes`` centres with probabilities and the centres' scores, in one
        launch (``_PREFIX`` + sample_modes_f32, csrc/g2k_modes.hip) ->
        modes.SampleModes.  modes in 1..32, k in modes..256, iters in 0..64."""
        from .modes import _sample_modes
        d, head = self._sampled_inputs(pred, targets, n_active, n_frames, ped_mask, targets_shared)
        return _sample_modes(self._PREFIX + "sample_modes_f32", head, d, pred, targets, n_active, k,
                             modes, iters, seed, miss_radius, n_frames, ped_mask, want_per_ped,
                             want_centres, stream)

    def sample_ranks(self, pred, targets, n_active, k, bins=None, seed=0, *, n_frames=None,
                     ped_mask=None, targets_shared=False, want_per_ped=False, stream=None):
        """Rank-histogram calibration of the K draws ``sample(pred, seed +
        i)``, i < k, in one launch (``_PREFIX`` + sample_ranks_f32,
        csrc/g2k_ranks.hip): the target's rank among the draws per step (a
        kernel density pre-rank) and per trajectory (an energy pre-rank),
        uniform when the target comes from the head's law ->
        ranks.SampleRanks.  k in 4..255; ``bins`` divides k + 1, at most 64
        (None: the largest divisor <= 32)."""
        from .ranks import _sample_ranks
        d, head = self._sampled_inputs(pred, targets, n_active, n_frames, ped_mask, targets_shared)
        return _sample_ranks(self._PREFIX + "sample_ranks_f32", head, d, pred, targets, n_active, k, bins,
                             seed, n_frames, ped_mask, want_per_ped, stream)

    def sample_kin(self, pred, targets, n_active, k, bins=None, seed=0, *, n_frames=None,
                   ped_mask=None, targets_shared=False, want_per_ped=False, stream=None):
        """Kinematic scores of the K draws ``sample(pred, seed + i)``, i < k,
        in one launch (``_PREFIX`` + sample_kin_f32, csrc/g2k_kin.hip): per
        group of features (speed, acc, lacc, straight) the fair CRPS and the
        target's PIT rank among the draws, uniform when the target moves as
        the head's draws do -> kin.SampleKin.  k in 2..255; ``bins`` divides
        k + 1, at most 64 (None: the largest divisor <= 32)."""
        from .kin import _sample_kin
        d, head = self._sampled_inputs(pred, targets, n_active, n_frames, ped_mask, targets_shared)
        return _sample_kin(self._PREFIX + "sample_kin_f32", head, d, pred, targets, n_active, k, bins,
                           seed, n_frames, ped_mask, want_per_ped, stream)

    def couple_scores(self, pred, targets, n_active, k, bins=None, seed=0, *, reach=None, n_frames=None,
                      ped_mask=None, want_per_couple=False, want_per_frame=False, targets_shared=False,
                      stream=None):
        """Couple-distance scores of the K JOINT draws ``sample(pred, seed +
        i)``, i < k, in one call (``_PREFIX`` + couple_scores_f32,
        csrc/g2k_couples.hip): per couple of a scene-frame's members whose mean
        predictions come within ``reach`` (None: every couple) the closest
        approach and the final separation, their fair CRPS and the targets'
        PIT rank among the draws, uniform when the targets depend on each other
        as the head's joint draws do -> couples.CoupleScores.  k in 2..64;
        ``bins`` divides k + 1, at most 64 (None: the largest divisor <= 32)."""
        from .couples import _couple_scores
        d, head = self._sampled_inputs(pred, targets, n_active, n_frames, ped_mask, targets_shared)
        return _couple_scores(self._PREFIX + "couple_scores_f32", head, d, pred, targets, n_active, k,
                              bins, seed, reach, n_frames, ped_mask, want_per_couple, want_per_frame,
                              stream)

    def scene_ranks(self, pred, targets, n_active, k, bins=None, seed=0, *, n_frames=None, ped_mask=None,
                    targets_shared=False, want_per_frame=False, stream=None):
        """Scene-level rank calibration of the K JOINT draws ``sample(pred,
        seed + i)``, i < k, in one call (``_PREFIX`` + scene_ranks_f32,
        csrc/g2k_scene_ranks.hip): per scene-frame with two members or more
        the targets' whole configuration ranked among the draws' by
        typicality, common mode and within-scene spread, uniform when the
        targets come from the head's joint law, and the fair energy score of
        that law -> sceneranks.SceneRanks.  GPU tensors only.  k in 2..64;
        ``bins`` divides k + 1, at most 64 (None: the largest divisor <= 32)."""
        from .sceneranks import _scene_ranks
        d, head = self._sampled_inputs(pred, targets, n_active, n_frames, ped_mask, targets_shared)
        return _scene_ranks(self._PREFIX + "scene_ranks_f32", head, d, pred, targets, n_active, k, bins,
                            seed, n_frames, ped_mask, want_per_frame, stream)

    def scene_modes(self, pred, targets, n_active, k, m, iters=10, miss_radius=0.0, seed=0, *, n_frames=None,
                    ped_mask=None, targets_shared=False, want_per_frame=False, want_modes=True, stream=None):
        """K-medoid reduction of the K JOINT draws ``sample(pred, seed + i)``,
        i < k, of every scene-frame to ``m`` scene modes, each one of the draws
        (named by its index) with a probability, and the modes' scores, in one
        call (``_PREFIX`` + scene_modes_f32, csrc/g2k_scene_modes.hip):
        minJADE_M / minJFDE_M, their Brier variants, the scene-level miss rate
        at ``miss_radius``, the clustering cost, and the minJADE of the first m
        raw draws and of all k -> scenemodes.SceneModes.  GPU tensors only.  m
        in 1..32, k in max(m, 2)..64, iters in 0..32."""
        from .scenemodes import _scene_modes
        d, head = self._sampled_inputs(pred, targets, n_active, n_frames, ped_mask, targets_shared)
        return _scene_modes(self._PREFIX + "scene_modes_f32", head, d, pred, targets, n_active, k, m, iters,
                            miss_radius, seed, n_frames, ped_mask, want_per_frame, want_modes, stream)


class GaussianHead(SampledEvals):
    """The per-step head.  Its sampled evaluations (SampledEvals) run over the
    draws of ``sample``, 12 independent steps each: ``best_of_k`` is
    g2k_best_of_k_f32, ``kde_nll`` g2k_kde_nll_f32, ``joint_eval``
    g2k_joint_eval_f32 (the one head that does not refuse host tensors there),
    ``sample_scores`` g2k_sample_scores_f32, ``sample_modes``
    g2k_sample_modes_f32, ``sample_ranks`` g2k_sample_ranks_f32,
    ``sample_kin`` g2k_sample_kin_f32 and ``couple_scores``
    g2k_couple_scores_f32."""
    _PREFIX = "g2k_"

    def __init__(self, log_sigma=0.0, device="cuda"):
        h = torch.zeros((3, PRED_LEN), dtype=torch.float32, device=device)
        h[:2] = float(log_sigma)
        self.head = h

    def _head_tensor(self, dev):
        _check_dev("head", self.head, dev, torch.float32)
        return self.head

    def nll(self, pred, targets, n_active, *, n_frames=None, ped_mask=None, want_dpred=False,
            stream=None):
        """-> (nll, pairs, dhead [3, 12], dpred [S, F, 2L, Nmax] or None)."""
        lib = _lib.load()
        dev = pred.device
        d = self._dims(pred)
        S, F, Nmax = d.S, d.F, d.Nmax
        _check_dev("pred", pred, dev, torch.float32)
        _check_dev("head", self.head, dev, torch.float32)
        _check_dev("n_active", n_active, dev, torch.int32)
        if tuple(targets.shape) != (S, F, Nmax, PRED_LEN, 2):
            raise ValueError(f"targets must be [{S}, {F}, {Nmax}, {PRED_LEN}, 2]")
        _check_dev("targets", targets, dev, torch.float32)
        out = torch.empty(3 * PRED_LEN + 2, dtype=torch.float32, device=dev)
        dpred = torch.zeros_like(pred) if want_dpred else None
        ws = torch.empty(max(1, int(lib.g2k_nll_workspace_bytes(ctypes.byref(d)))), dtype=torch.uint8,
                         device=dev)
        rc = lib.g2k_nll_f32(ctypes.byref(d), _ptr(pred), _ptr(targets), _ptr(n_active),
                             _ptr(n_frames), _ptr(ped_mask), _ptr(self.head), _ptr(out), _ptr(dpred),
                             _ptr(ws), ws.numel(), _stream(stream))
        _lib.check("g2k_nll_f32", rc)
        return out[3 * PRED_LEN], out[3 * PRED_LEN + 1], out[:3 * PRED_LEN].view(3, PRED_LEN), dpred

    def _r2(self, levels, dev):
        """The levels' radii -2 log1p(-p), float64, on ``dev`` (formed on the
        host once per set of levels: a repeated call copies nothing)."""
        cache = self.__dict__.setdefault("_r2_cache", {})
        key = (levels, str(dev))
        if key not in cache:
            cache.clear()
            cache[key] = (-2.0 * torch.log1p(-torch.tensor(levels, dtype=torch.float64))).to(dev)
        return cache[key]

    def stats(self, pred, targets, n_active, levels=DEFAULT_LEVELS, *, n_frames=None, ped_mask=None,
              targets_shared=False, use_head=True, stream=None):
        """Calibration in one launch (g2k_head_stats_f32): the per-step
        residual moments over the pairs and their closed-form head (``fit``),
        and, with ``use_head``, this head's NLL, q = squared Mahalanobis
        distance and the pairs inside the ``levels``' ellipses (level p: q <=
        -2 ln(1 - p), the chi^2(2) quantile) -> HeadStats."""
        levels = tuple(float(p) for p in levels) if use_head else ()
        if len(levels) > MAX_LEVELS:
            raise ValueError(f"{len(levels)} levels: {MAX_LEVELS} at most")
        for p in levels:
            if not 0.0 < p < 1.0:
                raise ValueError(f"level {p}: 0 < p < 1")
        lib = _lib.load()
        dev = pred.device
        d = self._dims(pred)
        S = d.S
        _check_pairs_inputs(d, pred, targets, n_active, n_frames, ped_mask, targets_shared)
        if use_head:
            _check_dev("head", self.head, dev, torch.float32)
        nl = len(levels)
        r2 = self._r2(levels, dev) if nl else None
        # S = 0 launches nothing: the outputs are the empty launch's zeros
        make = torch.zeros if S == 0 else torch.empty
        stats = make((PRED_LEN, 8), dtype=torch.float64, device=dev)
        inside = make((PRED_LEN, nl), dtype=torch.int64, device=dev) if use_head else None
        fit = make((3, PRED_LEN), dtype=torch.float32, device=dev)
        ws = torch.empty(max(8, int(lib.g2k_head_stats_workspace_bytes(ctypes.byref(d), nl))),
                         dtype=torch.uint8, device=dev)
        rc = lib.g2k_head_stats_f32(ctypes.byref(d), _ptr(pred), _ptr(targets), _ptr(n_active),
                                    _ptr(n_frames), _ptr(ped_mask),
                                    _ptr(self.head) if use_head else None, _ptr(r2), nl, _ptr(stats),
                                    _ptr(inside) if nl else None, _ptr(fit), _ptr(ws), ws.numel(),
                                    _stream(stream))
        _lib.check("g2k_head_stats_f32", rc)
        return HeadStats(stats=stats, inside=inside, fit_head=fit, levels=levels, r2=r2,
                         has_head=bool(use_head))

    def fit(self, pred, targets, n_active, *, n_frames=None, ped_mask=None, targets_shared=False,
            stream=None):
        """Set ``self.head`` to the closed-form maximum-likelihood head of the
        residuals (one stats launch without a head; the device writes the
        head) -> that launch's HeadStats.  ValueError when there is no pair."""
        hs = self.stats(pred, targets, n_active, (), n_frames=n_frames, ped_mask=ped_mask,
                        targets_shared=targets_shared, use_head=False, stream=stream)
        if hs.pairs == 0:
            raise ValueError("fit: no (scene, frame, pedestrian) pair to fit the head on")
        self.head = hs.fit_head
        return hs

    def sample(self, pred, seed=0, stream=None):
        """One draw around pred [S, F, 2L, Nmax] (same layout out)."""
        lib = _lib.load()
        d = self._dims(pred)
        _check_dev("pred", pred, pred.device, torch.float32)
        out = torch.empty_like(pred)
        rc = lib.g2k_gauss_sample_f32(ctypes.byref(d), _ptr(pred), _ptr(self.head),
                                      ctypes.c_uint64(int(seed)), _ptr(out), _stream(stream))
        _lib.check("g2k_gauss_sample_f32", rc)
        return out
