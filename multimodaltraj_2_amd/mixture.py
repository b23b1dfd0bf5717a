"""The Gaussian-mixture trajectory head (csrc/g2k_mix.hip; include/g2k_mix.h
states the definition): up to 8 full-covariance Gaussians over a pair's
24-vector of residuals, component m = {w_m, b_m [24], L_m [24, 24]} in one
parameter block ``params`` [8, 608] (per slot: w, 7 unused floats, b, L
row-major).  A slot with w == 0 is dead.  fullcov.FullCovHead is its one-slot,
b = 0 special case: one ellipsoid, where this head can say "keeps walking *or*
stops *or* turns".  The build's: the reference has no probabilistic head, so
its parity is unpinned (tests/mixture_ref.py is the float64 checker).

``em_step`` is one EM iteration on the device, ``fit`` a number of them without
a host read in between, ``stats`` the E-step alone (the NLL of a given
mixture), ``sample`` one reproducible draw per (scene, frame, pedestrian) and
``best_of_k`` the fused minADE_K / minFDE_K over such draws
(csrc/g2k_bestk.hip with the MixHead policy); ``joint_eval`` and ``kde_nll``
are the other heads' fused joint best-of-K and KDE-NLL over the same draws
(csrc/g2k_joint.hip, csrc/g2k_kde.hip).

The entry points were added after ABI 11 and are declared in a header of their
own, so this module binds them itself on the handle ``_lib.load()`` returns
(``SYMBOLS`` below must equal include/g2k_mix.h)."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from statistics import NormalDist

import numpy as np
import torch

from . import _lib
from .frame_step import PRED_LEN, _check_dev, _ptr, _stream
from .nll import SampledEvals, _check_pairs_inputs

DIM = 2 * PRED_LEN
SLOTS = 8
PITCH = 608
OFF_B, OFF_L = 8, 32

_D = ctypes.POINTER(_lib.G2KDims)
_vp, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
# exported symbol -> (restype, argtypes); must match include/g2k_mix.h
SYMBOLS = {
    "g2k_mix_em_workspace_bytes": (_i64, [_D]),
    "g2k_mix_em_f32": (_int, [_D, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "g2k_mix_sample_f32": (_int, [_D, _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp]),
    "g2k_mix_best_of_k_workspace_bytes": (_i64, [_D]),
    "g2k_mix_best_of_k_f32": (_int, [_D, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64,
                                     ctypes.c_int32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "g2k_mix_joint_eval_workspace_bytes": (_i64, [_D]),
    "g2k_mix_joint_eval_f32": (_int, [_D, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64,
                                      ctypes.c_int32, ctypes.c_float, _vp, _vp, _vp, _vp, _vp, _i64,
                                      _vp]),
    "g2k_mix_kde_nll_workspace_bytes": (_i64, [_D]),
    "g2k_mix_kde_nll_f32": (_int, [_D, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64,
                                   ctypes.c_int32, ctypes.c_float, _vp, _vp, _vp, _i64, _vp]),
}


def load():
    """``_lib.load()``'s handle with this header's symbols bound (once); a
    library without them is an error, there is no fallback."""
    return _lib.bind(_lib.load(), "mix", SYMBOLS)


@dataclass
class MixtureStats:
    """One E-step's outputs (include/g2k_mix.h).  Every property is one host
    read (float64); a figure whose denominator is 0 is NaN."""
    moments: torch.Tensor               # [8, 25, 24] float64: G_m, then s_m
    resp: torch.Tensor                  # [8, 2] float64 {N_m, hard count}
    total: torch.Tensor                 # [4] float64 {pairs, sum log density, 0, 0}

    @property
    def pairs(self) -> int:
        return int(self.total[0].item())

    @property
    def loglik(self) -> float:
        """The mean log density per pair."""
        t = self.total.cpu().numpy()
        return float(t[1] / t[0]) if t[0] > 0 else float("nan")

    @property
    def nll(self) -> float:
        return -self.loglik

    @property
    def usage(self):
        """[8]: the share of the pairs hard-assigned to each slot."""
        n = float(self.total[0].item())
        h = self.resp[:, 1].cpu().numpy()
        return h / n if n > 0 else np.full(h.shape, np.nan)

    @property
    def resp_mass(self):
        """[8]: N_m / pairs, what the M-step makes the weights."""
        n = float(self.total[0].item())
        h = self.resp[:, 0].cpu().numpy()
        return h / n if n > 0 else np.full(h.shape, np.nan)


@dataclass
class MixtureFit:
    """``MixtureHead.fit``'s outputs."""
    loglik: np.ndarray                  # [iters] float64: the mean log density BEFORE each step
    pairs: int
    resp: torch.Tensor                  # [8, 2] float64: the last step's {N_m, hard count}

    @property
    def gain(self) -> float:
        """The last minus the first log-likelihood per pair."""
        return float(self.loglik[-1] - self.loglik[0]) if len(self.loglik) else 0.0


class MixtureHead(SampledEvals):
    """The Gaussian-mixture head.  Its sampled evaluations (nll.SampledEvals)
    are FullCovHead's over this head's draws ``sample(pred, seed + i)``, i <
    k: ``best_of_k`` is g2k_mix_best_of_k_f32, ``kde_nll`` g2k_mix_kde_nll_f32,
    ``sample_scores`` g2k_mix_sample_scores_f32, ``sample_modes``
    g2k_mix_sample_modes_f32 and ``joint_eval`` g2k_mix_joint_eval_f32 (GPU
    tensors only), where each member of a scene-frame draws with the component
    its own selector picks, so one joint sample mixes components across the
    pedestrians."""
    _PREFIX = "g2k_mix_"
    _JOINT_GPU_ONLY = True

    def __init__(self, components=3, device="cuda"):
        components = int(components)
        if not 1 <= components <= SLOTS:
            raise ValueError(f"components = {components}: 1..{SLOTS}")
        p = np.zeros((SLOTS, PITCH), np.float32)
        p[:components, 0] = 1.0 / components
        p[:components, OFF_L:] = np.eye(DIM, dtype=np.float32).reshape(-1)
        self.params = torch.from_numpy(p).to(device)

    # -- views of the block -------------------------------------------------
    @property
    def weights(self) -> torch.Tensor:
        return self.params[:, 0]

    @property
    def means(self) -> torch.Tensor:
        return self.params[:, OFF_B:OFF_L]

    @property
    def chols(self) -> torch.Tensor:
        return self.params[:, OFF_L:].view(SLOTS, DIM, DIM)

    @property
    def components(self) -> int:
        """The number of live slots (one host read)."""
        return int((self.params[:, 0] != 0).sum().item())

    @classmethod
    def from_block(cls, block, device=None):
        """A head around a parameter block [8, 608] (a tensor, or anything
        NumPy reads: rounded to float32 once)."""
        if isinstance(block, torch.Tensor):
            t = block.to(torch.float32)
            if device is not None:
                t = t.to(device)
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(block, np.float32))).to(
                device if device is not None else "cuda")
        if tuple(t.shape) != (SLOTS, PITCH):
            raise ValueError(f"params must be [{SLOTS}, {PITCH}]")
        h = cls.__new__(cls)
        h.params = t.contiguous()
        return h

    @classmethod
    def from_fullcov(cls, fc, device=None):
        """One live slot, b = 0, L = ``fc.chol``: the full-covariance head as
        a mixture (the same density and, bit for bit, the same draws)."""
        chol = fc.chol
        dev = device if device is not None else chol.device
        p = torch.zeros((SLOTS, PITCH), dtype=torch.float32, device=dev)
        p[0, 0] = 1.0
        p[0, OFF_L:] = torch.tril(chol.to(dev, torch.float32)).reshape(-1)
        h = cls.__new__(cls)
        h.params = p
        return h

    @classmethod
    def init_from(cls, fullcov_stats, components, device=None):
        """The deterministic start of EM from a ``FullCovHead.stats(use_head=
        False)`` launch: with C the residuals' uncentred second moments
        (float64, on the host), lambda_1 and v_1 its leading eigenpair (v_1
        signed so that its largest-magnitude entry is positive), b_m = z_m
        sqrt(lambda_1) v_1 where z_m is the standard-normal quantile of
        (m + 1/2) / M; every L_m is that launch's ``fit_chol`` and w = 1 / M."""
        M = int(components)
        if not 1 <= M <= SLOTS:
            raise ValueError(f"components = {M}: 1..{SLOTS}")
        if fullcov_stats.pairs == 0:
            raise ValueError("init_from: no (scene, frame, pedestrian) pair to start from")
        C = np.asarray(fullcov_stats.cov, np.float64)
        lam, vec = np.linalg.eigh(0.5 * (C + C.T))
        v = vec[:, -1]
        if v[np.argmax(np.abs(v))] < 0:
            v = -v
        scale = np.sqrt(max(float(lam[-1]), 0.0))
        nd = NormalDist()
        p = np.zeros((SLOTS, PITCH), np.float32)
        fit = fullcov_stats.fit_chol.detach().cpu().numpy().astype(np.float32)
        for m in range(M):
            p[m, 0] = np.float32(1.0 / M)
            p[m, OFF_B:OFF_L] = (nd.inv_cdf((m + 0.5) / M) * scale * v).astype(np.float32)
            p[m, OFF_L:] = np.tril(fit).reshape(-1)
        dev = device if device is not None else fullcov_stats.fit_chol.device
        return cls.from_block(p, device=dev)

    # -- launches -----------------------------------------------------------
    def _check_params(self, dev, t=None):
        t = self.params if t is None else t
        if tuple(t.shape) != (SLOTS, PITCH):
            raise ValueError(f"params must be [{SLOTS}, {PITCH}]")
        _check_dev("params", t, dev, torch.float32)

    def _head_tensor(self, dev):
        self._check_params(dev)
        return self.params

    def _bind(self):
        load()

    def _em_buffers(self, lib, d, dev, rows=1):
        # S = 0 launches nothing: the outputs are the empty launch's zeros
        make = torch.zeros if d.S == 0 else torch.empty
        moments = make((SLOTS, DIM + 1, DIM), dtype=torch.float64, device=dev)
        resp = make((SLOTS, 2), dtype=torch.float64, device=dev)
        total = make((rows, 4), dtype=torch.float64, device=dev)
        need = int(lib.g2k_mix_em_workspace_bytes(ctypes.byref(d)))
        if need < 0:
            raise ValueError(f"mixture: S={d.S} F={d.F} Nmax={d.Nmax} is out of range")
        ws = torch.empty(max(8, need), dtype=torch.uint8, device=dev)
        return moments, resp, total, ws

    def _em(self, lib, d, pred, targets, n_active, n_frames, ped_mask, mix_in, moments, resp,
            total_ptr, mix_out, ws, stream):
        rc = lib.g2k_mix_em_f32(ctypes.byref(d), _ptr(pred), _ptr(targets), _ptr(n_active),
                                _ptr(n_frames), _ptr(ped_mask), _ptr(mix_in), _ptr(moments),
                                _ptr(resp), total_ptr, _ptr(mix_out), _ptr(ws), ws.numel(),
                                _stream(stream))
        _lib.check("g2k_mix_em_f32", rc)

    def stats(self, pred, targets, n_active, *, n_frames=None, ped_mask=None, targets_shared=False,
              stream=None):
        """The E-step alone (g2k_mix_em_f32 without mix_out): this mixture's
        log density over the pairs, the responsibilities' sums and the hard
        assignments -> MixtureStats."""
        return self.em_step(pred, targets, n_active, n_frames=n_frames, ped_mask=ped_mask,
                            targets_shared=targets_shared, update=False, stream=stream)

    def em_step(self, pred, targets, n_active, *, n_frames=None, ped_mask=None, targets_shared=False,
                update=True, stream=None):
        """One EM iteration on the device (g2k_mix_em_f32): the E-step under
        the current ``params`` and, with ``update``, the M-step, whose block
        becomes ``params`` -> the E-step's MixtureStats (the log-likelihood is
        the one BEFORE the update)."""
        lib = load()
        dev = pred.device
        d = self._dims(pred)
        _check_pairs_inputs(d, pred, targets, n_active, n_frames, ped_mask, targets_shared)
        self._check_params(dev)
        moments, resp, total, ws = self._em_buffers(lib, d, dev)
        new = torch.empty_like(self.params) if update else None
        self._em(lib, d, pred, targets, n_active, n_frames, ped_mask, self.params, moments, resp,
                 total.data_ptr(), new, ws, stream)
        if update and d.S > 0:
            self.params = new
        return MixtureStats(moments=moments, resp=resp, total=total[0])

    def fit(self, pred, targets, n_active, *, iters=30, init=None, n_frames=None, ped_mask=None,
            targets_shared=False, stream=None):
        """``iters`` EM iterations, launches only: the blocks ping-pong between
        two device buffers, iteration i's totals land in row i of an [iters, 4]
        buffer, and nothing is read back until the end.  ``init``: None = the
        deterministic start ``init_from`` a no-head full-covariance stats
        launch on the same data with this head's number of live slots; a
        MixtureHead or a block [8, 608] = that mixture (``init=self`` goes on
        from the current one).  Sets ``params`` -> MixtureFit; ValueError when
        there is no pair."""
        from .fullcov import FullCovHead
        lib = load()
        iters = int(iters)
        if iters < 1:
            raise ValueError(f"iters = {iters}: >= 1")
        dev = pred.device
        d = self._dims(pred)
        _check_pairs_inputs(d, pred, targets, n_active, n_frames, ped_mask, targets_shared)
        if init is None:
            st = FullCovHead(device=dev).stats(pred, targets, n_active, (), n_frames=n_frames,
                                               ped_mask=ped_mask, targets_shared=targets_shared,
                                               use_head=False, stream=stream)
            if st.pairs == 0:
                raise ValueError("fit: no (scene, frame, pedestrian) pair to fit the head on")
            start = MixtureHead.init_from(st, self.components, device=dev).params
        elif isinstance(init, MixtureHead):
            start = init.params
        else:
            start = MixtureHead.from_block(init, device=dev).params
        self._check_params(dev, start)
        moments, resp, totals, ws = self._em_buffers(lib, d, dev, rows=iters)
        bufs = [start.clone(), torch.empty_like(start)]
        for i in range(iters):
            self._em(lib, d, pred, targets, n_active, n_frames, ped_mask, bufs[i & 1], moments, resp,
                     totals.data_ptr() + 32 * i, bufs[(i + 1) & 1], ws, stream)
        t = totals.cpu().numpy()
        pairs = int(t[0, 0])
        if pairs == 0:
            raise ValueError("fit: no (scene, frame, pedestrian) pair to fit the head on")
        self.params = bufs[iters & 1]
        return MixtureFit(loglik=t[:, 1] / t[:, 0], pairs=pairs, resp=resp)

    def sample(self, pred, seed=0, want_components=False, stream=None):
        """One draw around pred [S, F, 2L, Nmax] (same layout out); with
        ``want_components`` -> (draw, comp [S, F, Nmax] int32, the component
        each trajectory was drawn from)."""
        lib = load()
        d = self._dims(pred)
        _check_dev("pred", pred, pred.device, torch.float32)
        self._check_params(pred.device)
        out = torch.empty_like(pred)
        comp = torch.empty((d.S, d.F, d.Nmax), dtype=torch.int32, device=pred.device) \
            if want_components else None
        rc = lib.g2k_mix_sample_f32(ctypes.byref(d), _ptr(pred), _ptr(self.params),
                                    ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), _ptr(out), _ptr(comp),
                                    _stream(stream))
        _lib.check("g2k_mix_sample_f32", rc)
        return (out, comp) if want_components else out
