"""The launches of g2k_encoder_chain_f32 that the parity tests run, as data,
and the float64 restatement of the chain they are held to
(tests/test_encoder_chain_cases.py checks the claims on the CPU,
tests/test_encoder_chain_builds_gpu.py runs the cases on the GPU).

encoder_chain_launch (csrc/g2k_ops.hip) builds twelve instantiations of
g2k_encoder_chain_kernel<TPW, U, FS>: H 64 / 128 / 256 / 512 x (num_units,
feature_size) (1, 2) / (2, 4) / (4, 8).  Each has its own cell (chain_cell:
16 U lanes, K = 16 / FS frequency blocks, the units of a row trading m_freq
by DPP quad permutes), so each needs its own launch against the oracle.

Why every case starts from an O(1) h0: after ONE recurrence frame every entry
of h is 1/H to three digits, so the state the cell reads, h[:, :16], is almost
constant from the second frame of a launch on, and a state-wiring error in the
cell (the wrong unit's c_time, the c / m halves exchanged, a wrong block
offset) moves Xe by 1e-2 and more only in the FIRST frame of a launch with an
O(1) h0 (measured with this oracle at u 2, H 64: 0.96, 9.5e-3, 1.8e-4, 3.3e-6,
4.5e-8 in frames 0..4).  test_encoder_chain_cases.py asserts that the inputs
built here can tell such a kernel from a right one.

A case names the branch of the kernel it is there to reach.  Inputs come from
one seeded builder (the footprint test's choices, which keep A, cost and pred
O(1)): X scale 0.5, Rel = N(0, 1)^2, cell W scale 0.7, b scale 0.3, peep
N(0, 1), h0 = h0_scale N(0, 1), lambda 0.1.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, replace

import numpy as np

from oracle import g2k_ref as ref

D, T, L2 = 16, 8, 24
LAM = 0.1
HS = (64, 128, 256, 512)
SHAPES = ((1, 2), (2, 4), (4, 8))              # (num_units, feature_size) the launcher builds
BUILDS = {(H, u) for H in HS for u, _ in SHAPES}


@dataclass(frozen=True)
class Case:
    id: str
    H: int
    u: int                       # num_units; feature_size = 2 u
    peep: bool
    Nmax: int
    F: int
    n_active: tuple              # per batch
    n_frames: tuple              # per batch, as handed to the kernel (may lie outside [0, F])
    seed: int
    branch: str                  # what the case is there to reach
    h0_scale: float = 1.0
    rel_scale: tuple = ()        # per batch factor on Rel (large logits); () = 1

    @property
    def fs(self):
        return 2 * self.u

    @property
    def K(self):
        return D // self.fs

    @property
    def S(self):
        return len(self.n_frames)

    @property
    def frames(self):
        """Frames per batch that run: n_frames clamped to [0, F] (include/g2k_hip.h)."""
        return tuple(min(max(int(n), 0), self.F) for n in self.n_frames)

    @property
    def run(self):
        """[S, F] bool: the frames that run."""
        m = np.zeros((self.S, self.F), bool)
        for s, n in enumerate(self.frames):
            m[s, :n] = True
        return m


def _f32(rng, *shape, scale=1.0):
    return (scale * rng.standard_normal(shape)).astype(np.float32)


def build(case):
    """The case's float32 inputs (host arrays), from its seed alone."""
    rng = np.random.default_rng(case.seed)
    S, F, N, u, fs = case.S, case.F, case.Nmax, case.u, case.fs
    w = dict(Wi=_f32(rng, N, D), Wii=_f32(rng, D, T), Wv=_f32(rng, T, D + 2), bv=_f32(rng, D),
             Wr=_f32(rng, T, 2), Wc=_f32(rng, L2, T), Wo=_f32(rng, T, N))
    X, Rel, G = _f32(rng, S, F, D + 2, D, scale=0.5), _f32(rng, S, 2, D) ** 2, _f32(rng, S, D, T)
    if case.rel_scale:
        Rel = Rel * np.asarray(case.rel_scale, np.float32)[:, None, None]
    cW, cb, cP = _f32(rng, fs + 2 * u, 3 * u, scale=0.7), _f32(rng, 3 * u, scale=0.3), _f32(rng, 4, u)
    h0 = _f32(rng, D, case.H, scale=case.h0_scale)
    return dict(w=w, X=X, Rel=Rel, G=G, cW=cW, cb=cb, cP=cP if case.peep else None, h0=h0,
                n_active=np.asarray(case.n_active, np.int32),
                n_frames=np.asarray(case.n_frames, np.int32))


def cell_ref(case, inp, x, state):
    """The oracle's cell on one frame's x [D, D] with ``state`` [D, >= 16]."""
    peep = None if inp["cP"] is None else tuple(inp["cP"].astype(np.float64))
    return ref.gridlstm_cell(x, state, inp["cW"], inp["cb"], peep, feature_size=case.fs,
                             num_units=case.u)


def chain_ref(case, inp=None):
    """The chain in float64: batch after batch, frame after frame, the cell on
    X[s][f][:D] with h as its state, the one-feed forward from [Xe; X[s][f][D:]],
    one recurrence frame.  Returns Xe [S, F, D, D], attn [S, F, D, D], cost
    [S, F, T, T] and pred [S, F, 2L, Nmax] (meaningful where ``run``; pred zero
    in the columns >= n_active), ``state`` = the cell's new state of the last run
    frame (None when no frame runs) and the final h [D, H]."""
    inp = build(case) if inp is None else inp
    f64 = lambda a: np.asarray(a, np.float64)                   # noqa: E731
    S, F, N = case.S, case.F, case.Nmax
    w, X = inp["w"], inp["X"]
    out = dict(Xe=f64(X[:, :, :D]).copy(), attn=np.zeros((S, F, D, D)), cost=np.zeros((S, F, T, T)),
               pred=np.zeros((S, F, L2, N)), run=case.run, state=None)
    h = f64(inp["h0"])
    for s, nf in enumerate(case.frames):
        n = min(max(int(case.n_active[s]), 0), N)
        for f in range(nf):
            x0, st = cell_ref(case, inp, X[s, f, :D], h)
            o = ref.mcr_forward(*map(f64, (np.concatenate((x0, X[s, f, D:])), inp["Rel"][s],
                                           inp["G"][s], w["Wv"], w["bv"], w["Wr"], w["Wc"],
                                           w["Wo"][:, :n])), LAM)
            out["Xe"][s, f], out["attn"][s, f], out["cost"][s, f] = x0, o["attn"], o["cost"]
            out["pred"][s, f, :, :n] = o["pred_path_band"].reshape(L2, n)
            out["state"] = st
            h = ref.recurrence_step(o["attn"], h)
    out["h"] = h
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """(inputs, chain_ref) of a case, computed once and shared read-only."""
    inp = build(case)
    out = chain_ref(case, inp)
    for a in list(inp.values()) + list(inp["w"].values()) + list(out.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return inp, out


def column_spread(A):
    """The widest max - min of a column of A [D, D]."""
    return float((A.max(axis=0) - A.min(axis=0)).max())


def min_prefix(A):
    """The smallest sum_{k<=r} exp(A_k - max of the column) over rows r and
    columns of A: attn_tile_wave leaves its main path below 1e-30."""
    return float(np.cumsum(np.exp(A - A.max(axis=0)), axis=0).min())


# ---------------------------------------------------------------------------
# every build, with and without peepholes
# ---------------------------------------------------------------------------
BUILD_FRAMES = (0, 3, 0, 1, 2, 0)     # leading / middle / trailing skipped batch, a one-frame batch
BUILD_ACTIVE = (5, 17, 9, 0, 1, 3)    # the batches that run: Nmax, 0 and 1


# a case whose plain seed misses test_encoder_chain_cases.py's 1e-2 bar takes another one
# (build-h512-u1-peep: x block 1 zeroed moved output block 2 by 9.7e-3)
RESEED = {"build-h512-u1-peep": 1}


def _build_cases():
    out = []
    for H in HS:
        for u, _ in SHAPES:
            for peep in (True, False):
                cid = f"build-h{H}-u{u}-{'peep' if peep else 'nopeep'}"
                out.append(Case(
                    cid, H, u, peep, 17, 3, BUILD_ACTIVE, BUILD_FRAMES,
                    seed=41000 + 10 * H + 2 * u + peep + 100000 * RESEED.get(cid, 0),
                    branch=f"<{H // 64}, {u}, {2 * u}>: skipped batches before, between and after; "
                           "both parities of cur; a one-frame batch; pred flushed after a batch "
                           "boundary and after the last frame; n_active Nmax, 0, 1"))
    return out


BUILD_CASES = _build_cases()

# ---------------------------------------------------------------------------
# edges: u 1 and u 4 at H 64 and 512
# ---------------------------------------------------------------------------
EDGE_BUILDS = ((64, 1), (64, 4), (512, 1), (512, 4))
# Rel factors of the large-logit cases (batch 0 plain, batch A, batch B), found on the CPU
# with this oracle; test_encoder_chain_cases.py asserts what they are for
LOGIT_SCALES = {(64, 1): (1.0, 5.0, 12.0), (64, 4): (1.0, 10.0, 20.0),
                (512, 1): (1.0, 6.0, 12.0), (512, 4): (1.0, 15.0, 40.0)}


def _edge(kind, H, u, **kw):
    seeds = {"nmax1": 1, "nmax256": 2, "clamp": 3, "none": 4, "nan": 5, "logits": 6, "wide-h0": 7}
    return Case(f"{kind}-h{H}-u{u}", H, u, True, seed=52000 + 100 * seeds[kind] + 10 * (H // 64) + u,
                **kw)


NMAX_CASES, CLAMP_CASES, NONE_CASES, NAN_CASES, LOGIT_CASES = [], [], [], [], []
for _H, _u in EDGE_BUILDS:
    NMAX_CASES.append(_edge("nmax1", _H, _u, Nmax=1, F=2, n_active=(1, 1), n_frames=(2, 2),
                            branch="Nmax 1: pred_of and the Wo staging with one column"))
    NMAX_CASES.append(_edge("nmax256", _H, _u, Nmax=256, F=2, n_active=(256, 130), n_frames=(2, 2),
                            branch="Nmax 256: sWo full, pred_of walks 6144 entries on 192 threads "
                                   "under the next frame's cell"))
    CLAMP_CASES.append(_edge("clamp", _H, _u, Nmax=17, F=2, n_active=(17, 9), n_frames=(5, -2),
                             branch="n_frames F + 3 and -2: clamped to F and 0"))
    NONE_CASES.append(_edge("none", _H, _u, Nmax=17, F=2, n_active=(17, 9, 1), n_frames=(0, 0, 0),
                            branch="no batch has frames: h in, h out, nothing else"))
    NAN_CASES.append(_edge("nan", _H, _u, Nmax=17, F=3, n_active=(5, 17, 9, 3), n_frames=(2, 0, 3, 1),
                           branch="NaN in every inactive input: frames >= n_frames, the skipped "
                                  "batch, Wo's columns >= the widest running batch"))
    LOGIT_CASES.append(_edge("logits", _H, _u, Nmax=17, F=2, n_active=(17, 9, 5), n_frames=(2, 2, 2),
                             rel_scale=LOGIT_SCALES[(_H, _u)],
                             branch="attn_tile_wave inside the chain: its main path at its widest "
                                    "(batch 1) and its running-(max, sum) fallback (batch 2)"))
WIDE_H0_CASE = _edge("wide-h0", 512, 4, Nmax=17, F=3, n_active=(17, 9), n_frames=(3, 2), h0_scale=10.0,
                     branch="h0 = 10 N(0, 1): frame 0's row-max shift, saturated gates in the cell")
REPEAT_CASES = [c for c in BUILD_CASES if c.id in ("build-h64-u1-peep", "build-h256-u2-peep",
                                                   "build-h512-u4-peep")]


def clamped_twin(case):
    """The same launch with n_frames already inside [0, F]."""
    return replace(case, id=case.id + "-twin", n_frames=case.frames)


def wo_twin(case):
    """The same launch with every n_active <= 1 (Wo's columns >= 1 are then inactive)."""
    return replace(case, id=case.id + "-wo", n_active=tuple(min(n, 1) for n in case.n_active))


EDGE_CASES = NMAX_CASES + CLAMP_CASES + NONE_CASES + NAN_CASES + LOGIT_CASES + [WIDE_H0_CASE]
CASES = BUILD_CASES + EDGE_CASES
