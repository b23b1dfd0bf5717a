"""The inputs of the scene-coupled head's tests (tests/test_coupled_head.py on
the CPU, tests/test_coupled_head_gpu.py on the device): tests/couples_cases.py's
``inputs(i)`` — the same shapes, masks and NaN poison — with the head's
parameter block ``cpl`` [2, 24, 24] = {Lw, Lb} added.  Even cases cut the
case's full-covariance law in two as ``CoupledHead.from_fullcov(chol, 0.6)``
does (Lb a multiple of Lw); odd cases give the shared part a covariance of its
own (slower decay over the steps, other scales: Lb no multiple of Lw).  Entries
above the diagonals hold NaN: they are never read.

The stats launch deals WHOLE scene-frames to its workgroups (csrc/
g2k_coupled.hip: per = ceil(256 / Nmax) scene-frames each at least, W =
min(256, ceil(S F / per)) workgroups), so a range never ends inside a
scene-frame; ``stats_geometry`` restates that and STATS names what each case
reaches.  Test helper, not a test module."""
import functools

import numpy as np

from tests import couples_cases as cc
from tests.bestk_ref import pair_mask

L = 12
DIM = 24
SHARE = 0.6
IDS = cc.IDS


def factors(chol, odd, rng):
    """{Lw, Lb} float64 from a case's full-covariance factor."""
    chol = np.tril(np.asarray(chol, np.float64))
    if not odd:
        return np.sqrt(1.0 - SHARE) * chol, np.sqrt(SHARE) * chol
    T = 0.95 ** np.abs(np.subtract.outer(np.arange(L), np.arange(L)))
    sc = rng.uniform(0.3, 1.0, DIM)
    Bc = np.kron(T, np.array([[1.0, 0.3], [0.3, 1.0]])) * np.outer(sc, sc)
    return np.sqrt(0.5) * chol, np.linalg.cholesky(Bc)


@functools.lru_cache(maxsize=None)
def inputs(i):
    """couples_cases.inputs(i) plus cpl [2, 24, 24] float32 (NaN above the diagonals)."""
    c = dict(cc.inputs(i))
    Lw, Lb = factors(c["chol"], i % 2 == 1, np.random.default_rng(9100 + i))
    cpl = np.stack([Lw, Lb]).astype(np.float32)
    cpl[:, np.triu_indices(DIM, 1)[0], np.triu_indices(DIM, 1)[1]] = np.nan
    c["cpl"] = cpl
    return c


def stats_geometry(S, F, N):
    """(W workgroups, U scene-frames each) of g2k_coupled_stats_f32."""
    sf = S * F
    per = -(-256 // N)
    W = max(1, min(256, -(-sf // per)))
    return W, -(-sf // W)


# what the stats tests run: a couples case, and n_active replaced or not
#         name       case     n_active       reaches
STATS = [("k2",      "k2",    None),         # one workgroup writes the outputs itself; P = 8, 2, 1, 0; n_frames < F
         ("k20",     "k20",   None),         # masked members, an empty scene
         ("reach",   "reach", None),         # two workgroups: the rows path; P = 21
         ("shared",  "shared", None),        # G2K_STEP_TARGETS_SHARED, masked, n_frames < F
         ("k23",     "k23",   None),         # Nmax 40: no divisor of 256
         ("n256",    "n256",  None),         # a scene-frame per workgroup, every column a member
         ("deal",    "deal",  None),         # 64 workgroups of 4 scene-frames; random P, masked
         ("single",  "k2",    [1, 1, 1, 0]),  # N == G: no scene-frame with two members
         ("nopair",  "k2",    [0, 0, 0, 0])]  # no pair at all
STATS_IDS = [s[0] for s in STATS]


@functools.lru_cache(maxsize=None)
def stats_inputs(j):
    """STATS[j] -> the case's dict with n_active replaced (its members are a
    subset of the case's, so what is poisoned stays unread) and ``members``."""
    _, case, nact = STATS[j]
    c = dict(inputs(IDS.index(case)))
    if nact is not None:
        c["n_active"] = np.array(nact, np.int32)
        S, F, _, N = c["pred"].shape
        c["members"] = pair_mask(S, F, N, c["n_active"], c["n_frames"], c["ped_mask"])
    return c


def coupled_law_targets(pred, Lw, Lb, members_per_frame, rng):
    """Targets [S, F, N, L, 2] float32 around pred whose residuals follow the
    head's own law, r = Lb zc + Lw z, for the property and the fit tests."""
    S, F, _, N = pred.shape
    zc = rng.standard_normal((S, F, 1, DIM))
    z = rng.standard_normal((S, F, N, DIM))
    r = zc @ np.asarray(Lb).T + z @ np.asarray(Lw).T                      # [S, F, N, 24] time-major
    mu = np.stack([pred[:, :, :L], pred[:, :, L:]], axis=-1).transpose(0, 1, 3, 2, 4)   # [S, F, N, L, 2]
    return (mu + r.reshape(S, F, N, L, 2)).astype(np.float32)
