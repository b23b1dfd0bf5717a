"""The draw probe's table (tests/test_draw_probe.py checks every claim below
from integers alone; tests/test_draw_probe_gpu.py runs the heads' device-side
draw on the rows): members whose 12 elements e_scene + col + t Nmax lie below,
across and above a multiple of E = 2^32, where the 64-bit element index that the
heads handle in 32-bit halves (csrc/g2k_head_draw.h) carries into its high word.

A row's claim is, per column, the high word of the member's step-0 element
(``hi0``) and the first step whose element has the next high word (``cross``;
None: the member never straddles), and the same for the scene-frame's shared
sweep, column 0's, which only the scene-coupled head makes (``shared``).  Test
helper, not a test module."""
import collections

import numpy as np

E = 1 << 32
L = 12
SEEDS = ((7 << 32) + 99,          # both words plain
         (1 << 64) - 1)           # both words all ones: the coupled head's salt XOR flips every bit of them
SEED_IDS = ("s7", "ones")

Case = collections.namedtuple("Case", "name Nmax e_scene cols hi0 cross shared")

_C7 = tuple(range(7))


def _split3(lo, hi):
    """cols 0..6: ``lo`` for columns below 3, ``hi`` from column 3 on."""
    return tuple(lo if n < 3 else hi for n in _C7)


CASES = [
    # control: the last element is E - 8, the high word 0 throughout
    Case("below", 7, E - 91, _C7, (0,) * 7, (None,) * 7, None),
    # cols >= 3 cross at step 1, cols < 3 at step 2; the shared element (column 0) crosses at step 2, a
    # different step from members 3..6
    Case("t1", 7, E - 7 - 3, _C7, (0,) * 7, _split3(2, 1), 2),
    # the same at steps 6 / 7
    Case("t6", 7, E - 42 - 3, _C7, (0,) * 7, _split3(7, 6), 7),
    # cols >= 3 cross at the last step; cols < 3 and the shared element never cross
    Case("t11", 7, E - 77 - 3, _C7, (0,) * 7, _split3(None, 11), None),
    # column 3's step-0 element is exactly E; cols > 3 lie wholly above (high word 1 from the start); cols
    # < 3 and the shared element cross at step 1
    Case("step0", 7, E - 3, _C7, _split3(0, 1), _split3(1, None), 1),
    # high word 1 -> 2: the carry is the step-0 high word + 1, not the constant 1
    Case("second", 7, 2 * E - 42 - 3, _C7, (1,) * 7, _split3(7, 6), 7),
    # high word 5, no straddle
    Case("above", 7, 5 * E + 123, _C7, (5,) * 7, (None,) * 7, None),
    # the widest stride: cols >= 128 cross at step 6, the others at step 7
    Case("n256", 256, E - 1536 - 128, (0, 127, 128, 255), (0,) * 4, (7, 7, 6, 6), 7),
    # Nmax 1: the member is the shared element; it crosses at step 6
    Case("n1", 1, E - 6, (0,), (0,), (6,), 6),
]
IDS = [c.name for c in CASES]
STRADDLING = [c.name for c in CASES if any(s is not None for s in c.cross) or c.shared is not None]


def first_cross(e0, Nmax):
    """(high word of e0, first step t whose element e0 + t Nmax has a higher one or None)."""
    hi0 = e0 >> 32
    for t in range(L):
        if (e0 + t * Nmax) >> 32 != hi0:
            return hi0, t
    return hi0, None


def params(which):
    """Head ``which``'s parameters: the existing cases' — head, chol and mix
    (three live slots of eight, NaN in the dead ones and above the diagonals)
    of tests/ranks_cases.py's first case, cpl (NaN above the diagonals, Lb of
    its own structure) of tests/scene_ranks_cases.py's second."""
    from tests import ranks_cases, scene_ranks_cases
    if which == "coupled":
        return scene_ranks_cases.inputs(1)["cpl"]
    return ranks_cases.inputs(0)[{"per_step": "head", "fullcov": "chol", "mix": "mix"}[which]]


def unit_params(which):
    """Head ``which``'s parameters under which a draw around mu = 0 is the
    element's two normals themselves: sigma = 1, rho = 0; chol = I; one live
    slot, w = 1, b = 0, L = I; cpl = {I, 0}."""
    from tests import mixture_ref as mr
    eye = np.eye(2 * L, dtype=np.float32)
    if which == "per_step":
        return np.zeros((3, L), np.float32)
    if which == "fullcov":
        return eye
    if which == "mix":
        return mr.block([1.0])
    return np.stack([eye, np.zeros_like(eye)])
