"""The launches of the fixed-frame forward build (g2k_scene_kernel<..., FX =
20>, csrc/g2k_scene.hip) that the parity tests run, as data
(tests/test_step_fixed.py checks the claims on the CPU,
tests/test_step_fixed_wide_gpu.py runs the cases on the GPU).

The build differs from the general kernel in what depends on Nmax and flags:
scene_layout_fixed aliases the position window (27 rows of 2 Nmax floats) onto
the As ring (20 slots of 256) while it fits, 54 Nmax <= 5120: Nmax <= 94.
Wider scenes keep a window of their own for as long as that layout fits
kCoresidentLds (N_LAST); the kernel forms the layout again from Nmax and takes
only the target stride from the host (G2K_STEP_TARGETS_SHARED); W (the rows of
the pos buffer) stays a runtime value.

A case names what it is there to reach and carries what it claims of the
launch: the window aliased or its own, the prediction tiles (16 columns each,
dealt over four producer waves) and the workgroups a CU holds.  Inputs come
from synthetic.make_batch(S = 4, ..., h0_scale = 1.0), expected outputs from
oracle.g2k_ref.scene_step per scene, cached per (H, Nmax, n_frames, targets
shared) and shared read-only by both pred layouts.
"""
from __future__ import annotations

import ctypes
import functools
from dataclasses import dataclass

import numpy as np

from multimodaltraj_2_amd import _lib
from multimodaltraj_2_amd import frame_step as fs
from multimodaltraj_2_amd.synthetic import make_batch
from oracle import g2k_ref as ref

F, S = 20, 4
W_PLAIN = F - 1 + fs.OBS_LEN          # 27: the window of a stride-1 scene
RING = F * fs.HIDDEN_LEN * fs.HIDDEN_LEN   # the As ring, floats
CU_LDS = 160 * 1024
N_ALIAS = 94                          # 54 * 94 = 5076 <= 5120 < 54 * 95


def fixed_range(H=128):
    """The Nmax in 1..256 whose co-resident F = 20 launch takes the fixed build."""
    return [n for n in range(1, 257)
            if fs.step_fixed_geometry(S, F, H, n, coresident=True)["frames"] == F]


# The largest Nmax of the fixed build, as the library answers (host arithmetic;
# tests/test_step_fixed.py pins the number and that the range has no holes)
N_LAST = max(fixed_range())


def mid_active(Nmax):
    """n_active of the third scene: about 4/5 of Nmax, ending inside a tile at
    neither its first nor its last column (so the last tiles of a wide scene
    hold nobody)."""
    m = Nmax - Nmax // 5
    while (m - 1) % 16 in (0, 15):
        m -= 1
    return m


N_FRAMES = {"frames-1-0-20-13": (1, 0, 20, 13), "frames-none": None}
REACHES = {
    32: "two tiles, the benchmark's width (the twins of the shared-target and long-pos launches)",
    33: "3 tiles, odd (4-byte position DMA, the mask not one load)",
    48: "3 full tiles, Nmax % 4 == 0 (16-byte segments)",
    64: "4 tiles with a partial n_active, a mask and short n_frames",
    93: "aliased, odd, 6 tiles (the tile loop wraps over 4 producers)",
    94: "aliased, the last window that fits the ring (5076 of 5120 floats), Nmax % 4 == 2, wide DMA",
    95: "the first window of its own, odd",
    N_LAST: "the largest Nmax of the fixed build",
}


@dataclass(frozen=True)
class Case:
    id: str
    H: int
    Nmax: int
    layout: str                  # pred layout: "band" / "ped"
    n_active: tuple              # per scene
    frames_id: str               # key of N_FRAMES
    masked: tuple                # (scene, column) pairs with ped_mask 0
    targets_shared: bool = False
    extra_rows: int = 0          # rows of pos past the window (W = 27 + extra_rows)
    # what the case claims of its launch
    aliased: bool = True         # the window shares the ring's space
    tiles: int = 1
    wgs_per_cu: int = 3
    reaches: str = ""

    @property
    def n_frames(self):
        return N_FRAMES[self.frames_id]

    @property
    def frames(self):
        """Frames per scene that run."""
        return (F,) * S if self.n_frames is None else self.n_frames

    @property
    def W(self):
        return W_PLAIN + self.extra_rows

    @property
    def key(self):
        return (self.H, self.Nmax, self.frames_id, self.targets_shared)

    def mask(self):
        m = np.ones((S, self.Nmax), bool)
        for s, col in self.masked:
            m[s, col] = False
        return m


def _case(kind, H, Nmax, layout, frames_id, **kw):
    n_active = (0, 1, mid_active(Nmax), Nmax)
    # the widest scene: one masked pedestrian in the first tile, one in the
    # middle of the last (the tile's other columns keep their pairs)
    last = (Nmax - 1) // 16 * 16
    masked = ((3, 5), (3, last + (Nmax - 1 - last) // 2))
    lds = 3 if Nmax <= 48 else 2          # (13,368 floats fit three times at 48, 13,788 at 64 do not)
    return Case(f"{kind}-h{H}-n{Nmax}-{layout}-{frames_id}", H, Nmax, layout, n_active, frames_id,
                masked, aliased=Nmax <= N_ALIAS, tiles=(Nmax + 15) // 16,
                wgs_per_cu=min(lds, 3 if H < 256 else 2), reaches=REACHES[Nmax], **kw)


def _outputs():
    shapes = [(128, n) for n in (33, 48, 64, 93)]
    shapes += [(H, n) for n in (94, 95, N_LAST) for H in (64, 128, 256)]
    return [_case("out", H, n, layout, fid)
            for H, n in shapes for layout in ("band", "ped") for fid in N_FRAMES]


OUTPUT_CASES = _outputs()
SHARED_CASES = [_case("shared", 128, n, layout, "frames-1-0-20-13", targets_shared=True)
                for n in (32, 94, 95) for layout in ("band", "ped")]
LONG_POS_CASES = [_case("longpos", 128, n, layout, "frames-1-0-20-13", extra_rows=3)
                  for n in (32, 94) for layout in ("band", "ped")]
CASES = OUTPUT_CASES + SHARED_CASES + LONG_POS_CASES


def plain_twin(case):
    """The same launch with a target set per frame and a pos buffer of the window's rows."""
    return _case("plain", case.H, case.Nmax, case.layout, case.frames_id)


def dims(case, coresident=True):
    """The g2k_dims of the case's launch (W as the case has it)."""
    return _lib.G2KDims(S, F, fs.OBS_LEN, fs.PRED_LEN, fs.HIDDEN_LEN, case.H, case.Nmax, case.W, 1,
                        fs.step_flags(case.layout, case.targets_shared, coresident=coresident))


def fixed_geometry(case, coresident=True):
    """fs.step_fixed_geometry for the case's own dims: frame_step's wrapper
    derives W from F and the stride, a long pos buffer has more."""
    lib = _lib.bind(_lib.load(), "step_fixed", fs.FIXED_SYMBOLS)
    d = dims(case, coresident)
    out = (ctypes.c_int32 * len(fs.FIXED_GEOM_FIELDS))()
    _lib.check("g2k_step_fixed_geometry", lib.g2k_step_fixed_geometry(ctypes.byref(d), 0, 1, 256, out))
    return dict(zip(fs.FIXED_GEOM_FIELDS, (int(v) for v in out)))


@functools.lru_cache(maxsize=None)
def reference(key):
    """(batch, want) of a case's key (H, Nmax, frames_id, targets_shared):
    the make_batch inputs — with shared targets, frame 0's target set in every
    frame — and per scene the oracle's (pred, h, metrics, frames run).  The mask
    is the same for every case of an Nmax.  Computed once, shared read-only."""
    H, Nmax, frames_id, shared = key
    c = _case("ref", H, Nmax, "band", frames_id, targets_shared=shared)
    b = make_batch(S, Nmax, H, F=F, seed=131 + Nmax, n_active=np.array(c.n_active, np.int32),
                   h0_scale=1.0)
    if shared:
        b.targets = np.ascontiguousarray(np.broadcast_to(b.targets[:, :1], b.targets.shape))
    mask = c.mask()
    w = fs.init_params(Nmax, seed=0).numpy()
    want = []
    for s in range(S):
        nf = c.frames[s]
        pr, h, m, _ = ref.scene_step(b.pos[s], b.vislet[s], b.G[s], w, b.targets[s], c.n_active[s],
                                     b.h0[s], n_frames=nf, stride=1, ped_mask=mask[s])
        for a in (pr, h, m):
            a.setflags(write=False)
        want.append((pr, h, m, nf))
    for a in (b.pos, b.vislet, b.G, b.targets, b.n_active, b.h0):
        a.setflags(write=False)
    return b, tuple(want)
