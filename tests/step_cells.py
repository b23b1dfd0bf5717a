"""The cells of the fused scene kernel's dispatch that the parity tests run,
as data (tests/test_step_cells.py checks the claims on the CPU,
tests/test_step_cells_gpu.py runs the cells against the float64 oracle).

The scene kernel (csrc/g2k_scene.hip) is a family of template
instantiations picked at launch (launch_np / launch_kp) on top of an LDS
layout (scene_layout) with its own thresholds.  A cell names one launch —
entry point, dims, flags, scenes — and the geometry it is there to reach:
the kernel variant, TPW, NP, the frames per chunk fc, the chunk count for F,
dwo_seq, own0 and the split.  The claim is what the cell is FOR; when a
threshold moves, test_step_cells.py fails instead of the cell silently
running some other build.  A claim is never edited to follow the library: the
cell's F / stride / Nmax are moved until the claim is reached again.

entry: "fwd" = g2k_step_fused_f32 (fs.step_fused, want_attn), "train" =
g2k_train_step_f32 (ts.TrainPlan with h0: the build of the real H), "grad" =
g2k_step_grad_f32 (ts.GradPlan: no h_in, the H = 64 build whatever H says).
split 0 = automatic (resolved for 256 CUs, an MI355X).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

CUS = 256          # the automatic split's device: an MI355X


@dataclass(frozen=True)
class Cell:
    id: str
    entry: str                     # "fwd" | "train" | "grad"
    H: int
    Nmax: int
    F: int
    stride: int = 1
    loss: str = "l2"               # train / grad
    layout: str = "band"           # pred layout: "band" | "ped"
    shared: bool = False           # G2K_STEP_TARGETS_SHARED
    split: int = 1                 # 0: automatic
    coresident: bool = False       # fwd only
    n_active: tuple = ()           # per scene; () = default_n_active
    n_frames: tuple = ()           # per scene; () = default_n_frames(claim)
    zero_fill: bool = False        # inactive columns of pos / vislet / targets zeroed (real-data form)
    pred_tol: float = 1e-4         # close() bound of pred (test_step_cells_gpu.py MEASURED where wider)
    claim: dict = field(default_factory=dict)   # variant tpw np fc chunks dwo_seq own0 split

    @property
    def scenes(self):
        return self.n_active or default_n_active(self.Nmax)

    @property
    def frames(self):
        return self.n_frames or default_n_frames(self.F, self.claim["fc"], self.claim["chunks"])

    @property
    def S(self):
        return len(self.scenes)


def default_n_active(Nmax):
    """One scene at Nmax, one crossing a 16-column tile by one (33, or 17 below
    Nmax 34), one at about two thirds (an odd residue)."""
    cross = 33 if Nmax >= 34 else 17
    return (Nmax, min(cross, Nmax), max(2 * Nmax // 3 - 1, 1))


def default_n_frames(F, fc, chunks):
    """One scene with every frame (so the chunk claim is what runs), one ending
    one frame into the last chunk, one ending one frame into the second chunk
    (three chunks or more) or two frames short."""
    last = (chunks - 1) * fc + 1
    third = fc + 1 if chunks >= 3 else max(F - 2, 1)
    return (F, last, third)


def ped_mask(S, Nmax):
    """[S, Nmax] bool: masked pedestrians at several residues mod 4 in every
    scene (1, 6, 11, 16, ... / 2, 9, 16, 23, ... / 3, 9, 15, 21, ...); pedestrian 0
    always has a target (the n_active = 1 scenes keep their one pair)."""
    m = np.ones((S, Nmax), bool)
    for s in range(S):
        start, step = ((1, 5), (2, 7), (3, 6))[s % 3]
        m[s, start::step] = False
    return m


def _c(variant, tpw, np_, fc, chunks, dwo_seq=0, own0=0, split=1):
    return dict(variant=variant, tpw=tpw, np=np_, fc=fc, chunks=chunks, dwo_seq=dwo_seq,
                own0=own0, split=split)


N01 = dict(n_active=(0, 1, 20), n_frames=(5, 4, 5), zero_fill=True)

FORWARD = [
    # H 512: the lone-launch NP 4 build <8, 4>
    Cell("fwd-h512-band", "fwd", 512, 32, 20, claim=_c("general", 8, 4, 20, 1)),
    Cell("fwd-h512-ped", "fwd", 512, 32, 20, layout="ped", claim=_c("general", 8, 4, 20, 1)),
    Cell("fwd-h512-split3", "fwd", 512, 32, 20, split=3, claim=_c("general", 8, 4, 20, 1, split=3)),
    Cell("fwd-h512-stride2", "fwd", 512, 32, 12, stride=2, claim=_c("general", 8, 4, 12, 1)),
    Cell("fwd-h512-coresident", "fwd", 512, 32, 20, split=0, coresident=True,
         claim=_c("general", 8, 4, 20, 1)),
    # the co-resident 8-wave builds <1, 4> <2, 4> <4, 4>
    Cell("fwd-h64-coresident", "fwd", 64, 32, 20, split=0, coresident=True,
         claim=_c("general", 1, 4, 20, 1)),
    Cell("fwd-h128-coresident", "fwd", 128, 32, 20, split=0, coresident=True,
         claim=_c("general", 2, 4, 20, 1)),
    Cell("fwd-h256-coresident", "fwd", 256, 32, 20, split=0, coresident=True,
         claim=_c("general", 4, 4, 20, 1)),
    # loop-invariant frames: stride 0, shared targets, automatic split, two chunks (32 + 8)
    Cell("fwd-inv-h64", "fwd", 64, 32, 40, stride=0, shared=True, split=0, n_frames=(40, 33, 37),
         claim=_c("inv", 1, 12, 32, 2)),
    Cell("fwd-inv-h256", "fwd", 256, 32, 40, stride=0, shared=True, split=0, n_frames=(40, 33, 37),
         claim=_c("inv", 4, 12, 32, 2)),
    Cell("fwd-inv-h512", "fwd", 512, 32, 40, stride=0, shared=True, split=0, n_frames=(40, 33, 37),
         claim=_c("inv", 8, 4, 32, 2)),
    Cell("fwd-inv-n85", "fwd", 128, 85, 40, stride=0, shared=True, split=0, n_frames=(40, 33, 37),
         claim=_c("inv", 2, 12, 32, 2)),
    Cell("fwd-inv-ped", "fwd", 128, 32, 40, stride=0, shared=True, split=0, layout="ped",
         n_frames=(40, 33, 37), claim=_c("inv", 2, 12, 32, 2)),
    # the first width off the path: the general kernel with one target set (tfb == 0);
    # automatically split over 4 workgroups, and in one
    Cell("fwd-inv-n86-general", "fwd", 128, 86, 40, stride=0, shared=True, split=0,
         n_frames=(40, 33, 37), pred_tol=4.5e-4,
         claim=_c("general", 2, 12, 32, 2, split=4)),
    Cell("fwd-inv-n86-general-split1", "fwd", 128, 86, 40, stride=0, shared=True, split=1,
         n_frames=(40, 33, 37), claim=_c("general", 2, 12, 32, 2)),
    # the layout's halving loop: fc 16 (16 + 16 + 8), 10 (10 + 10), 16
    Cell("fwd-halved-n256-s1", "fwd", 64, 256, 40, pred_tol=1.46e-3,
         claim=_c("general", 1, 12, 16, 3)),
    Cell("fwd-halved-n256-s2", "fwd", 64, 256, 20, stride=2, pred_tol=7.8e-4,
         claim=_c("general", 1, 12, 10, 2)),
    Cell("fwd-halved-n200-s2", "fwd", 64, 200, 40, stride=2, pred_tol=6.6e-4,
         claim=_c("general", 1, 12, 16, 3)),
    # overlapping and disjoint windows
    Cell("fwd-stride3", "fwd", 128, 30, 6, stride=3, claim=_c("general", 2, 12, 6, 1)),
    Cell("fwd-stride9", "fwd", 128, 30, 6, stride=9, claim=_c("general", 2, 12, 6, 1)),
    # empty and one-pedestrian scenes
    Cell("fwd-n01", "fwd", 64, 20, 5, claim=_c("general", 1, 12, 5, 1), **N01),
]

TRAIN = [
    # strides other than 1 (dV over overlapping / disjoint windows, wcmax), per-frame targets
    Cell("train-stride2", "train", 128, 32, 12, stride=2, claim=_c("general", 2, 8, 12, 1)),
    Cell("train-stride3-ped", "train", 128, 32, 12, stride=3, layout="ped",
         claim=_c("general", 2, 8, 12, 1)),
    Cell("train-stride9", "train", 128, 32, 12, stride=9, claim=_c("general", 2, 8, 6, 2)),
    Cell("train-stride0-per-frame", "train", 128, 32, 12, stride=0,
         claim=_c("general", 2, 8, 12, 1)),
    Cell("train-nll-stride2", "train", 128, 32, 12, stride=2, loss="nll",
         claim=_c("nll", 2, 8, 6, 2)),
    # the no-h_in entry point: the H = 64 build whatever H says
    Cell("grad-l2-stride2", "grad", 128, 32, 12, stride=2, claim=_c("general", 1, 8, 12, 1)),
    Cell("grad-nll-stride2", "grad", 128, 32, 12, stride=2, loss="nll",
         claim=_c("nll", 1, 8, 6, 2)),
    # NLL with dWo^T added in frame order (Nmax >= 86 at NP 8), small fc
    Cell("train-nll-n86-ped", "train", 128, 86, 9, loss="nll", layout="ped",
         claim=_c("nll", 2, 8, 9, 1, dwo_seq=1)),
    Cell("train-nll-n256-f9", "train", 128, 256, 9, loss="nll",
         claim=_c("nll", 2, 8, 3, 3, dwo_seq=1)),
    Cell("train-nll-n256-f20", "train", 128, 256, 20, loss="nll",
         claim=_c("nll", 2, 8, 3, 7, dwo_seq=1)),
    Cell("train-nll-n256-s2", "train", 128, 256, 9, stride=2, loss="nll",
         claim=_c("nll", 2, 8, 2, 5, dwo_seq=1)),
    # fc == 1: F 37 is the shortest at stride 2 (36 still holds two frames), F 10 at stride 3
    Cell("train-nll-n256-fc1-s2", "train", 128, 256, 37, stride=2, loss="nll",
         n_active=(256, 33), n_frames=(37, 3), claim=_c("nll", 2, 8, 1, 37, dwo_seq=1)),
    Cell("train-nll-n256-fc1-s3", "train", 128, 256, 10, stride=3, loss="nll",
         claim=_c("nll", 2, 8, 1, 10, dwo_seq=1)),
    Cell("train-nll-n256-split3", "train", 128, 256, 9, loss="nll", split=3,
         claim=_c("nll", 2, 8, 3, 3, dwo_seq=1, split=3)),
    # H 512: the 4-producer train build (dwo_seq from Nmax 129)
    Cell("train-h512-nll-n48", "train", 512, 48, 12, loss="nll", claim=_c("nll", 8, 4, 12, 1)),
    Cell("train-h512-nll-n200", "train", 512, 200, 9, loss="nll",
         claim=_c("nll", 8, 4, 9, 1, dwo_seq=1)),
    Cell("train-h512-l2-n200", "train", 512, 200, 9, claim=_c("general", 8, 4, 9, 1, dwo_seq=1)),
    # block ownership (two workgroups per scene, L2)
    Cell("train-blk-h64-ped", "train", 64, 32, 20, split=2, layout="ped",
         claim=_c("blk", 1, 8, 20, 1, own0=8, split=2)),
    Cell("train-blk-h512", "train", 512, 32, 20, split=2,
         claim=_c("blk", 8, 4, 20, 1, own0=4, split=2)),
    Cell("train-blk-own1", "train", 128, 256, 9, stride=2, split=2,
         claim=_c("blk", 2, 8, 5, 2, dwo_seq=1, own0=1, split=2)),
    # F = fc + 1: the last chunk holds one frame, of which workgroup 0 owns none
    Cell("train-blk-last-chunk-1", "train", 128, 7, 33, split=2, n_active=(7, 5, 1),
         claim=_c("blk", 2, 8, 32, 2, own0=8, split=2)),
    # 8 + 7: an odd last chunk (workgroup 0 owns 3 of 7)
    Cell("train-blk-odd-last-chunk", "train", 128, 256, 15, split=2,
         claim=_c("blk", 2, 8, 8, 2, dwo_seq=1, own0=3, split=2)),
    # loop-invariant frames (stride 0, shared targets, L2, automatic split)
    Cell("train-inv-h64", "train", 64, 32, 40, stride=0, shared=True, split=0, n_frames=(40, 33, 37),
         claim=_c("inv", 1, 8, 32, 2)),
    Cell("train-inv-h256", "train", 256, 32, 40, stride=0, shared=True, split=0,
         n_frames=(40, 33, 37), claim=_c("inv", 4, 8, 32, 2)),
    Cell("train-inv-h512", "train", 512, 32, 40, stride=0, shared=True, split=0,
         n_frames=(40, 33, 37), claim=_c("inv", 8, 4, 32, 2)),
    Cell("train-inv-n85", "train", 128, 85, 40, stride=0, shared=True, split=0,
         n_frames=(40, 33, 37), claim=_c("inv", 2, 8, 32, 2)),
    Cell("train-inv-ped", "train", 128, 32, 40, stride=0, shared=True, split=0, layout="ped",
         n_frames=(40, 33, 37), claim=_c("inv", 2, 8, 32, 2)),
    Cell("train-inv-n86-general", "train", 128, 86, 40, stride=0, shared=True, split=1,
         n_frames=(40, 33, 37), claim=_c("general", 2, 8, 32, 2, dwo_seq=1)),
    # empty and one-pedestrian scenes
    Cell("train-n01-l2", "train", 64, 20, 5, claim=_c("general", 1, 8, 5, 1), **N01),
    Cell("train-n01-nll", "train", 64, 20, 5, loss="nll", claim=_c("nll", 1, 8, 5, 1), **N01),
]

CELLS = FORWARD + TRAIN

# every (TPW, NP) launch_np can select, per mode (g2k_scene.hip launch_np)
FORWARD_BUILDS = {(1, 12), (2, 12), (4, 12), (1, 4), (2, 4), (4, 4), (8, 4)}
TRAIN_BUILDS = {(1, 8), (2, 8), (4, 8), (8, 4)}
FORWARD_VARIANTS = {"general", "inv"}
TRAIN_VARIANTS = {"general", "nll", "inv", "blk"}
