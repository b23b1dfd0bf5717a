"""CPU: every cell of tests/eval_cells.py reaches the geometry it claims, read
from the library's own planning calls (host arithmetic, no HIP call):

  KS, FC, C   g2k_best_of_k_geometry (the bestk_geom that best_of_k_kernel and
              kde_nll_kernel share)
  W           g2k_head_stats_workspace_bytes / g2k_fullcov_stats_workspace_bytes
              divided by the row size (one row per workgroup); U = ceil(S F Nmax / W)
  KD          g2k_joint_eval_workspace_bytes / (S max(F, 1) 40), then min(., (K + 1) // 2)
  rows        S x the split of g2k_step_geometry

and the cells together name every branch the table was written for: KS 8, 32
(cut by the fill limit, not by K) and 64, a lane with one, two and three draws,
a second workgroup of the per-pair rows kernels; W 17 (the second thread of a
value in g2k_head_stats_rows_kernel, the second trip of g2k_fullcov_rows_
kernel), W 33 (the second trip of the former) and the cap W 256 with U > 512;
KD = 1 with K > 1 in both joint kernels, F > 64 in g2k_joint_rows_kernel; a
second and a third trip of g2k_grad_rows_kernel.  A moved constant fails here,
loudly, instead of leaving a GPU cell that runs some other path than the one it
was written for.  What cannot be read from outside (the 16 / 32 rows per trip
of the stats rows kernels, 256 rows per trip of the gradient's, the joint
kernels' 64-lane waves) is stated here once, next to the claim it supports."""
import ctypes

import numpy as np
import pytest

from multimodaltraj_2_amd import _lib
from multimodaltraj_2_amd import frame_step as fs
from multimodaltraj_2_amd.nll import best_of_k_geometry
from tests import eval_cells as ec
from tests import kde_cases as kc
from tests.bestk_ref import pair_mask

NL = len(ec.LEVELS)
HEAD_ROW = (96 + 12 * NL) * 8          # bytes of a workgroup's row, g2k_calib.hip
FULLCOV_ROW = (460 + 13 * NL) * 8      # ... g2k_fullcov.hip
BK_FILL = 2 * 256 * 1024               # g2k_bestk_geom.h kBkFill


def _dims(S, F, Nmax):
    return _lib.G2KDims(S, F, 8, 12, 16, 64, Nmax, 8, 0)


def test_cell_ids_are_unique():
    ids = [c.id for c in ec.PER_PAIR + ec.STATS + ec.JOINT + ec.TRAIN + [ec.NLL]]
    assert len(ids) == len(set(ids))


# ---------------------------------------------------------------------------
# per-pair family
# ---------------------------------------------------------------------------
def pair_geometry(c):
    g = best_of_k_geometry(c.S, c.F, c.Nmax, c.K)
    ks = g["ks"]
    lanes = [len(range(j, c.K, ks)) for j in range(ks)]
    k_alone = best_of_k_geometry(1, 1, 1, c.K)["ks"]       # 1 slot: only K and the cap stop KS
    return dict(ks=ks, fc=g["fc"], c=g["c"], draws=(min(lanes), max(lanes)), by_fill=ks < k_alone,
                row_wgs=-(-c.S * 8 // 256) if g["c"] > 1 else 0)


@pytest.mark.parametrize("cell", ec.PER_PAIR, ids=lambda c: c.id)
def test_pair_cell_reaches_its_claimed_geometry(cell):
    assert pair_geometry(cell) == cell.claim
    assert len(cell.n_active) == cell.S and max(cell.n_active) <= cell.Nmax
    assert cell.n_frames is None or (len(cell.n_frames) == cell.S and max(cell.n_frames) == cell.F)
    slots = cell.S * cell.F * cell.Nmax
    if cell.claim["by_fill"]:                              # this KS is the first to reach the fill limit
        assert slots * cell.claim["ks"] // 2 < BK_FILL <= slots * cell.claim["ks"]


def test_pair_cells_cover_the_dealings():
    by = {c.id: c for c in ec.PER_PAIR}
    assert {c.claim["ks"] for c in ec.PER_PAIR} == {8, 32, 64}
    assert by["ks8"].K % by["ks8"].claim["ks"] != 0        # K is not a multiple of KS
    c = by["ks32-fill"]
    assert c.claim["by_fill"] and best_of_k_geometry(1, 1, 1, c.K)["ks"] == 64
    assert c.claim["c"] > 1 and c.claim["row_wgs"] == 2    # a second workgroup of the rows kernels
    assert sorted(c.n_active)[-2:] == [6, 256] and 0 in c.n_active
    x = ec.pair_inputs(c)                                  # ... whose scenes (32 on) have pairs
    assert pair_mask(c.S, c.F, c.Nmax, x["n_active"], x["n_frames"], x["ped_mask"])[32:].sum() >= 4
    big = c.n_active.index(256)                            # the full scene keeps both chunks
    assert c.n_frames[big] == c.F and x["ped_mask"][big].sum() > 128
    # one, two and three draws per lane at the cap of 64 lanes
    assert {d for x in ec.PER_PAIR if x.claim["ks"] == 64 for d in x.claim["draws"]} == {1, 2, 3}
    assert all(x.n_active == (2,) for x in ec.PER_PAIR if x.claim["ks"] == 64)


def test_kde_cases_run_the_fill_cell():
    """tests/kde_cases.py holds ks32-fill's shape for both KDE entry points: KS
    32 by the fill limit, two chunks per scene, a second rows workgroup."""
    i = kc.IDS.index("ks32fill")
    _, S, F, N, K = kc.CASES[i][:5]
    c = next(c for c in ec.PER_PAIR if c.id == "ks32-fill")
    assert (S, F, N, K) == (c.S, c.F, c.Nmax, c.K) and tuple(kc.CASES[i][5]) == c.n_active
    assert best_of_k_geometry(S, F, N, K) == dict(ks=32, fc=1, c=2)
    assert 32 in {best_of_k_geometry(*x[1:5])["ks"] for x in kc.CASES}
    assert S * 8 > 256 and kc.inputs(i)["pairs"][32:].sum() >= 4       # the second workgroup's scene


def test_best_of_k_geometry_is_the_launchers():
    """By the constants of g2k_bestk_geom.h, for the shapes the header names:
    S 256 x F 20 x Nmax 32 runs KS 4, FC 2; the real-data evaluation KS 16."""
    assert best_of_k_geometry(256, 20, 32, 20) == dict(ks=4, fc=2, c=10)
    assert best_of_k_geometry(400, 1, 32, 20) == dict(ks=16, fc=1, c=1)
    assert best_of_k_geometry(3, 0, 20, 20) == dict(ks=16, fc=1, c=1)      # no frame: one workgroup
    assert best_of_k_geometry(1, 1, 1, 1) == dict(ks=1, fc=1, c=1)
    assert best_of_k_geometry(2, 40, 32, 7) == dict(ks=4, fc=2, c=20)


# ---------------------------------------------------------------------------
# stats family
# ---------------------------------------------------------------------------
def stats_geometry(c):
    lib = _lib.load()
    d = _dims(c.S, c.F, c.Nmax)
    hb = int(lib.g2k_head_stats_workspace_bytes(ctypes.byref(d), NL))
    fb = int(lib.g2k_fullcov_stats_workspace_bytes(ctypes.byref(d), NL))
    assert hb % HEAD_ROW == 0 and fb % FULLCOV_ROW == 0
    assert hb // HEAD_ROW == fb // FULLCOV_ROW              # both kernels deal the slots alike
    w = hb // HEAD_ROW
    return dict(w=w, u=-(-c.S * c.F * c.Nmax // w))


@pytest.mark.parametrize("cell", ec.STATS, ids=lambda c: c.id)
def test_stats_cell_reaches_its_claimed_geometry(cell):
    assert stats_geometry(cell) == cell.claim


def test_stats_cells_cover_the_rows_kernels_trips():
    w = {c.id: c.claim["w"] for c in ec.STATS}
    # g2k_head_stats_rows_kernel: thread (i, j) keeps slices 16 j .. 16 j + 15, a trip is 32 rows
    assert 16 < w["w17"] <= 32 < w["w33"] <= 64
    # g2k_fullcov_rows_kernel: a trip is 16 rows
    assert -(-w["w17"] // 16) == 2 and -(-w["w33"] // 16) == 3
    cap = next(c for c in ec.STATS if c.id == "cap")
    assert cap.claim["w"] == 256 and cap.claim["u"] > 512
    assert cap.claim["u"] % cap.Nmax != 0                   # a range ends inside a scene-frame
    for c in ec.STATS:                                      # random sizes with 0, one full scene
        x = ec.stats_inputs(c)
        assert 0 in x["n_active"] and 0 in x["n_frames"] and x["pairs"] >= 200
        assert (x["n_active"][0], x["n_frames"][0]) == (c.Nmax, c.F)
        # the pairs of every workgroup's range: each trip of 16 rows (and so each of 32) and the
        # last row have some, so a trip that is dropped or read wrongly changes the sums
        m = pair_mask(c.S, c.F, c.Nmax, x["n_active"], x["n_frames"], x["ped_mask"]).reshape(-1)
        W, U = c.claim["w"], c.claim["u"]
        per_row = np.array([m[r * U:(r + 1) * U].sum() for r in range(W)])
        assert per_row.sum() == x["pairs"] and per_row[-1] > 0
        assert all(per_row[r0:r0 + 16].sum() > 0 for r0 in range(0, W, 16))


# ---------------------------------------------------------------------------
# joint family
# ---------------------------------------------------------------------------
def joint_geometry(c):
    lib = _lib.load()
    d = _dims(c.S, c.F, c.Nmax)
    nb = int(lib.g2k_joint_eval_workspace_bytes(ctypes.byref(d)))
    assert nb == int(lib.g2k_fullcov_joint_eval_workspace_bytes(ctypes.byref(d)))
    assert nb % (c.S * max(c.F, 1) * 40) == 0
    kd = min(nb // (c.S * max(c.F, 1) * 40), (c.K + 1) // 2)
    waves = 1 if c.Nmax <= 64 else 4                        # joint_geom
    gl = passes = 0
    if waves == 1:                                          # joint_wave_kernel: P <= Nmax
        p = min(max(c.n_active), c.Nmax)
        gl = 16 if p <= 16 else 32 if p <= 32 else 64
        items = 2 + len(range(0, c.K, kd))                  # slice 0: targets, mean, its draws
        passes = -(-items // (64 // gl))
    # g2k_joint_rows_kernel: lane l adds frames l, l + 64, ...
    return dict(waves=waves, kd=kd, gl=gl, passes=passes, lane0_frames=len(range(0, c.F, 64)))


@pytest.mark.parametrize("cell", ec.JOINT, ids=lambda c: c.id)
def test_joint_cell_reaches_its_claimed_geometry(cell):
    assert joint_geometry(cell) == cell.claim
    assert len(cell.n_active) == cell.S and (cell.n_frames is None or len(cell.n_frames) == cell.S)


def test_joint_cells_cover_one_unit_per_scene_frame():
    for c in ec.JOINT:
        assert c.claim["kd"] == 1 and c.K > 1               # one unit makes every draw
    assert {c.claim["waves"] for c in ec.JOINT} == {1, 4}
    waves = next(c for c in ec.JOINT if c.id == "kd1-waves")
    # g2k_joint_rows_kernel: lane l adds frames l, l + 64, ...; F = 65 gives lane 0 two
    assert waves.F > 64 and waves.n_frames.count(waves.F) >= 1
    x = ec.joint_inputs(waves)                              # ... and frame 64 has members and couples
    last = pair_mask(waves.S, waves.F, waves.Nmax, x["n_active"], x["n_frames"], x["ped_mask"])[:, 64]
    assert (last.sum(axis=1) >= 2).sum() >= 3
    assert {0, 1, 2, waves.Nmax} <= set(waves.n_active) and {0, 1} <= set(waves.n_frames)
    wave = next(c for c in ec.JOINT if c.id == "kd1-wave")
    assert set(wave.n_active) == {0, 1, 2, 3, 4}
    # the production geometry the table names: S 256 x F 20
    lib = _lib.load()
    d = _dims(256, 20, 32)
    assert int(lib.g2k_joint_eval_workspace_bytes(ctypes.byref(d))) == 256 * 20 * 40


# ---------------------------------------------------------------------------
# train family
# ---------------------------------------------------------------------------
def train_geometry(c):
    g = fs.step_geometry(c.S, c.F, c.H, c.Nmax, train=True, has_h_in=True, split=c.split)
    assert g["split"] == fs.step_geometry(c.S, c.F, c.H, c.Nmax, train=True, has_h_in=False,
                                          split=c.split)["split"]
    rows = c.S * g["split"]
    trips = -(-rows // ec.ROWS_PER_TRIP)
    return dict(rows=rows, trips=trips, last=rows - (trips - 1) * ec.ROWS_PER_TRIP)


@pytest.mark.parametrize("cell", ec.TRAIN, ids=lambda c: c.id)
def test_train_cell_reaches_its_claimed_rows(cell):
    assert train_geometry(cell) == cell.claim
    lib = _lib.load()
    d = _lib.G2KDims(cell.S, cell.F, 8, 12, 16, cell.H, cell.Nmax, cell.F - 1 + 8, 1,
                     fs.step_flags(split=cell.split))
    P = int(lib.g2k_grad_size(ctypes.byref(d)))
    nws = int(lib.g2k_train_workspace_bytes(ctypes.byref(d)))
    assert nws >= cell.claim["rows"] * (P + 2) * 4 > (cell.claim["rows"] - 1) * (P + 2) * 4
    nf = ec.train_n_frames(cell)
    assert {0, 1, cell.F} <= set(nf.tolist())
    assert nf[-1] == cell.F and ec.train_mask(cell)[-1].any()      # the last trip's rows are not zero


def test_nll_cell_reaches_its_claimed_rows():
    c = ec.NLL
    lib = _lib.load()
    nb = int(lib.g2k_nll_workspace_bytes(ctypes.byref(_dims(c.S, c.F, c.Nmax))))
    rows = nb // (38 * 4)                                   # one row [3 L + 2] per scene
    trips = -(-rows // ec.ROWS_PER_TRIP)
    assert dict(rows=rows, trips=trips, last=rows - (trips - 1) * ec.ROWS_PER_TRIP) == c.claim


def test_train_cells_cover_the_later_trips():
    assert {c.claim["trips"] for c in ec.TRAIN} == {2, 3}
    assert all(0 < c.claim["last"] < 8 for c in ec.TRAIN + [ec.NLL])    # clamped loads past the last row
    assert ec.NLL.claim["trips"] == 2
