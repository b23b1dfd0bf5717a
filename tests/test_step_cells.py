"""CPU: every cell of tests/step_cells.py reaches the scene-kernel build and
LDS layout it claims (g2k_step_geometry: the launcher's own arithmetic, no HIP
call), and the cells together cover the dispatch: every (TPW, NP) build
launch_np can select in either mode, every kernel variant, both pred layouts,
and the chunk / ownership sizes at which the kernel takes another path.  A
moved threshold fails here, loudly, instead of leaving a GPU cell that runs
some other build than the one it was written for."""
import pytest

from multimodaltraj_2_amd import frame_step as fs
from tests import step_cells as sc

KEYS = ("variant", "tpw", "np", "fc", "chunks", "dwo_seq", "own0", "split")


def geometry(c, cus=sc.CUS):
    return fs.step_geometry(c.S, c.F, c.H, c.Nmax, c.stride, train=c.entry != "fwd",
                            has_h_in=c.entry != "grad", cus=cus, pred_layout=c.layout,
                            targets_shared=c.shared, loss=c.loss, split=c.split,
                            coresident=c.coresident)


def test_cell_ids_are_unique():
    ids = [c.id for c in sc.CELLS]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("cell", sc.CELLS, ids=lambda c: c.id)
def test_cell_reaches_its_claimed_geometry(cell):
    g = geometry(cell)
    assert {k: g[k] for k in KEYS} == cell.claim
    assert g["ped_major"] == (cell.layout == "ped")
    assert 0 < g["lds_bytes"] <= 160 * 1024
    # the scenes the cell runs: one with every frame (the chunk claim runs), one at Nmax
    assert len(cell.frames) == cell.S and max(cell.frames) == cell.F
    assert max(cell.scenes) == cell.Nmax and all(0 <= f <= cell.F for f in cell.frames)
    assert g["chunks"] == -(-cell.F // g["fc"])


def _claims(cells):
    return [c.claim for c in cells]


def test_every_selectable_build_is_claimed():
    fwd = {(c["tpw"], c["np"]) for c in _claims(sc.FORWARD)}
    trn = {(c["tpw"], c["np"]) for c in _claims(sc.TRAIN)}
    assert fwd == sc.FORWARD_BUILDS, sc.FORWARD_BUILDS ^ fwd
    assert trn == sc.TRAIN_BUILDS, sc.TRAIN_BUILDS ^ trn
    assert {c["variant"] for c in _claims(sc.FORWARD)} == sc.FORWARD_VARIANTS
    assert {c["variant"] for c in _claims(sc.TRAIN)} == sc.TRAIN_VARIANTS
    # every variant at the 4-producer H = 512 build and below it, in both modes
    for cells, variants in ((sc.FORWARD, sc.FORWARD_VARIANTS), (sc.TRAIN, sc.TRAIN_VARIANTS)):
        for v in variants:
            tpws = {c.claim["tpw"] for c in cells if c.claim["variant"] == v}
            assert 8 in tpws and tpws - {8}, (v, tpws)
    # both pred layouts through every variant of either mode
    for layout in ("band", "ped"):
        assert {(c.entry, c.claim["variant"]) for c in sc.CELLS if c.layout == layout} >= (
            {("fwd", v) for v in sc.FORWARD_VARIANTS} | {("train", v) for v in sc.TRAIN_VARIANTS})
    # INV at every H, in both modes; the no-h_in entry point once per loss
    for cells in (sc.FORWARD, sc.TRAIN):
        assert {c.H for c in cells if c.claim["variant"] == "inv"} == {64, 128, 256, 512}
    assert {c.loss for c in sc.CELLS if c.entry == "grad"} == {"l2", "nll"}


def test_chunk_and_ownership_sizes_are_claimed():
    fcs = {c.claim["fc"] for c in sc.CELLS}
    assert {1, 2, 3} <= fcs
    # a halved fc (below min(F, 32)) with a partial last chunk, in both modes
    for cells in (sc.FORWARD, sc.TRAIN):
        assert any(c.claim["fc"] < min(c.F, 32) and c.F % c.claim["fc"] for c in cells)
    own = {(c.claim["own0"], c.claim["np"]) for c in sc.TRAIN if c.claim["variant"] == "blk"}
    assert {(1, 8), (4, 4), (8, 8)} <= own
    # NLL with dWo^T in frame order at NP 8 and at NP 4; the widest INV and the first width off it
    assert {c.claim["np"] for c in sc.TRAIN
            if c.claim["variant"] == "nll" and c.claim["dwo_seq"]} == {8, 4}
    for entry in ("fwd", "train"):
        assert any(c.Nmax == 85 and c.claim["variant"] == "inv" for c in sc.CELLS if c.entry == entry)
        assert any(c.Nmax == 86 and c.shared and c.stride == 0 and c.claim["variant"] == "general"
                   for c in sc.CELLS if c.entry == entry)
    # BLK: a last chunk of one frame (workgroup 0 owns none of it) and an odd last chunk
    blk = [c for c in sc.TRAIN if c.claim["variant"] == "blk"]
    assert any(c.F == c.claim["fc"] + 1 for c in blk)
    assert any(c.claim["chunks"] > 1 and (c.F % c.claim["fc"]) % 2 == 1 and c.F % c.claim["fc"] > 1
               for c in blk)
    # BLK: a scene whose second workgroup (no chain: idle recurrence waves) owns NP + 1 ..
    # NP + 3 frames of the last chunk, so 1..3 of its four recurrence waves take a frame
    def second_owns(c, nf):
        cnt = nf - (nf - 1) // c.claim["fc"] * c.claim["fc"]
        return cnt - min(c.claim["own0"], cnt // 2)
    assert any(c.claim["np"] < second_owns(c, nf) < c.claim["np"] + 4 for c in blk for nf in c.frames)
    # train mode off strides 0 and 1, overlapping and disjoint windows
    assert {2, 3, 9} <= {c.stride for c in sc.TRAIN}
    # empty and one-pedestrian scenes through every entry point's loss
    assert {(c.entry, c.loss) for c in sc.CELLS if 0 in c.scenes and 1 in c.scenes} == {
        ("fwd", "l2"), ("train", "l2"), ("train", "nll")}


def test_automatic_split_of_the_cells_is_the_mi355x_one():
    """The cells with an automatic split claim the answer for 256 CUs; a
    device with fewer (80) would split the 3-scene launches less."""
    for c in sc.CELLS:
        if c.split == 0 and c.claim["variant"] == "inv":
            assert geometry(c, cus=80)["split"] == 1          # loop-invariant: always one workgroup
    c = next(c for c in sc.CELLS if c.id == "fwd-inv-n86-general")
    assert geometry(c, cus=3)["split"] == 1 and geometry(c, cus=6)["split"] == 2
