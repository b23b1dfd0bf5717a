"""CPU: the fixed-frame forward build (g2k_scene_kernel<..., FX = 20>) is
chosen exactly where include/g2k_step_fixed.h says — forward, the co-resident
geometry, stride 1, one workgroup per scene, F = 20, H < 512 — and nowhere
else; the workgroups a CU holds follow from the reported LDS; and
g2k_step_geometry's claimed fields do not move (g2k_step_fixed_geometry: host
arithmetic, no HIP call)."""
import pytest

from multimodaltraj_2_amd import frame_step as fs
from tests import step_cells as sc
from tests import step_fixed_cases as cases
from tests.test_step_cells import KEYS, geometry

CU_LDS = 160 * 1024


def fixed(F=20, H=128, Nmax=32, stride=1, **kw):
    kw.setdefault("coresident", True)
    return fs.step_fixed_geometry(3, F, H, Nmax, stride, **kw)


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("Nmax", [1, 16, 17, 32, 64])
@pytest.mark.parametrize("layout", ["band", "ped"])
def test_fixed_build_is_chosen(H, Nmax, layout):
    g = fixed(H=H, Nmax=Nmax, pred_layout=layout)
    assert g["frames"] == 20
    geo = fs.step_geometry(3, 20, H, Nmax, coresident=True, pred_layout=layout)
    assert (geo["variant"], geo["np"], geo["fc"], geo["chunks"], geo["split"]) == ("general", 4, 20, 1, 1)
    assert g["lds_bytes"] == geo["lds_bytes"] == fs.step_lds_bytes(3, 20, H, Nmax, 27, 1, True)


def test_fixed_build_with_shared_targets():
    """One target set for every frame at stride 1 is still the general variant."""
    assert fixed(targets_shared=True)["frames"] == 20


@pytest.mark.parametrize("kw", [
    dict(F=19), dict(F=21), dict(stride=0), dict(stride=2), dict(split=2), dict(H=512),
    dict(train=True, coresident=False), dict(coresident=False),
    dict(stride=0, targets_shared=True),          # loop-invariant frames
    dict(Nmax=256),                               # the LDS does not fit twice: 12 producers
], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_fixed_build_is_not_chosen(kw):
    g = fixed(**kw)
    assert g["frames"] == 0
    assert g["workgroups_per_cu"] in (1, 2)


def test_other_builds_residency():
    """The other 8-wave forward builds are sized for two workgroups per CU;
    H = 512, 12 producers and train mode run one."""
    assert fixed(F=19)["workgroups_per_cu"] == 2
    assert fixed(stride=2)["workgroups_per_cu"] == 2
    assert fixed(H=512)["workgroups_per_cu"] == 1
    assert fixed(coresident=False)["workgroups_per_cu"] == 1
    assert fixed(Nmax=256)["workgroups_per_cu"] == 1
    assert fixed(train=True, coresident=False)["workgroups_per_cu"] == 1


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("Nmax", [1, 16, 17, 32, 40, 41, 64, 94, 95])
def test_workgroups_per_cu_is_how_often_the_lds_fits(H, Nmax):
    """Capped at 3 (24 waves of <= 80 VGPRs); at 2 for the H 256 build, which
    needs 90 VGPRs and would spill at 80 (csrc/g2k_scene.hip scene_waves_per_eu)."""
    g = fixed(H=H, Nmax=Nmax)
    if g["frames"] == 0:                          # (wide scenes: the LDS no longer fits twice)
        assert fs.step_geometry(3, 20, H, Nmax, coresident=True)["np"] == 12
        return
    assert g["workgroups_per_cu"] == min(CU_LDS // g["lds_bytes"], 3 if H < 256 else 2)
    assert g["workgroups_per_cu"] == fs.step_workgroups_per_cu(3, 20, H, Nmax, 27, 1, True)
    assert fs.step_coresidency(3, 20, H, Nmax, 27, 1, True) == 2


def test_workgroups_per_cu_at_the_benchmark_shapes():
    """Nmax 32 (eth_hotel_synth): the position window shares the As ring's
    space — 12,948 floats, three per CU.  Nmax 64 (kfold4, relational): 13,788
    floats fit twice, not three times (3 x 55,152 B is 1,616 B over)."""
    g = fixed(Nmax=32)
    assert g == dict(frames=20, workgroups_per_cu=3, lds_bytes=12948 * 4)
    assert 3 * g["lds_bytes"] <= CU_LDS
    g = fixed(Nmax=64)
    assert g["frames"] == 20 and g["workgroups_per_cu"] == CU_LDS // g["lds_bytes"] == 2


def test_window_never_outgrows_the_ring():
    """The aliased window (27 rows of 2 Nmax floats) fits the ring (20 slots of
    256) up to Nmax 94; wider scenes of the fixed build (95 is one) keep a
    window of their own: the LDS grows by the window there, and by less than
    one window anywhere below."""
    def floats(n):
        return fixed(Nmax=n)["lds_bytes"] // 4
    narrow = [floats(n) for n in (92, 93, 94)]
    assert fixed(Nmax=94)["frames"] == 20
    assert fixed(Nmax=95)["frames"] == 20
    assert floats(95) - floats(94) >= 27 * 2 * 95
    assert max(narrow) - min(narrow) < 27 * 2 * 92
    assert 27 * 2 * 94 <= cases.RING < 27 * 2 * 95 and cases.N_ALIAS == 94
    # past the step the window is counted with the rest: one more pedestrian
    # costs the window's two columns again
    assert floats(96) - floats(95) >= 27 * 2


N_LAST = cases.N_LAST                 # found by scanning (tests/step_fixed_cases.py fixed_range)


@pytest.mark.parametrize("H", [64, 128, 256])
def test_fixed_build_serves_one_range_of_nmax(H):
    """The fixed build serves every Nmax from 1 to N_last = 104 and none above,
    at every H it has: scene_producers chooses 4 producers while the general
    layout (a window of its own, H not in it) fits kCoresidentLds = 20480
    floats — 12108 + 80 N + rup4(2 N) + rup4(ceil(N / 4)) is 20456 at N 104 and
    20538 at 105.  So 95..104 run the fixed build un-aliased; above, the 12
    producers of a lone launch."""
    taken = [n for n in range(1, 257) if fixed(H=H, Nmax=n)["frames"] == 20]
    last = max(taken)
    assert taken == list(range(1, last + 1)) == cases.fixed_range(H)
    assert last == N_LAST == 104
    assert last >= 95
    for n in range(last + 1, 257):
        assert fs.step_geometry(3, 20, H, n, coresident=True)["np"] == 12, n
    for n in (95, last):                          # the un-aliased layout is the general one
        assert fixed(H=H, Nmax=n)["lds_bytes"] == fs.step_geometry(3, 20, H, n, coresident=True)["lds_bytes"]
    assert fixed(H=H, Nmax=last)["lds_bytes"] == 20456 * 4 <= fs.CORESIDENT_LDS
    # the first Nmax past it: the general layout no longer fits twice (12
    # producers change only the per-producer metric rows, 8 floats each)
    assert fs.step_geometry(3, 20, H, last + 1, coresident=True)["lds_bytes"] == (20538 + 8 * 8) * 4


def test_case_table_covers_what_it_is_for():
    """Every Nmax of the table at H 128, the three TPW builds at 94, 95 and
    N_last, both layouts and both n_frames sets everywhere; per case n_active
    (0, 1, inside a tile, Nmax) and two masked pedestrians in the widest scene,
    one in its first and one in its last tile."""
    out = {(c.H, c.Nmax, c.layout, c.frames_id) for c in cases.OUTPUT_CASES}
    want = [(128, n) for n in (33, 48, 64, 93)] + [(H, n) for H in (64, 128, 256) for n in (94, 95, N_LAST)]
    assert out == {(H, n, lay, fid) for H, n in want for lay in ("band", "ped") for fid in cases.N_FRAMES}
    assert len(cases.OUTPUT_CASES) == len(out) and len({c.id for c in cases.CASES}) == len(cases.CASES)
    assert ({(c.Nmax, c.layout) for c in cases.SHARED_CASES}
            == {(n, lay) for n in (32, 94, 95) for lay in ("band", "ped")})
    assert {c.Nmax for c in cases.LONG_POS_CASES} == {32, 94}
    assert all(c.targets_shared and c.H == 128 for c in cases.SHARED_CASES)
    assert all(c.extra_rows == 3 and c.W == 30 and c.H == 128 for c in cases.LONG_POS_CASES)
    assert sorted(cases.N_FRAMES.values(), key=str) == [(1, 0, 20, 13), None]
    for c in cases.CASES:
        n0, n1, mid, full = c.n_active
        assert (n0, n1, full) == (0, 1, c.Nmax) and len(c.n_active) == cases.S == 4
        assert 1 < mid < c.Nmax and (mid - 1) % 16 not in (0, 15), c.id     # its last column
        assert mid % 16 != 0 and (mid + 15) // 16 >= 2                      # (inside a tile, not the first)
        (s0, first), (s1, last) = c.masked
        assert s0 == s1 == 3 and first < 16 and last // 16 == (c.Nmax - 1) // 16 and first != last
        assert sorted(c.frames) == [0, 1, 13, 20] or c.frames == (20,) * 4
        assert c.frames[3] in (13, 20)            # the masked, widest scene runs


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.id)
def test_cases_keep_their_claims(case):
    """A case claims what g2k_step_fixed_geometry reports of its launch."""
    g = cases.fixed_geometry(case)
    assert g["frames"] == 20
    assert cases.fixed_geometry(case, coresident=False)["frames"] == 0
    assert case.tiles == (case.Nmax + 15) // 16
    assert g["workgroups_per_cu"] == case.wgs_per_cu == min(CU_LDS // g["lds_bytes"],
                                                             3 if case.H < 256 else 2)
    # aliased: the layout without the window's 54 Nmax floats; own window: with them
    # (scene_layout_fc: 12108 floats that do not depend on Nmax, Wi, Wo, the
    # vislet rows, the mask row)
    def rup4(x):
        return (x + 3) // 4 * 4
    n = case.Nmax
    rest = 12108 + 16 * n + 8 * n + rup4(2 * n) + rup4((n + 3) // 4)
    assert case.aliased == (n <= 94)
    assert g["lds_bytes"] == (rest + (0 if case.aliased else 27 * 2 * n)) * 4
    assert g["lds_bytes"] == fs.step_geometry(cases.S, 20, case.H, n, coresident=True,
                                              pred_layout=case.layout)["lds_bytes"]
    if case.extra_rows == 0:
        assert g == fixed(H=case.H, Nmax=case.Nmax, pred_layout=case.layout,
                          targets_shared=case.targets_shared)


def test_aliased_column_is_consistent_across_the_step():
    """94 -> 95: the table's last aliased and first own-window cases differ in
    LDS by one whole window and more."""
    for H in (64, 128, 256):
        a, = {cases.fixed_geometry(c)["lds_bytes"] for c in cases.OUTPUT_CASES if (c.H, c.Nmax) == (H, 94)}
        b, = {cases.fixed_geometry(c)["lds_bytes"] for c in cases.OUTPUT_CASES if (c.H, c.Nmax) == (H, 95)}
        assert all(c.aliased for c in cases.CASES if c.Nmax == 94)
        assert not any(c.aliased for c in cases.CASES if c.Nmax >= 95)
        assert b - a >= 27 * 2 * 95 * 4


@pytest.mark.parametrize("case", cases.SHARED_CASES + cases.LONG_POS_CASES, ids=lambda c: c.id)
def test_shared_and_long_pos_cases_take_their_plain_twins_build(case):
    """One target set for every frame, or rows of pos past the window, change
    neither the build nor the LDS."""
    twin = cases.plain_twin(case)
    assert (twin.targets_shared, twin.extra_rows, twin.W) == (False, 0, 27)
    assert cases.fixed_geometry(case) == cases.fixed_geometry(twin)
    assert cases.fixed_geometry(case)["frames"] == 20


@pytest.mark.parametrize("cell", [c for c in sc.FORWARD if c.id.endswith("-coresident")],
                         ids=lambda c: c.id)
def test_coresident_cells_keep_their_claims(cell):
    assert len([c for c in sc.FORWARD if c.id.endswith("-coresident")]) == 4
    g = geometry(cell)
    assert {k: g[k] for k in KEYS} == cell.claim
    f = fs.step_fixed_geometry(cell.S, cell.F, cell.H, cell.Nmax, cell.stride, coresident=True,
                               split=cell.split, cus=sc.CUS)
    assert f["frames"] == (20 if cell.H < 512 else 0)
    assert f["lds_bytes"] == g["lds_bytes"]


def test_rejects_what_step_geometry_rejects():
    from multimodaltraj_2_amd import _lib
    with pytest.raises(_lib.G2KError):
        fs.step_fixed_geometry(3, 20, 100, 32, coresident=True)       # H not a build's
    with pytest.raises(_lib.G2KError):
        fs.step_fixed_geometry(3, 20, 128, 32, cus=0, coresident=True)
