"""CPU: the fixed-frame forward build (g2k_scene_kernel<..., FX = 20>) is
chosen exactly where include/g2k_step_fixed.h says — forward, the co-resident
geometry, stride 1, one workgroup per scene, F = 20, H < 512 — and nowhere
else; the workgroups a CU holds follow from the reported LDS; and
g2k_step_geometry's claimed fields do not move (g2k_step_fixed_geometry: host
arithmetic, no HIP call)."""
import pytest

from multimodaltraj_2_amd import frame_step as fs
from tests import step_cells as sc
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
    256) up to Nmax 94; wider scenes keep a window of their own, if they reach
    the fixed build at all: the LDS grows by the window there."""
    def floats(n):
        return fixed(Nmax=n)["lds_bytes"] // 4
    narrow = [floats(n) for n in (92, 93, 94)]
    assert fixed(Nmax=94)["frames"] == 20
    if fixed(Nmax=95)["frames"] == 20:
        assert floats(95) - floats(94) >= 27 * 2 * 95
    assert max(narrow) - min(narrow) < 27 * 2 * 92


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
