"""CPU: the Gaussian-mixture head's fused joint best-of-K and KDE-NLL
(g2k_mix_joint_eval_f32, g2k_mix_kde_nll_f32, include/g2k_mix.h;
MixtureHead.joint_eval / kde_nll; evaluate.py) — the parts that need no GPU.
The four symbols are declared, bound and exported; every validator of the two
full-covariance entry points is repeated and rejects before any GPU call; the
wrappers check their arguments; the checkers (tests/mix_eval_ref.py) reduce to
the full-covariance checkers for MixtureHead.from_fullcov's one-slot block; the
figure tuples; and, on the checkers alone, what the GPU tests rely on: the cap
on the ambiguous couple-draws of every joint run, the KDE gate (the restated
precision of THIS head's moment scheme against float64 over the GPU cases'
inputs with the checker's draws, never the kernel's output) and the share of
steps next to a clip decision."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib, mixture
from tests import fullcov_joint_ref as fj
from tests import fullcov_ref as fr
from tests import kde_cases as kc
from tests import kde_ref as kr
from tests import mix_eval_ref as me
from tests import mixture_ref as mr
from tests.bestk_ref import MASK64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 16                         # a non-NULL pointer, 16-byte aligned (never dereferenced)
_EINVAL, _EUNSUPPORTED = -1, -4
NEW = ("g2k_mix_joint_eval_workspace_bytes", "g2k_mix_joint_eval_f32",
       "g2k_mix_kde_nll_workspace_bytes", "g2k_mix_kde_nll_f32")
FLOOR = -20.0


def _dims(**kw):
    d = dict(S=2, F=20, T=8, L=12, D=16, H=128, Nmax=32, W=27, stride=1)
    d.update(kw)
    return _lib.G2KDims(**d)


def test_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "g2k_mix.h")).read(), flags=re.S)
    lib = mixture.load()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in mixture.SYMBOLS and name not in _lib.SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is mixture.SYMBOLS[name][0] and list(fn.argtypes) == mixture.SYMBOLS[name][1]
    # the full-covariance entry points' signatures (pointers there are c_void_p too)
    assert len(mixture.SYMBOLS[NEW[1]][1]) == len(_lib.SYMBOLS["g2k_fullcov_joint_eval_f32"][1])
    assert len(mixture.SYMBOLS[NEW[3]][1]) == len(_lib.SYMBOLS["g2k_fullcov_kde_nll_f32"][1])
    assert lib.g2k_abi_version() == 11 and _lib.ABI_VERSION == 11
    hdr = open(os.path.join(ROOT, "include", "g2k_mix.h")).read()
    assert "Alignment (bytes) of g2k_mix_joint_eval_f32: targets 8, sums_i 8," in hdr
    assert "Alignment (bytes) of g2k_mix_kde_nll_f32: targets 8, per_ped 16," in hdr
    assert "g2k_mix_" not in open(os.path.join(ROOT, "include", "g2k_hip.h")).read()


# ---------------------------------------------------------------------------
# the validators: those of tests/test_fullcov_joint.py and tests/test_kde_nll.py
# ---------------------------------------------------------------------------
def _joint(lib, d, K=20, radius=0.2, ws_bytes=1 << 30, fn="g2k_mix_joint_eval_f32", **over):
    a = dict(pred=P, targets=P, n_active=P, mix=P, sums_f=P, sums_i=P, ws=P)
    a.update(over)
    rc = getattr(lib, fn)(ctypes.byref(d) if d is not None else None, a["pred"], a["targets"],
                          a["n_active"], None, None, a["mix"], ctypes.c_uint64(5), K,
                          ctypes.c_float(radius), None, None, a["sums_f"], a["sums_i"], a["ws"], ws_bytes,
                          None)
    return rc, (lib.g2k_last_error() or b"")


def test_joint_entry_point_validates():
    lib = mixture.load()
    d = _dims()

    def rejects(word, dims=d, code=_EINVAL, **kw):
        rc, msg = _joint(lib, dims, **kw)
        assert rc == code and word in msg, (kw, rc, msg)

    rejects(b"dims is NULL", dims=None)
    for name in ("pred", "targets", "n_active", "mix", "sums_f", "sums_i"):
        rejects(b"NULL", **{name: None})
    for K in (0, 4097):
        rejects(b"K=%d (1..4096)" % K, K=K)
    for radius in (-0.5, float("nan"), float("inf")):
        rejects(b"radius", radius=radius)
    for Nmax in (0, 300):
        rejects(b"Nmax=%d" % Nmax, dims=_dims(Nmax=Nmax))
    rejects(b"mix_joint_eval reads pred_path_band", dims=_dims(flags=_lib.STEP_PRED_PED_MAJOR),
            code=_EUNSUPPORTED)
    assert _joint(lib, _dims(flags=_lib.STEP_PRED_PED_MAJOR))[0] == \
        _joint(lib, _dims(flags=_lib.STEP_PRED_PED_MAJOR), fn="g2k_fullcov_joint_eval_f32", mix=P)[0]
    # shared targets pass: validation reaches the workspace check, the last before a launch
    rejects(b"workspace", dims=_dims(flags=_lib.STEP_TARGETS_SHARED), ws_bytes=0)
    rejects(b"targets must be 8-byte aligned", targets=20)
    rejects(b"sums_i must be 8-byte aligned", sums_i=20)
    rejects(b"workspace must be 4-byte aligned", ws=18)
    size = lib.g2k_mix_joint_eval_workspace_bytes
    for dd in (_dims(), _dims(S=256), _dims(S=3, F=1, Nmax=256), _dims(S=1, F=0), _dims(S=0)):
        assert size(ctypes.byref(dd)) == lib.g2k_fullcov_joint_eval_workspace_bytes(ctypes.byref(dd))
    need = size(ctypes.byref(d))
    assert need == 2 * 20 * 8 * 10 * 4
    rejects(b"workspace of %d bytes needed (got %d)" % (need, need - 1), ws_bytes=need - 1)
    rejects(b"workspace", ws=None)
    assert size(ctypes.byref(_dims(S=-1))) == -1 and size(None) == -1
    # S = 0: nothing to run, validated all the same
    assert _joint(lib, _dims(S=0), ws_bytes=0)[0] == 0
    assert _joint(lib, _dims(S=0), ws=None, ws_bytes=0)[0] == 0
    rejects(b"K=0", dims=_dims(S=0), K=0)
    rejects(b"NULL", dims=_dims(S=0), mix=None)


def _kde(lib, d, **kw):
    a = dict(pred=P, targets=P, n_active=P, mix=P, K=20, log_floor=FLOOR, per_ped=P, out=P, ws=P,
             ws_bytes=2 * 20 * 32)
    assert set(kw) <= set(a), kw
    a.update(kw)
    rc = lib.g2k_mix_kde_nll_f32(ctypes.byref(d) if d is not None else None, a["pred"], a["targets"],
                                 a["n_active"], None, None, a["mix"], ctypes.c_uint64(7), a["K"],
                                 ctypes.c_float(a["log_floor"]), a["per_ped"], a["out"], a["ws"],
                                 a["ws_bytes"], None)
    return rc, (lib.g2k_last_error() or b"")


def test_kde_entry_point_validates():
    """tests/test_kde_nll.py::test_entry_points_validate for the new entry
    point: the same rejections in the same order."""
    lib = mixture.load()
    d = _dims()

    def rejects(word, dims=d, code=_EINVAL, **kw):
        rc, msg = _kde(lib, dims, **kw)
        assert rc == code and word in msg, (kw, rc, msg)

    rejects(b"dims is NULL", dims=None)
    rejects(b"mix_kde_nll reads pred_path_band", dims=_dims(flags=_lib.STEP_PRED_PED_MAJOR),
            code=_EUNSUPPORTED)
    for bad, word in ((dict(Nmax=0), b"Nmax=0"), (dict(Nmax=300), b"Nmax=300"), (dict(S=-1), b"S=-1"),
                      (dict(F=-1), b"F=-1")):
        rejects(word, dims=_dims(**bad))
    for K in (3, 0, -1, 4097):
        rejects(b"K=%d (4..4096)" % K, K=K)
    for v in (float("nan"), float("inf"), float("-inf")):
        rejects(b"log_floor=", log_floor=v)
    rejects(b"K=3 ", K=3, log_floor=float("nan"))                          # K before the floor
    rejects(b"log_floor=", log_floor=float("nan"), pred=None)               # the floor before the pointers
    for name in ("pred", "targets", "n_active", "mix", "out"):
        rejects(b"required buffer pointer is NULL", **{name: None})
    rejects(b"targets must be 8-byte aligned", targets=20)
    rejects(b"per_ped must be 16-byte aligned", per_ped=24)
    rejects(b"per_ped", per_ped=24, ws=None)                                # alignment before the workspace
    rejects(b"workspace", dims=_dims(flags=_lib.STEP_TARGETS_SHARED), ws_bytes=0)   # the flag passes
    need = 2 * 20 * 32
    size = lib.g2k_mix_kde_nll_workspace_bytes
    for S, F in [(2, 20), (1, 1), (3, 0), (0, 20), (256, 20), (7, 37)]:
        assert size(ctypes.byref(_dims(S=S, F=F))) == S * max(F, 1) * 32
    assert size(None) == -1 and size(ctypes.byref(_dims(S=-1))) == -1
    rejects(b"workspace of %d bytes needed (got %d)" % (need, need), ws=None)
    rejects(b"workspace of %d bytes needed (got %d)" % (need, need - 4), ws_bytes=need - 4)
    # nothing to do: S = 0 and F = 0 return 0 and launch nothing; still validated
    assert _kde(lib, _dims(S=0), ws=None, ws_bytes=0)[0] == 0
    assert _kde(lib, _dims(F=0), ws_bytes=2 * 32)[0] == 0
    assert _kde(lib, _dims(S=0, F=0), ws=None, ws_bytes=0, per_ped=None)[0] == 0
    rejects(b"K=3 ", dims=_dims(S=0), K=3)
    rejects(b"required buffer", dims=_dims(F=0), mix=None)
    rejects(b"workspace of 64 bytes", dims=_dims(F=0), ws_bytes=60)


def test_wrappers_check_arguments():
    mx = mixture.MixtureHead(components=3, device="cpu")
    pred = torch.zeros((1, 1, 24, 4))
    tg = torch.zeros((1, 1, 4, 12, 2))
    na = torch.ones(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):                    # CPU tensors: no launch
        mx.joint_eval(pred, tg, na, 2, 0.1)
    for k in (0, 4097):
        with pytest.raises(ValueError, match="k = "):
            mx.joint_eval(pred, tg, na, k, 0.1)
    for r in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError, match="radius"):
            mx.joint_eval(pred, tg, na, 2, r)
    for k in (3, 4097):
        with pytest.raises(ValueError, match="4..4096"):
            mx.kde_nll(pred, tg, na, k)
    with pytest.raises(ValueError, match="log_floor"):
        mx.kde_nll(pred, tg, na, 4, log_floor=float("-inf"))
    for call in (lambda *a, **kw: mx.joint_eval(*a, 2, 0.1, **kw), lambda *a, **kw: mx.kde_nll(*a, 4, **kw)):
        with pytest.raises(ValueError, match="pred must be"):
            call(torch.zeros((1, 1, 23, 4)), tg, na)
        with pytest.raises(ValueError, match="targets must be"):
            call(pred, torch.zeros((1, 1, 5, 12, 2)), na)
        with pytest.raises(ValueError, match="targets must be"):   # shared targets: one frame
            call(torch.zeros((1, 2, 24, 4)), torch.zeros((1, 2, 4, 12, 2)), na, targets_shared=True)
        with pytest.raises(ValueError, match="n_active"):
            call(pred, tg, torch.ones(2, dtype=torch.int32))
        with pytest.raises(ValueError, match="ped_mask"):
            call(pred, tg, na, ped_mask=torch.ones((1, 5), dtype=torch.uint8))
        with pytest.raises(ValueError, match="n_frames"):
            call(pred, tg, na, n_frames=torch.ones(2, dtype=torch.int32))
        with pytest.raises(TypeError, match="n_active"):
            call(pred, tg, torch.ones(1, dtype=torch.int64))
    mx.params = torch.zeros((8, 607))
    with pytest.raises(ValueError, match="params"):
        mx.joint_eval(pred, tg, na, 2, 0.1)
    with pytest.raises(ValueError, match="params"):
        mx.kde_nll(pred, tg, na, 4)


def test_figure_tuples():
    from multimodaltraj_2_amd import evaluate
    assert evaluate.MIX_JOINT_FIGURES == ("mix_jade", "mix_jfde", "mix_collision_rate",
                                          "mix_collision_rate_best")
    assert evaluate.MIX_KDE_FIGURES == ("mix_kde_nll", "mix_kde_nll_final", "mix_kde_clipped")
    assert evaluate.MIX_FIGURES == ("mix_min_ade", "mix_min_fde", "mix_nll", "mix_components",
                                    "mix_weight_max", "mix_loglik_gain")
    old = (evaluate.FIGURES + evaluate.JOINT_FIGURES + evaluate.CALIB_FIGURES + evaluate.FULLCOV_FIGURES
           + evaluate.FULLCOV_JOINT_FIGURES + evaluate.KDE_FIGURES + evaluate.FULLCOV_KDE_FIGURES
           + evaluate.MIX_FIGURES + ("scenes", "pairs", "K"))
    new = evaluate.MIX_JOINT_FIGURES + evaluate.MIX_KDE_FIGURES
    assert len(set(new)) == 7 and not set(new) & set(old)


# ---------------------------------------------------------------------------
# the checkers alone
# ---------------------------------------------------------------------------
def _from_fullcov(chol):
    from multimodaltraj_2_amd.fullcov import FullCovHead
    fc = FullCovHead(device="cpu")
    fc.chol = torch.from_numpy(np.asarray(chol, np.float32))
    return mixture.MixtureHead.from_fullcov(fc).params.numpy()


def test_checkers_reduce_to_the_full_covariance_checkers():
    """MixtureHead.from_fullcov's block (one slot, b = 0): the joint checker is
    tests/fullcov_joint_ref.py's (floats to 1e-12, integers exactly) and the
    KDE checker tests/kde_ref.py's on tests/fullcov_ref.py's draws; the NaN
    test block of the same factor gives the same."""
    c = kc.inputs(kc.IDS.index("k5"))
    chol = np.tril(c["chol"])
    block = _from_fullcov(chol)
    assert block[0, 0] == 1 and np.all(block[1:] == 0) and np.all(block[0, 1:mr.OFF_L] == 0)
    rng = np.random.default_rng(5)
    S, F, N, K, radius = 3, 2, 20, 4, 0.3
    pred = rng.standard_normal((S, F, 24, N)).astype(np.float32)
    tg = (pred.reshape(S, F, 2, 12, N).transpose(0, 1, 4, 3, 2)
          + 0.3 * rng.standard_normal((S, F, N, 12, 2))).astype(np.float32)
    nact, nfr = np.array([N, 7, 0], np.int32), np.array([2, 1, 2], np.int32)
    pm = (rng.random((S, N)) > 0.2).astype(np.uint8)
    A = fj.joint_eval_ref(pred, tg, nact, chol, 77, K, radius, nfr, pm)
    for blk in (block, me.one_slot_block(chol)):
        B = me.joint_eval_ref(pred, tg, nact, blk, 77, K, radius, nfr, pm)
        assert sorted(A) == sorted(B) and A["col_k"].sum() > 0
        for key in A:
            if A[key].dtype.kind == "f":
                np.testing.assert_allclose(B[key], A[key], rtol=0, atol=1e-12, err_msg=key)
            else:
                np.testing.assert_array_equal(B[key], A[key], err_msg=key)
    # KDE, on case k5's inputs (NaN columns past n_active)
    with np.errstate(invalid="ignore"):
        dm = np.stack([mr.sample(c["pred"], block, (c["seed"] + k) & MASK64)[0] for k in range(c["K"])])
        df = np.stack([fr.sample(c["pred"], chol, (c["seed"] + k) & MASK64) for k in range(c["K"])])
    m = c["pairs"]
    Rm = me.kde_nll_ref(dm.astype(np.float32), c["targets"], m, FLOOR)
    Rf = kr.kde_nll_ref(df.astype(np.float32), c["targets"], m, FLOOR)
    np.testing.assert_allclose(Rm["per_ped"], Rf["per_ped"], rtol=0, atol=1e-9)
    np.testing.assert_array_equal(Rm["clip"][m], Rf["clip"][m])
    assert m.sum() > 20 and not Rm["near_singular"][m].any()


def test_test_blocks():
    b = me.mix_block(0.3, 100)
    assert (b[:, 0] != 0).tolist() == [m in me.SLOTS3 for m in range(8)]
    assert np.all((b[list(me.SLOTS3), 0] >= 0.2) & (b[list(me.SLOTS3), 0] <= 1.0))
    assert np.isnan(b[1]).sum() == mr.PITCH - 1 and np.isnan(b[0, 1:8]).all()
    Lm = b[2, mr.OFF_L:].reshape(24, 24)
    assert np.isnan(Lm[np.triu_indices(24, 1)]).all() and np.isfinite(Lm[np.tril_indices(24)]).all()
    np.testing.assert_array_equal(Lm[np.tril_indices(24)],
                                  fj.walk_factor(0.3, np.random.default_rng(1102))[np.tril_indices(24)])
    assert (me.mix_block(0.3, 101, me.ALL8)[:, 0] != 0).all()
    # a finite checker result: the NaN were never read
    x, comp = mr.sample(np.zeros((1, 1, 24, 64), np.float32), b, 3)
    assert np.isfinite(x).all() and set(np.unique(comp)) <= set(me.SLOTS3) and len(np.unique(comp)) == 3
    for which, scale in me.KDE_SCALES.items():
        kb = me.kde_block(0, which)
        assert np.abs(kb[list(me.SLOTS3), mr.OFF_B:mr.OFF_L]).max() > 2 * scale


def test_joint_cap_on_the_checker():
    """Every joint run of tests/test_mix_eval_gpu.py, on the checker alone: the
    couple-draws within 1e-4 of the radius are at most 1e-3 of all couple-draws
    and at most 1 % of the collisions, so the bracket cannot hide a failure."""
    from tests.test_fullcov_joint_gpu import assert_cap
    runs, ids = me.joint_runs()
    assert len(runs) == 13 and runs[-1][2] == me.ALL8
    for (i, radius, slots), name in zip(runs, ids):
        R, c = me.joint_reference(i, radius, slots), me.joint_inputs(i, slots)
        assert_cap(int(R["amb_k"].sum()), c["K"] * int(R["per_frame_i"][..., 1].sum()),
                   int(R["col_k"].sum()), f"checker, run {name}")
    # the 8-slot run draws from every component in one scene-frame
    c = me.joint_inputs(runs[-1][0], me.ALL8)
    comp = mr.components(c["pred"].shape, c["mix"], c["seed"])
    assert len(np.unique(comp[0, 0, :64])) == 8


def test_kde_gate_measurement():
    """The GPU gate: worst |restated precision - float64| of a term and of a
    pair's kde_nll over the eight tests/kde_cases.py inputs with the checker's
    mixture draws, near and far blocks; mix_eval_ref.GATE is 8 x the recorded
    worst, and the record (to 10 %) is not below what is measured here.  The
    other heads' scheme (kde_ref's restatement: plain sums of x - mu) and the
    same sums centred on the pair's draw 0 (that restatement with draw 0 as the
    centre) are printed beside it: the candidates this head's scheme was chosen
    from."""
    worst = {w: [0.0, 0.0, 0.0, 0.0] for w in me.KDE_SCALES}
    for which in me.KDE_SCALES:
        for i, name in enumerate(kc.IDS):
            c = kc.inputs(i)
            m = c["pairs"]
            draws = me.kde_draws(i, which)
            A = me.kde_nll_ref(draws, c["targets"], m, FLOOR)
            B = me.kde_nll_ref(draws, c["targets"], m, FLOOR, pred=c["pred"], restated=True)
            with np.errstate(all="ignore"):
                C = kr.kde_nll_ref(draws, c["targets"], m, FLOOR, pred=c["pred"], restated=True)
                D = kr.kde_nll_ref(draws, c["targets"], m, FLOOR, pred=draws[0], restated=True)
            assert np.isfinite(A["per_ped"]).all() and np.isfinite(B["per_ped"]).all()
            dt = float(np.abs(A["term"][m] - B["term"][m]).max())
            dp = float(np.abs(A["per_ped"][..., :2] - B["per_ped"][..., :2]).max())
            do = float(np.abs(A["term"][m] - C["term"][m]).max())
            d0 = float(np.abs(A["term"][m] - D["term"][m]).max())
            print(f"{which} block, case {name}: {int(m.sum())} pairs, worst |restated - float64| term "
                  f"{dt:.3g}, pair {dp:.3g}; with plain sums of x - mu: term {do:.3g}, of x - draw 0: term "
                  f"{d0:.3g}")
            w = worst[which]
            w[0], w[1], w[2], w[3] = max(w[0], dt), max(w[1], dp), max(w[2], do), max(w[3], d0)
    for which, w in worst.items():
        print(f"{which} block: worst term {w[0]:.3g}, worst pair {w[1]:.3g} (plain sums of x - mu: term {w[2]:.3g}; "
              f"of x - draw 0: term {w[3]:.3g})")
    print(f"recorded {me.MEASURED_WORST:.3g}, gate {me.GATE:.3g}")
    assert me.GATE == 8 * me.MEASURED_WORST
    # 10 %: numpy's fp32 exp / log differ by an ulp between CPU dispatch paths
    assert max(max(w[:2]) for w in worst.values()) <= 1.1 * me.MEASURED_WORST


def test_kde_cases_stay_off_the_clip_decisions():
    """Steps whose float64 logp lies within the gate of the floor, or whose
    det H is next to 0 (mix_eval_ref.NEAR_SINGULAR), are left out of the GPU
    tests' exact clip counts: at most 1 % of a case's steps, both blocks."""
    for which in me.KDE_SCALES:
        for i, name in enumerate(kc.IDS):
            c = kc.inputs(i)
            m = c["pairs"]
            A = me.kde_nll_ref(me.kde_draws(i, which), c["targets"], m, FLOOR)
            near = (np.abs(A["logp"][m] - FLOOR) <= me.GATE) | A["near_singular"][m]
            print(f"{which} block, case {name}: {near.sum()} of {near.size} steps within the gate of "
                  f"the floor or next to det H = 0, clipped share {A['clip'][m].mean():.4f}")
            assert near.mean() <= 0.01
            assert not A["clip"][m].all()
