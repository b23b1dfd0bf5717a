"""CPU: the scene-coupled head (include/g2k_coupled.h,
multimodaltraj_2_amd/coupled.py, csrc/g2k_coupled.hip) — the header, the
module's binding table and the library's exports agree; every validator rejects
bad arguments before touching the GPU, in the order the header states; and the
checker tests/coupled_ref.py alone: against plain loops, the whitening identity
against a dense (24 P x 24 P) Gaussian density, the fit recovering a known law
(and clipping an indefinite B), and the reason the head exists — targets whose
residuals share 80 % of their variance within a scene-frame are calibrated
under the coupled head's joint draws and not under those of a full-covariance
head with the same marginals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib, coupled, couples, kin, mixture, modes, ranks, scores
from multimodaltraj_2_amd import build as g2k_build
from tests import coupled_cases as cx
from tests import coupled_ref as cr
from tests import couples_cases as cc
from tests import couples_ref as cpr
from tests import fullcov_ref as fr
from tests import test_couple_scores as tcs
from tests.bestk_ref import BOUNDARY_SEEDS, draw_seed
from tests.test_couple_scores import DEV_FIN, DEV_MATCHED, DEV_MIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2k_coupled.h")
P = 0x10000                    # a non-NULL pointer, 64-byte aligned (never dereferenced)
OK, EINVAL, EUNSUPPORTED = 0, -1, -4
DIM = 24


def _declarations():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(g2k_[a-z0-9_]+)\s*\(([^)]*)\)", src)}


def test_header_binding_and_exports_agree():
    decl = _declarations()
    assert sorted(decl) == sorted(coupled.SYMBOLS)
    for name, args in decl.items():
        assert len(args.split(",")) == len(coupled.SYMBOLS[name][1]), name
    # by symbol, after ABI 11: in no other header or table
    for table in (_lib.SYMBOLS, mixture.SYMBOLS, scores.SYMBOLS, modes.SYMBOLS, ranks.SYMBOLS, kin.SYMBOLS,
                  couples.SYMBOLS):
        assert not set(decl) & set(table)
    for other in ("g2k_hip.h", "g2k_mix.h", "g2k_scores.h", "g2k_modes.h", "g2k_ranks.h", "g2k_kin.h",
                  "g2k_couples.h"):
        assert "g2k_coupled_" not in open(os.path.join(ROOT, "include", other)).read()
    lib = coupled.load()
    for name, (res, args) in coupled.SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.g2k_abi_version() == _lib.ABI_VERSION == 11
    assert coupled.load() is lib
    src = open(HEADER).read()
    assert int(re.search(r"G2K_COUPLED_SALT (0x[0-9A-Fa-f]+)ull", src).group(1), 16) == coupled.SALT == cr.SALT
    # the top bit set, the low 13 bits clear: x ^ SALT is no member seed of K <= 4096 draws
    assert coupled.SALT >> 63 == 1 and coupled.SALT & 0x1FFF == 0
    for x in (0, 1, 4095, 2 ** 63, 2 ** 63 - 1, 2 ** 64 - 1, coupled.SALT, coupled.SALT - 1, 0x123456789ABCDEF0):
        assert min((x ^ coupled.SALT) - x & (2 ** 64 - 1), x - (x ^ coupled.SALT) & (2 ** 64 - 1)) >= 4096
    for macro, value in (("DIM", coupled.DIM), ("COUNTS", coupled.NCOUNTS), ("STATS", coupled.NSTATS)):
        assert int(re.search(rf"G2K_COUPLED_{macro} (\d+)", src).group(1)) == value
    assert ("Alignment (bytes).  g2k_coupled_stats_f32: targets 8, whiten 8, within 8,\n"
            " * between 8, counts 8, stats 8, workspace 8.") in src
    assert HEADER in [os.path.abspath(p) for p in g2k_build.HDR]    # hashed, and a change rebuilds
    assert coupled.CoupledHead._PREFIX == "g2k_coupled_" and coupled.CoupledHead._JOINT_GPU_ONLY


# ---------------------------------------------------------------------------
# the validators: before any HIP call, in the header's order
# ---------------------------------------------------------------------------
DIMS = dict(S=2, F=3, T=8, L=12, D=16, H=64, Nmax=64, W=8, stride=0, flags=0)
ROW = 920 * 8
NEED = 2 * ROW                 # 6 scene-frames, 4 per workgroup at least: 2 workgroups, a row each
ST_ARGS = dict(pred=P, targets=2 * P, n_active=3 * P, n_frames=None, ped_mask=None, whiten=4 * P, within=5 * P,
               between=6 * P, counts=7 * P, stats=8 * P, ws=9 * P, ws_bytes=NEED, stream=None)
NULL = "a required buffer pointer is NULL"
ALIGN8 = "whiten, within, between, counts and stats must be 8-byte aligned"
ST_CHECKS = [
    ("dims", [({"dims": None}, EINVAL, "dims is NULL")]),
    ("flags", [({"flags": f}, EUNSUPPORTED, f"coupled_stats: flags {f} (0 or G2K_STEP_TARGETS_SHARED)")
               for f in (1, 4, 6, 256)]),
    ("sizes", [({"Nmax": 0}, EINVAL, "S=2 F=3 Nmax=0 (Nmax 1..256, S F < 2^31)"),
               ({"Nmax": 257}, EINVAL, "S=2 F=3 Nmax=257 (Nmax 1..256, S F < 2^31)"),
               ({"S": -1}, EINVAL, "S=-1 F=3 Nmax=64 (Nmax 1..256, S F < 2^31)"),
               ({"S": 1 << 16, "F": 1 << 15}, EINVAL, "S=65536 F=32768 Nmax=64 (Nmax 1..256, S F < 2^31)")]),
    ("required", [({n: None}, EINVAL, NULL) for n in ("pred", "targets", "n_active", "within", "between",
                                                      "counts", "stats")]),
    ("targets", [({"targets": 2 * P + 4}, EINVAL, "targets must be 8-byte aligned")]),
    ("align", [({n: ST_ARGS[n] + 4}, EINVAL, ALIGN8) for n in ("whiten", "within", "between", "counts", "stats")]),
    ("ws_align", [({"ws": 9 * P + 4}, EINVAL, "workspace must be 8-byte aligned")]),
    ("ws_size", [({"ws_bytes": NEED - 1}, EINVAL, f"workspace of {NEED} bytes needed (got {NEED - 1}), 8-byte aligned"),
                 ({"ws": None}, EINVAL, f"workspace of {NEED} bytes needed (got {NEED}), 8-byte aligned")]),
]
ST_SUCCESSES = ({"S": 0}, {"S": 0, "ws": None, "ws_bytes": 0}, {"S": 0, "F": 0}, {"S": 0, "flags": 2},
                {"S": 0, "whiten": None}, {"S": 0, "targets": 2 * P + 8, "whiten": 4 * P + 8, "within": 5 * P + 8,
                                           "between": 6 * P + 8, "counts": 7 * P + 8, "stats": 8 * P + 8,
                                           "ws": 9 * P + 8, "pred": P + 4})
SM_ARGS = dict(pred=P, cpl=2 * P, seed=5, out=3 * P, stream=None)
SM_CHECKS = [
    ("dims", [({"dims": None}, EINVAL, "dims is NULL")]),
    ("flags", [({"flags": 1}, EUNSUPPORTED, "coupled_sample reads pred_path_band [S, F, 2L, Nmax]")]),
    ("sizes", [({"Nmax": 0}, EINVAL, "S=2 F=3 Nmax=0"), ({"Nmax": 257}, EINVAL, "S=2 F=3 Nmax=257"),
               ({"F": -1}, EINVAL, "S=2 F=-1 Nmax=64")]),
    ("required", [({n: None}, EINVAL, NULL) for n in ("pred", "cpl", "out")]),
]


def _call(lib, symbol, base, faults):
    dims, args, null_dims = dict(DIMS), dict(base), False
    for key, value in faults.items():
        if key == "dims":
            null_dims = True
        elif key in dims:
            dims[key] = value
        else:
            assert key in args, (symbol, key)
            args[key] = value
    d = None if null_dims else ctypes.byref(_lib.G2KDims(**dims))
    rc_ = getattr(lib, symbol)(d, *args.values())
    return rc_, (lib.g2k_last_error() or b"").decode()


@pytest.mark.parametrize("symbol,base,checks", [("g2k_coupled_stats_f32", ST_ARGS, ST_CHECKS),
                                                ("g2k_coupled_sample_f32", SM_ARGS, SM_CHECKS)],
                         ids=["stats", "sample"])
def test_each_fault_alone_and_in_order(symbol, base, checks):
    lib = coupled.load()
    for label, ways in checks:
        for faults, code, message in ways:
            assert _call(lib, symbol, base, faults) == (code, message), (label, faults)
    # every adjacent pair of checks, both faults present: the earlier check's report
    for (label, first), (label2, second) in zip(checks[1:], checks[2:]):
        faults, code, message = first[0]
        both = dict(second[0][0], **faults)
        assert _call(lib, symbol, base, both) == (code, message), (label, label2)


def test_the_fused_entry_points_check_as_their_twins():
    """g2k_coupled_couple_scores_f32 under tests/test_couple_scores.py's whole
    table of faults, successes and refusals; g2k_coupled_joint_eval_f32 faults
    as g2k_fullcov_joint_eval_f32 does, message for message but its name."""
    lib = coupled.load()
    tcs.test_each_fault_alone_and_in_order("g2k_coupled_couple_scores_f32", "coupled_couple_scores")
    tcs.test_successes_that_launch_nothing("g2k_coupled_couple_scores_f32", "coupled_couple_scores")
    d = ctypes.byref(_lib.G2KDims(**dict(DIMS, Nmax=5)))
    need = lib.g2k_coupled_joint_eval_workspace_bytes(d)
    assert need == _lib.load().g2k_fullcov_joint_eval_workspace_bytes(d) > 0
    base = dict(pred=P, targets=2 * P, n_active=3 * P, n_frames=None, ped_mask=None, head=4 * P, seed=1, K=20,
                radius=0.1, per_frame_f=None, per_frame_i=None, sums_f=5 * P, sums_i=6 * P, ws=7 * P, ws_bytes=need,
                stream=None)
    twin = _lib.load().g2k_fullcov_joint_eval_f32
    for faults in ({"K": 0}, {"K": 4097}, {"radius": -1.0}, {"head": None}, {"sums_i": None}, {"targets": 2 * P + 4},
                   {"sums_i": 6 * P + 4}, {"ws": 7 * P + 2}, {"ws_bytes": need - 1}, {"flags": 1}):
        args = dict(base, **{k: v for k, v in faults.items() if k != "flags"})
        dd = ctypes.byref(_lib.G2KDims(**dict(DIMS, Nmax=5, flags=faults.get("flags", 0))))
        got = lib.g2k_coupled_joint_eval_f32(dd, *args.values()), lib.g2k_last_error().decode()
        want = twin(dd, *args.values()), lib.g2k_last_error().decode().replace("fullcov_", "coupled_")
        assert got == want and got[0] != OK, (faults, got, want)
    d0 = ctypes.byref(_lib.G2KDims(**dict(DIMS, S=0)))
    assert lib.g2k_coupled_joint_eval_f32(d0, *base.values()) == OK


def test_empty_batches_and_workspace_queries():
    lib = coupled.load()
    for faults in ST_SUCCESSES:                              # S = 0: a no-op, nothing dereferenced
        assert _call(lib, "g2k_coupled_stats_f32", ST_ARGS, faults)[0] == OK, faults
    for faults in ({"S": 0}, {"F": 0}, {"S": 0, "pred": P + 4, "cpl": 2 * P + 4, "out": 3 * P + 4}):
        assert _call(lib, "g2k_coupled_sample_f32", SM_ARGS, faults)[0] == OK, faults
    assert _call(lib, "g2k_coupled_stats_f32", ST_ARGS, {"S": 0, "flags": 4})[0] == EUNSUPPORTED
    assert _call(lib, "g2k_coupled_stats_f32", ST_ARGS, {"S": 0, "stats": None}) == (EINVAL, NULL)
    size = lib.g2k_coupled_stats_workspace_bytes

    def d(**kw):
        return ctypes.byref(_lib.G2KDims(**dict(DIMS, **kw)))
    assert size(d()) == NEED and size(d(S=1)) == 0 and size(d(S=0)) == 0 and size(d(F=0)) == 0
    assert size(d(S=4096, F=4)) == 256 * ROW and size(d(Nmax=256)) == 6 * ROW and size(d(Nmax=5, S=9, F=6)) == 2 * ROW
    assert size(None) == -1 and size(d(Nmax=0)) == -1 and size(d(Nmax=257)) == -1 and size(d(S=-1)) == -1
    for j, (name, case, _) in enumerate(cx.STATS):
        c = cx.stats_inputs(j)
        S, F, _, N = c["pred"].shape
        W, U = cx.stats_geometry(S, F, N)
        assert size(d(S=S, F=F, Nmax=N)) == (W * ROW if W > 1 else 0), name
        assert W * U >= S * F
    reach = {n: cx.stats_geometry(*[cx.stats_inputs(j)["pred"].shape[k] for k in (0, 1, 3)])[0]
             for j, (n, _, _) in enumerate(cx.STATS)}
    assert reach["k2"] == reach["k20"] == reach["shared"] == reach["single"] == 1       # writes the outputs itself
    assert reach["reach"] == 2 and reach["n256"] == 2 and reach["deal"] == 64            # the rows path


def test_stats_cases_reach_what_they_claim():
    seen = set()
    for j, (name, _, _) in enumerate(cx.STATS):
        c = cx.stats_inputs(j)
        Pn = c["members"].sum(axis=2)
        seen |= {("P", min(int(p), 3)) for p in np.unique(Pn)}
        n, g = int(Pn.sum()), int((Pn > 0).sum())
        if n == g and n > 0:
            seen.add("N == G")
        if n == 0:
            seen.add("no pair")
        if c["ped_mask"] is not None:
            seen.add("masked")
        if c["n_frames"] is not None and (c["n_frames"] < c["pred"].shape[1]).any():
            seen.add("n_frames < F")
        if c["shared"]:
            seen.add("shared")
    assert seen == {("P", 0), ("P", 1), ("P", 2), ("P", 3), "N == G", "no pair", "masked", "n_frames < F", "shared"}
    # Lb a multiple of Lw in the even cases, not in the odd ones
    for i in range(len(cx.IDS)):
        Lw, Lb = (np.tril(np.nan_to_num(m.astype(np.float64))) for m in cx.inputs(i)["cpl"])
        off = np.abs(Lb - Lb[0, 0] / Lw[0, 0] * Lw).max() / np.abs(Lb).max()
        assert (off < 1e-6) == (i % 2 == 0) and (off > 0.1) == (i % 2 == 1)
        assert np.isnan(cx.inputs(i)["cpl"][:, 0, 1]).all()


# ---------------------------------------------------------------------------
# flags and figure names
# ---------------------------------------------------------------------------
def test_evaluation_flags():
    from multimodaltraj_2_amd import evaluate
    from multimodaltraj_2_amd.argParser import ArgsParser
    a = ArgsParser().parser.parse_args([])
    assert a.coupled_head == "off"
    for mode in ("train", "eval"):
        assert ArgsParser().parser.parse_args(["--num_samples", "20", "--coupled_head", mode]).coupled_head == mode
    with pytest.raises(SystemExit):
        ArgsParser().parser.parse_args(["--coupled_head", "on"])
    assert evaluate.COUPLED_FIGURES == ("coupled_share", "coupled_nll", "coupled_nll_gain", "coupled_q_within",
                                        "coupled_q_between", "coupled_clipped")
    assert evaluate.COUPLED_JOINT_FIGURES == ("coupled_jade", "coupled_jfde", "coupled_collision_rate",
                                              "coupled_collision_rate_best")
    assert evaluate.COUPLED_CPL_FIGURES == tuple("coupled_" + k for k in evaluate.CPL_FIGURES)
    # refused before any data is read or any launch made
    a = ArgsParser().parser.parse_args(["--coupled_head", "eval"])
    with pytest.raises(ValueError, match="--num_samples"):
        evaluate.evaluate_best_of_k(a, None, None, log=lambda s: None)
    a.num_samples, a.couple_scores = 65, 1
    with pytest.raises(ValueError, match="2 <= K <= 64"):
        evaluate.evaluate_best_of_k(a, None, None, log=lambda s: None)
    # the figures of a result, in the stated order, on hand-made sums
    st = coupled.CoupledStats(within=torch.eye(DIM, dtype=torch.float64) * 90.0,
                              between=torch.eye(DIM, dtype=torch.float64) * 50.0,
                              counts=torch.tensor([100, 10, 10, 1000]),
                              stats=torch.tensor([300.0, 500.0, 24.0 * 90, 24.0 * 10, 7.0, 0.0], dtype=torch.float64),
                              log_det_lw=0.5)
    assert st.pairs == 100 and st.groups == 10
    np.testing.assert_allclose(st.W, np.eye(DIM))                    # 90 / (100 - 10)
    np.testing.assert_allclose(st.B_raw, np.eye(DIM) * 0.4)          # (50 - 10 * 1) / 100
    assert st.share == pytest.approx(0.4 / 1.4)
    const = 12 * np.log(2 * np.pi) + 0.5
    assert st.nll == pytest.approx(3.0 + const) and st.nll_independent == pytest.approx(5.0 + const)
    assert st.nll_gain == pytest.approx(2.0) and st.q_within_ratio == 1.0 and st.q_between_ratio == 1.0
    head = coupled.CoupledHead(device="cpu")
    head.clipped = 3
    fig = evaluate.coupled_figures(head, st)
    assert tuple(fig) == evaluate.COUPLED_FIGURES and fig["coupled_clipped"] == 3
    assert fig["coupled_nll_gain"] == st.nll_gain and fig["coupled_share"] == st.share
    none = coupled.CoupledStats(within=st.within, between=st.between, counts=st.counts, stats=st.stats,
                                has_head=False)
    assert none.nll is None and none.nll_gain is None and none.q_within_ratio is None


def test_python_argument_checks_and_host_paths():
    """What needs no GPU of the head's Python: the constructors, the marginal,
    the whitener and the refusals."""
    from multimodaltraj_2_amd.fullcov import FullCovHead
    c = cx.inputs(1)
    Lw, Lb = (np.tril(np.nan_to_num(m.astype(np.float64))) for m in c["cpl"])
    h = coupled.CoupledHead.from_factors(Lw, Lb, device="cpu")
    assert tuple(h.cpl.shape) == (2, DIM, DIM) and h.cpl.dtype == torch.float32 and h.clipped == 0
    A, lam = h.whitener()
    W, B = (h.cpl[0].double().numpy() @ h.cpl[0].double().numpy().T, h.cpl[1].double().numpy() @ h.cpl[1].double().numpy().T)
    np.testing.assert_allclose(A @ W @ A.T, np.eye(DIM), atol=1e-10)
    np.testing.assert_allclose(A @ B @ A.T, np.diag(lam), atol=1e-10)
    m = h.marginal()
    assert isinstance(m, FullCovHead)
    np.testing.assert_allclose(m.chol.double().numpy() @ m.chol.double().numpy().T, W + B, rtol=1e-5, atol=1e-6)
    fc = FullCovHead(device="cpu")
    fc.chol = torch.from_numpy(np.tril(np.nan_to_num(c["chol"])))
    two = coupled.CoupledHead.from_fullcov(fc, 0.6)
    np.testing.assert_allclose(two.cpl[0].numpy(), np.sqrt(0.4) * fc.chol.numpy(), rtol=1e-6)
    np.testing.assert_allclose(two.cpl[1].numpy(), np.sqrt(0.6) * fc.chol.numpy(), rtol=1e-6)
    np.testing.assert_allclose(two.marginal().chol.numpy(), fc.chol.numpy(), rtol=1e-5, atol=1e-6)
    zero = coupled.CoupledHead.from_fullcov(fc, 0.0)
    assert not zero.cpl[1].any() and not zero.whitener()[1].any()
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError, match="share"):
            coupled.CoupledHead.from_fullcov(fc, bad)
    with pytest.raises(ValueError, match="Lw and Lb"):
        coupled.CoupledHead.from_factors(Lw[:3], Lb)
    # the whitener follows cpl
    h.cpl = two.cpl
    np.testing.assert_allclose(h.whitener()[1], np.full(DIM, 1.5), rtol=1e-5)
    pred = torch.zeros((2, 1, DIM, 4))
    tg = torch.zeros((2, 1, 4, 12, 2))
    na = torch.full((2,), 4, dtype=torch.int32)
    for call in (lambda: h.stats(pred, tg[:, :, :3], na), lambda: h.fit(pred, tg, na[:1]),
                 lambda: h.joint_eval(pred, tg[:1], na, 4, 0.1), lambda: h.couple_scores(pred, tg, na[:1], 4)):
        with pytest.raises(ValueError, match="must be"):
            call()
    with pytest.raises(ValueError, match="GPU tensor"):
        h.joint_eval(pred, tg, na, 4, 0.1)
    h.cpl = h.cpl[:1]
    with pytest.raises(ValueError, match="cpl must be"):
        h.sample(pred)
    with pytest.raises(NotImplementedError, match="marginal"):
        two.best_of_k(pred, tg, na, 4)


# ---------------------------------------------------------------------------
# the checker alone
# ---------------------------------------------------------------------------
def test_checker_against_plain_loops():
    c = cx.stats_inputs(cx.STATS_IDS.index("k2"))
    g = cr.group_residuals(c["pred"], c["targets"], c["n_active"], c["n_frames"], c["ped_mask"])
    assert [len(r) for r in g] == [8, 8, 2, 0, 1, 1, 0, 0]
    a, b = cr.sums(g), cr.sums_loops(g)
    np.testing.assert_allclose(a["within"], b["within"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(a["between"], b["between"], rtol=1e-12, atol=1e-12)
    assert list(a["counts"]) == list(b["counts"]) == [20, 5, 3, 8 * 8 * 2 + 4 + 1 + 1]
    # the residuals are fullcov_ref's, regrouped
    flat = fr.residuals(c["pred"], c["targets"], c["n_active"], c["n_frames"], c["ped_mask"])
    np.testing.assert_array_equal(np.concatenate(g), flat)
    # SSW + SSB = the uncentred second moments
    np.testing.assert_allclose(a["within"] + a["between"], flat.T @ flat, rtol=1e-12, atol=1e-12)
    # the sampler by loops: one member of one scene-frame
    i = cx.IDS.index("k20")
    c = cx.inputs(i)
    Lw, Lb = fr.lower(c["cpl"][0]), fr.lower(c["cpl"][1])
    x = cr.sample(c["pred"], c["cpl"], c["seed"])
    z = fr.normals(c["pred"].shape, c["seed"])
    zc = fr.normals(c["pred"].shape, c["seed"] ^ cr.SALT)
    s, f = 1, 0
    for n in np.flatnonzero(c["members"][s, f])[:3]:
        for t in range(12):
            for co in range(2):
                i_ = 2 * t + co
                want = float(c["pred"][s, f, co * 12 + t, n])
                want += sum(Lb[i_, j] * zc[s, f, 0, j] for j in range(i_ + 1))
                want += sum(Lw[i_, j] * z[s, f, n, j] for j in range(i_ + 1))
                assert x[s, f, co * 12 + t, n] == pytest.approx(want, rel=1e-12, abs=1e-12)
    # two members of a scene-frame share c; Lb = 0 is the full-covariance sampler
    zero = np.stack([c["cpl"][0], np.zeros((DIM, DIM), np.float32)])
    np.testing.assert_array_equal(cr.sample(c["pred"], zero, 5), fr.sample(c["pred"], c["cpl"][0], 5))


@pytest.mark.parametrize("odd", [False, True], ids=["multiple", "own"])
def test_whitening_identity(odd):
    rng = np.random.default_rng(11)
    c = cx.inputs(1 if odd else 0)
    Lw, Lb = fr.lower(c["cpl"][0]), fr.lower(c["cpl"][1])
    W, B = Lw @ Lw.T, Lb @ Lb.T
    A, lam = cr.whitener(Lw, Lb)
    np.testing.assert_allclose(A @ W @ A.T, np.eye(DIM), atol=1e-11)
    np.testing.assert_allclose(A @ B @ A.T, np.diag(lam), atol=1e-11)
    ld = float(np.log(np.diag(Lw)).sum())
    for Pn in (1, 2, 5):
        r = rng.standard_normal((Pn, 1, DIM)) @ Lw.T + rng.standard_normal((1, 1, DIM)) @ Lb.T
        r = r[:, 0]
        got, want = cr.group_nll(r, A, lam, ld), cr.dense_nll(r, W, B)
        print(f"P {Pn}: whitened {got:.12g} dense {want:.12g}")
        assert abs(got - want) <= 1e-10 * abs(want)
        ind = cr.group_nll_independent(r, A, lam, ld)
        dense_ind = sum(cr.dense_nll(r[k:k + 1], W + B, np.zeros((DIM, DIM))) for k in range(Pn))
        assert abs(ind - dense_ind) <= 1e-10 * abs(dense_ind)
        if Pn == 1:
            assert abs(got - ind) <= 1e-10 * abs(got)            # one member: its marginal
    # lambda = 0: the coupled NLL is the independent head's
    A0, lam0 = cr.whitener(Lw, np.zeros((DIM, DIM)))
    assert not lam0.any()
    g = [rng.standard_normal((Pn, DIM)) for Pn in (1, 3, 6)]
    st = cr.nll_stats(g, A0, lam0)
    assert st[0] == pytest.approx(st[1], rel=1e-13) and st[3] + st[2] == pytest.approx(2 * st[0], rel=1e-13)
    assert st[4] == 0.0 and st[5] == 0.0


def _law(rng):
    """A known law: W, B from a case's factors."""
    c = cx.inputs(1)
    return fr.lower(c["cpl"][0]), fr.lower(c["cpl"][1])


def test_fit_recovers_the_law():
    Lw, Lb = _law(None)
    W, B = Lw @ Lw.T, Lb @ Lb.T
    truth = np.trace(B) / np.trace(W + B)
    shares = []
    for seed in range(5):
        rng = np.random.default_rng(100 + seed)
        groups = []
        for _ in range(400):                                   # unbalanced: P in 1..12
            Pn = int(rng.integers(1, 13))
            groups.append(rng.standard_normal((Pn, DIM)) @ Lw.T + rng.standard_normal((1, DIM)) @ Lb.T)
        s = cr.sums(groups)
        Wh, Bh = cr.moments_fit(s["within"], s["between"], s["counts"])
        fit = cr.project(Wh, Bh)
        shares.append(np.trace(fit["B"]) / np.trace(fit["W"] + fit["B"]))
        # the fitted head's q ratios on its own data: 1 by construction of the moments, up to the clipping
        st = cr.nll_stats(groups, fit["A"], fit["lam"])
        N, G = int(s["counts"][0]), int(s["counts"][1])
        assert st[2] / (DIM * (N - G)) == pytest.approx(1.0, abs=1e-4)
        assert st[0] < st[1]                                   # the coupling is worth something
        # coupled.project is the checker's
        Lw2, Lb2, A2, lam2, cl2 = coupled.project(coupled.ridged(Wh), Bh)
        np.testing.assert_allclose(Lw2, fit["Lw"], rtol=1e-12)
        np.testing.assert_allclose(Lb2 @ Lb2.T, fit["Lb"] @ fit["Lb"].T, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(lam2, fit["lam"], rtol=1e-9, atol=1e-12)
        assert cl2 == fit["clipped"]
    spread = max(shares) - min(shares)
    print(f"share: truth {truth:.4f}, fitted {min(shares):.4f}..{max(shares):.4f}")
    assert abs(np.mean(shares) - truth) <= spread and spread < 0.1


def test_indefinite_between_is_clipped():
    """Independent residuals in few groups: the raw B has negative eigenvalues;
    they are clipped, counted, and the factors stay usable."""
    rng = np.random.default_rng(3)
    groups = [rng.standard_normal((6, DIM)) for _ in range(12)]
    s = cr.sums(groups)
    Wh, Bh = cr.moments_fit(s["within"], s["between"], s["counts"])
    assert np.linalg.eigvalsh(Bh).min() < 0
    fit = cr.project(Wh, Bh)
    assert fit["clipped"] > 0 and (fit["lam"] >= 0).all() and np.linalg.eigvalsh(fit["B"]).min() > -1e-12
    assert np.isfinite(fit["Lb"]).all() and np.isfinite(fit["Lw"]).all() and (np.diag(fit["Lw"]) > 0).all()
    x = cr.sample(np.zeros((1, 1, DIM, 4)), np.stack([fit["Lw"], fit["Lb"]]), 1)
    assert np.isfinite(x).all()
    Lw2, Lb2, A2, lam2, cl2 = coupled.project(coupled.ridged(Wh), Bh)
    assert cl2 == fit["clipped"] and np.isfinite(Lb2).all()
    # every eigenvalue negative: Lb is zeros
    z = cr.project(np.eye(DIM), -np.eye(DIM))
    assert z["clipped"] == DIM and not z["Lb"].any() and not z["lam"].any()
    assert not coupled.project(np.eye(DIM), -np.eye(DIM))[1].any()


# ---------------------------------------------------------------------------
# what the head is for
# ---------------------------------------------------------------------------
PROP = dict(S=8, F=8, N=16, K=20, B=7, seed=4242, sigma=0.5, share=0.8, side=4.0, fit_seed=77, score_seed=78)


def property_pred():
    return cc.property_setup(PROP["S"], PROP["F"], PROP["N"], PROP["side"])


def property_targets(pred, which):
    """Two independent sets of coupled targets: one to fit on, one to score."""
    return cc.coupled_targets(pred, PROP["sigma"], PROP["share"], rng_seed=PROP[which + "_seed"])


def property_check(score, label=""):
    """``score(kind)`` -> dict feature -> dict(dev, crps, pit_mean) of the
    scoring targets under the K joint draws of the "coupled" head fitted on the
    other set and of the "fullcov" head with the same marginals."""
    co, fc = score("coupled"), score("fullcov")
    for kind, v in (("coupled", co), ("fullcov", fc)):
        print(f"{label}{kind}: " + ", ".join(f"{g} dev {v[g]['dev']:.4f} crps {v[g]['crps']:.4f} pit "
                                             f"{v[g]['pit_mean']:.4f}" for g in cpr.FEATURES))
    assert co["min"]["dev"] < DEV_MATCHED and co["fin"]["dev"] < DEV_MATCHED
    assert fc["fin"]["dev"] > DEV_FIN and fc["min"]["dev"] > DEV_MIN
    assert co["fin"]["crps"] < fc["fin"]["crps"]


@pytest.mark.parametrize("at", BOUNDARY_SEEDS)
def test_couple_scores_boundary_seeds_have_no_ties_and_see_the_carry(at):
    """Case k2 with the scene-coupled head at the seeds whose low word carries at
    draw 1 (tests/test_coupled_head_gpu.py runs g2k_coupled_couple_scores_f32
    there)."""
    c = cx.inputs(cx.IDS.index("k2"))

    def draws_of(carry):
        with np.errstate(invalid="ignore"):
            return np.stack([cr.sample(c["pred"], c["cpl"], draw_seed(BOUNDARY_SEEDS[at], k, carry))
                             for k in range(c["K"])]).astype(np.float32)
    tcs.carry_check(draws_of, c, f"k2 seed {at} coupled")


def test_coupled_targets_are_matched_by_the_coupled_head():
    S, F, N, K, B, seed = (PROP[k] for k in ("S", "F", "N", "K", "B", "seed"))
    pred = property_pred()
    members = np.ones((S, F, N), bool)
    na = np.full(S, N, np.int32)
    s = cr.sums(cr.group_residuals(pred, property_targets(pred, "fit"), na))
    fit = cr.project(*cr.moments_fit(s["within"], s["between"], s["counts"]))
    share = np.trace(fit["B"]) / np.trace(fit["W"] + fit["B"])
    print(f"fitted share {share:.4f}, clipped {fit['clipped']}")
    assert abs(share - PROP["share"]) < 0.03 and fit["clipped"] == 0
    cpl = np.stack([fit["Lw"], fit["Lb"]]).astype(np.float32)
    marg = np.linalg.cholesky(fit["W"] + fit["B"]).astype(np.float32)
    tg = property_targets(pred, "score")

    def score(kind):
        if kind == "coupled":
            draws = np.stack([cr.sample(pred, cpl, seed + k) for k in range(K)]).astype(np.float32)
        else:
            draws = np.stack([fr.sample(pred, marg, seed + k) for k in range(K)]).astype(np.float32)
        R = cpr.couple_scores_ref(draws, tg, pred, members, K, B)
        assert R["tot"][:, 0].sum() == S * F * N * (N - 1) // 2
        fig = cpr.figures(R["sums"], R["hist"], R["tot"], K)
        return {g: fig[g] for g in cpr.FEATURES}
    property_check(score)
