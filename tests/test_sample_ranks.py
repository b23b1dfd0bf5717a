"""CPU: the rank-histogram calibration (include/g2k_ranks.h,
multimodaltraj_2_amd/ranks.py, csrc/g2k_ranks.hip) — the header, the module's
binding table and the library's exports agree; every validator rejects bad
arguments before touching the GPU; the launch geometry is what
tests/ranks_cases.py claims, every branch of it reached; and the float64
checker tests/ranks_ref.py alone: against plain loops, closed forms, the
interval margins and the wide-interval cap on the oracle's draws, and the
reason the ranks exist — a target drawn from the head's own law has a uniform
rank, a head three times too wide does not."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from multimodaltraj_2_amd import _lib, mixture, modes, ranks, scores
from multimodaltraj_2_amd import build as g2k_build
from oracle import g2k_ref as ref
from tests import ranks_cases as rc
from tests import ranks_ref as rr
from tests.bestk_ref import SEED_A
from tests.bestk_ref import MASK64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2k_ranks.h")
P = 0x10000                    # a non-NULL pointer, 64-byte aligned (never dereferenced)
OK, EINVAL, EUNSUPPORTED = 0, -1, -4
ENTRIES = (("g2k_sample_ranks_f32", "sample_ranks"), ("g2k_fullcov_sample_ranks_f32", "fullcov_sample_ranks"),
           ("g2k_mix_sample_ranks_f32", "mix_sample_ranks"))
L = 12


def _declarations():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(g2k_[a-z0-9_]+)\s*\(([^)]*)\)", src)}


# ---------------------------------------------------------------------------
# the header, the binding and the exports
# ---------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    decl = _declarations()
    assert sorted(decl) == sorted(ranks.SYMBOLS)
    for name, args in decl.items():
        assert len(args.split(",")) == len(ranks.SYMBOLS[name][1]), name
    # by symbol, after ABI 11: in no other header or table
    for table in (_lib.SYMBOLS, mixture.SYMBOLS, scores.SYMBOLS, modes.SYMBOLS):
        assert not set(decl) & set(table)
    for other in ("g2k_hip.h", "g2k_mix.h", "g2k_scores.h", "g2k_modes.h"):
        assert "sample_ranks" not in open(os.path.join(ROOT, "include", other)).read()
    lib = ranks.load()
    for name, (res, args) in ranks.SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.g2k_abi_version() == _lib.ABI_VERSION == 11
    assert ranks.load() is lib
    src = open(HEADER).read()
    for macro, value in (("KMIN", ranks.KMIN), ("KMAX", ranks.KMAX), ("BMAX", ranks.BMAX), ("ROWS", ranks.ROWS)):
        assert int(re.search(rf"G2K_RANKS_{macro} (\d+)", src).group(1)) == value
    assert (ranks.KMIN, ranks.KMAX, ranks.BMAX, ranks.ROWS) == (rr.K_MIN, rr.K_MAX, rr.B_MAX, rr.ROWS) == (4, 255, 64, 13)
    assert int(re.search(r"G2K_RANKS_GEOM_FIELDS (\d+)", src).group(1)) == len(ranks.GEOM_FIELDS)
    for i, f in enumerate(ranks.GEOM_FIELDS):
        assert int(re.search(rf"G2K_RANKS_GEOM_{f.upper()} (\d+)", src).group(1)) == i
    assert ranks.GEOM_FIELDS == scores.GEOM_FIELDS
    assert ("Alignment (bytes) of g2k_sample_ranks_f32, g2k_fullcov_sample_ranks_f32\n"
            " * and g2k_mix_sample_ranks_f32: targets 8, per_ped 16, hist 4, tot 8,\n"
            " * workspace 8.") in src
    assert HEADER in [os.path.abspath(p) for p in g2k_build.HDR]    # hashed, and a change rebuilds


# ---------------------------------------------------------------------------
# the validators: before any HIP call
# ---------------------------------------------------------------------------
DIMS = dict(S=2, F=3, T=8, L=12, D=16, H=64, Nmax=5, W=8, stride=0, flags=0)
NEED = 2 * 3 * (4 * 8 + 13 * 7 * 4)             # S * F rows of {tot [4] int64, hist [13][B = 7] int32}
ARGS = dict(pred=P, targets=2 * P, n_active=3 * P, n_frames=None, ped_mask=None, head=6 * P, seed=7, K=20,
            B=7, per_ped=7 * P, hist=8 * P, tot=10 * P, ws=9 * P, ws_bytes=NEED, stream=None)
FLAGS = "{name}: flags %d (0 or G2K_STEP_TARGETS_SHARED)"
NULL = "a required buffer pointer is NULL"
# the checks in the order the library runs them; each fault alone, with its code and full message
CHECKS = [
    ("dims", [({"dims": None}, EINVAL, "dims is NULL")]),
    ("flags", [({"flags": f}, EUNSUPPORTED, FLAGS % f) for f in (1, 4, 6, 256)]),
    ("sizes", [({"Nmax": 0}, EINVAL, "S=2 F=3 Nmax=0"), ({"Nmax": 257}, EINVAL, "S=2 F=3 Nmax=257"),
               ({"S": -1}, EINVAL, "S=-1 F=3 Nmax=5"), ({"F": -1}, EINVAL, "S=2 F=-1 Nmax=5")]),
    ("K", [({"K": 3, "B": 1}, EINVAL, "K=3 (4..255)"), ({"K": 256, "B": 1}, EINVAL, "K=256 (4..255)"),
           ({"K": 0, "B": 1}, EINVAL, "K=0 (4..255)")]),
    ("B", [({"B": 0}, EINVAL, "B=0 (1..64, a divisor of K + 1 = 21)"),
           ({"B": 4}, EINVAL, "B=4 (1..64, a divisor of K + 1 = 21)"),
           ({"B": 20}, EINVAL, "B=20 (1..64, a divisor of K + 1 = 21)"),
           ({"B": 65, "K": 129}, EINVAL, "B=65 (1..64, a divisor of K + 1 = 130)"),
           ({"B": -1}, EINVAL, "B=-1 (1..64, a divisor of K + 1 = 21)")]),
    ("required", [({n: None}, EINVAL, NULL) for n in ("pred", "targets", "n_active", "head", "hist", "tot")]),
    ("targets", [({"targets": 2 * P + 7}, EINVAL, "targets must be 8-byte aligned"),
                 ({"targets": 2 * P + 4}, EINVAL, "targets must be 8-byte aligned")]),
    ("per_ped", [({"per_ped": 7 * P + 15}, EINVAL, "per_ped must be 16-byte aligned"),
                 ({"per_ped": 7 * P + 8}, EINVAL, "per_ped must be 16-byte aligned")]),
    ("hist", [({"hist": 8 * P + 3}, EINVAL, "hist must be 4-byte aligned"),
              ({"hist": 8 * P + 2}, EINVAL, "hist must be 4-byte aligned")]),
    ("tot", [({"tot": 10 * P + 7}, EINVAL, "tot must be 8-byte aligned"),
             ({"tot": 10 * P + 4}, EINVAL, "tot must be 8-byte aligned")]),
    ("ws_align", [({"ws": 9 * P + 7}, EINVAL, "workspace must be 8-byte aligned"),
                  ({"ws": 9 * P + 4}, EINVAL, "workspace must be 8-byte aligned")]),
    ("ws_size", [({"ws_bytes": NEED - 1}, EINVAL, f"workspace of {NEED} bytes needed (got {NEED - 1})"),
                 ({"ws": None}, EINVAL, f"workspace of {NEED} bytes needed (got {NEED})"),
                 ({"ws_bytes": 0}, EINVAL, f"workspace of {NEED} bytes needed (got 0)")]),
]
# what returns G2K_OK without a launch, at the weakest alignments the header states
SUCCESSES = ({"S": 0}, {"S": 0, "ws": None, "ws_bytes": 0}, {"S": 0, "F": 0, "ws_bytes": 0},
             {"S": 0, "flags": 2}, {"S": 0, "per_ped": None, "K": 255, "B": 64}, {"S": 0, "K": 4, "B": 5},
             {"S": 0, "targets": 2 * P + 8, "per_ped": 7 * P + 16, "hist": 8 * P + 4, "tot": 10 * P + 8,
              "ws": 9 * P + 8, "pred": P + 4, "head": 6 * P + 4})
REFUSALS = (({"S": 0, "flags": 4}, EUNSUPPORTED, FLAGS % 4), ({"S": 0, "K": 3, "B": 1}, EINVAL, "K=3 (4..255)"),
            ({"S": 0, "B": 2}, EINVAL, "B=2 (1..64, a divisor of K + 1 = 21)"),
            ({"S": 0, "tot": None}, EINVAL, NULL), ({"S": 0, "ws": 9 * P + 4}, EINVAL,
                                                    "workspace must be 8-byte aligned"))


def _call(lib, symbol, faults):
    dims, args, null_dims = dict(DIMS), dict(ARGS), False
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


@pytest.mark.parametrize("symbol,name", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_each_fault_alone_and_in_order(symbol, name):
    lib = ranks.load()
    for label, ways in CHECKS:
        for faults, code, message in ways:
            assert _call(lib, symbol, faults) == (code, message.format(name=name)), (label, faults)
    # every adjacent pair of checks, both faults present: the earlier check's report
    for (label, first), (label2, second) in zip(CHECKS[1:], CHECKS[2:]):
        faults, code, message = first[0]
        both = dict(second[0][0], **faults)
        assert _call(lib, symbol, both) == (code, message.format(name=name)), (label, label2)


@pytest.mark.parametrize("symbol,name", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_successes_that_launch_nothing(symbol, name):
    lib = ranks.load()
    for faults in SUCCESSES:
        rc_, msg = _call(lib, symbol, faults)
        assert rc_ == OK, (faults, msg)
    for faults, code, message in REFUSALS:
        assert _call(lib, symbol, faults) == (code, message.format(name=name)), faults


def test_workspace_bytes_and_geometry_queries():
    lib = ranks.load()
    size = lib.g2k_sample_ranks_workspace_bytes

    def d(**kw):
        return ctypes.byref(_lib.G2KDims(**dict(DIMS, **kw)))
    assert size(d(), 7) == NEED and size(d(), 1) == 6 * (32 + 52) and size(d(), 64) == 6 * (32 + 52 * 64)
    assert size(d(F=0), 7) == 2 * (32 + 364) and size(d(S=0), 7) == 0
    assert size(None, 7) == -1
    for bad in (dict(Nmax=0), dict(Nmax=257), dict(S=-1), dict(F=-1)):
        assert size(d(**bad), 7) == -1
    assert size(d(), 0) == -1 and size(d(), 65) == -1 and size(d(), -3) == -1
    out = (ctypes.c_int32 * 5)()
    geo = lib.g2k_sample_ranks_geometry
    for args, msg in (((None, 20, out), "dims is NULL"), ((d(Nmax=257), 20, out), "S=2 F=3 Nmax=257"),
                      ((d(), 3, out), "K=3 (4..255)"), ((d(), 256, out), "K=256 (4..255)"),
                      ((d(), 20, None), "out is NULL")):
        assert geo(*args) == EINVAL and lib.g2k_last_error().decode() == msg
    assert geo(d(), 20, out) == OK and geo(d(S=0), 4, out) == OK and geo(d(flags=1), 255, out) == OK


# ---------------------------------------------------------------------------
# the geometry: what tests/ranks_cases.py claims, every branch reached
# ---------------------------------------------------------------------------
def test_geometry_claims_and_branches():
    reached = set()
    for i, case in enumerate(rc.CASES):
        name, S, F, N, K, B = case[:6]
        c = rc.inputs(i)
        g = ranks.sample_ranks_geometry(S, F, N, K)
        assert {k: g[k] for k in ("g", "fc", "c")} == c["geom"], (name, g)
        assert g["lanes"] == K and g["g"] * K <= 256
        assert rc.passes_of(i) == c["passes"], (name, rc.passes_of(i))
        assert (K + 1) % B == 0 and 1 <= B <= 64
        # LDS: the draws [256][24], the pairs' targets and means [32][24] each, their inverse
        # factors [32][12][4], the targets' sums [32][13], the lanes' bits [256], the histogram
        # [13][64] and the four totals; with the mixture head's 19376 bytes below 64 KB
        assert g["lds_bytes"] == 4 * (256 * 24 + 2 * 32 * 24 + 32 * 12 * 4 + 32 * 13 + 256 + 13 * 64 + 4)
        assert g["lds_bytes"] + 19376 <= 65536
        # the same shapes give the scores' kernel the same geometry
        assert {k: scores.sample_scores_geometry(S, F, N, K)[k] for k in ("g", "fc", "c")} == c["geom"]
        reached.add("G capped" if 256 // K > 32 else "G = 256 // K")
        raw = 4 * g["g"] // N
        reached.add("FC cut by F" if raw > F else "FC raised to 1" if raw < 1 else "FC = 4 G // Nmax")
        reached.add("rows kernel" if g["c"] > 1 else "one workgroup per scene")
        reached.add("several passes" if c["passes"] > 1 else "one pass")
        if c["passes"] > 1 and (int(c["n_active"].max()) * g["fc"]) % g["g"]:
            reached.add("partial last group")
        if K > 64:
            reached.add("pair past one wave")
        if K == 64:
            reached.add("pair = one wave")
        if 64 % K:
            reached.add("pair straddles waves")
        if g["fc"] > 1 and F % g["fc"]:
            reached.add("short last chunk")
        if any(int(n) == 0 for n in c["n_active"]):
            reached.add("empty scene")
        if c["shared"]:
            reached.add("shared targets")
        reached.add({4: "K minimum", 255: "K maximum"}.get(K, "K between"))
        reached.add("B = K + 1" if B == K + 1 else "B maximum" if B == 64 else "B minimum" if B == 1
                    else "several ranks per bin")
        if N == 256:
            reached.add("Nmax maximum")
    assert reached == {"G capped", "G = 256 // K", "FC cut by F", "FC raised to 1", "FC = 4 G // Nmax",
                       "rows kernel", "one workgroup per scene", "several passes", "one pass",
                       "partial last group", "pair past one wave", "pair = one wave", "pair straddles waves",
                       "short last chunk", "empty scene", "shared targets", "K minimum", "K maximum",
                       "K between", "B = K + 1", "B maximum", "B minimum", "several ranks per bin",
                       "Nmax maximum"}, reached
    # the evaluation's two timing shapes (tools/time_sample_ranks.py)
    assert ranks.sample_ranks_geometry(256, 20, 32, 20) == dict(g=12, lanes=20, fc=1, c=20, lds_bytes=42896)
    assert ranks.sample_ranks_geometry(128, 20, 256, 20)["c"] == 20
    # F = 0: one workgroup per scene, which writes the zeros
    assert ranks.sample_ranks_geometry(3, 0, 16, 20)["c"] == 1


# ---------------------------------------------------------------------------
# the checker against an independent restatement, and its margins
# ---------------------------------------------------------------------------
def _loops(x, y):
    """x [K, L, 2], y [L, 2] -> (the 13 ranks, -1 for a degenerate step) by plain loops."""
    K = x.shape[0]
    z = [y] + [x[k] for k in range(K)]
    out = []
    for t in range(L):
        pts = [p[t] for p in z]
        mx = sum(p[0] for p in pts) / (K + 1)
        my = sum(p[1] for p in pts) / (K + 1)
        cxx = sum((p[0] - mx) ** 2 for p in pts) / K
        cyy = sum((p[1] - my) ** 2 for p in pts) / K
        cxy = sum((p[0] - mx) * (p[1] - my) for p in pts) / K
        f = (K + 1) ** (-1.0 / 3.0)
        H = np.array([[cxx, cxy], [cxy, cyy]]) * f
        if not np.linalg.det(H) > 0:
            out.append(-1)
            continue
        Hi = np.linalg.inv(H)
        rho = [sum(float(np.exp(-0.5 * (p - q) @ Hi @ (p - q))) for j, q in enumerate(pts) if j != i)
               for i, p in enumerate(pts)]
        out.append(sum(rho[1 + k] > rho[0] for k in range(K)))
    e = [sum(float(np.sqrt(((p - q) ** 2).sum())) for j, q in enumerate(z) if j != i) for i, p in enumerate(z)]
    out.append(sum(e[1 + k] < e[0] for k in range(K)))
    return out


def test_checker_against_plain_loops():
    i = rc.IDS.index("k4")
    c = rc.inputs(i)
    checked = 0
    for which in rc.HEADS:
        draws = rc.oracle_draws(i, which)
        R = rr.sample_ranks_ref(draws, c["targets"], c["pairs"])
        x = rr.band_to_xy(draws).astype(np.float64)
        S, F, N = c["pairs"].shape
        y = np.broadcast_to(c["targets"].astype(np.float64), (S, F, N, L, 2))
        for s, f, n in np.argwhere(c["pairs"])[::3]:
            assert list(R["r"][s, f, n]) == _loops(x[:, s, f, n], y[s, f, n]), (which, s, f, n)
            checked += 1
        assert np.all(R["r"][~c["pairs"]] == 0) and np.all(R["r_lo"] <= R["r"]) and np.all(R["r"] <= R["r_hi"])
        assert R["r"].min() >= 0 and R["r"].max() <= c["K"] and not R["deg"].any()
    assert checked >= 12


def test_margins_and_wide_interval_cap_on_the_oracles_draws():
    """The recorded deviation bounds what the fp32 restatement does on every
    case and head (M is four times it), and M leaves at most WIDE_CAP of a
    case's (pair, row) intervals wider than one rank."""
    assert rr.M == 4 * rr.MEASURED and rr.A == 1e-30 and rr.WIDE_CAP == 0.05
    worst = 0.0
    for i, name in enumerate(rc.IDS):
        c = rc.inputs(i)
        for which in rc.HEADS:
            draws = rc.oracle_draws(i, which)
            dv = rr.deviation(draws, c["targets"], c["pairs"], c["pred"], which == "mix")
            R = rr.sample_ranks_ref(draws, c["targets"], c["pairs"])
            wide = float((R["r_hi"] > R["r_lo"])[c["pairs"]].mean())
            print(f"{name} {which}: deviation {dv:.3g}, wide intervals {wide:.4f}, degenerate {int(R['deg'].sum())}")
            assert wide <= rr.WIDE_CAP, (name, which, wide)
            assert not R["deg"].any() and not R["deg_open"][c["pairs"]].any()
            worst = max(worst, dv)
    print(f"worst deviation {worst:.3g} (recorded {rr.MEASURED}), M = {rr.M}")
    assert worst <= rr.MEASURED


@pytest.mark.parametrize("which", rc.HEADS)
def test_boundary_seed_intervals_and_the_carry(which):
    """Case k4 at seed A, whose low word carries at draw 1
    (tests/test_sample_ranks_gpu.py runs the kernel there): the wide-interval
    cap and no degenerate step on the restated draws, and the checker's ranks
    change when the draws are made with the carry dropped."""
    i = rc.IDS.index("k4")
    c = rc.inputs(i)
    R, D = (rr.sample_ranks_ref(rc.oracle_draws(i, which, SEED_A, carry), c["targets"], c["pairs"])
            for carry in (True, False))
    for v in (R, D):
        assert float((v["r_hi"] > v["r_lo"])[c["pairs"]].mean()) <= rr.WIDE_CAP
        assert not v["deg"].any() and not v["deg_open"][c["pairs"]].any()
    dv = rr.deviation(rc.oracle_draws(i, which, SEED_A), c["targets"], c["pairs"], c["pred"], which == "mix")
    assert dv <= rr.MEASURED
    # the ranks change by more than any interval's width allows: outside the right draws' intervals
    out = c["pairs"][..., None] & ((D["r"] < R["r_lo"]) | (D["r"] > R["r_hi"]))
    print(f"k4 seed A {which}: carry dropped, {int((D['r'] != R['r']).sum())} ranks change, {int(out.sum())} "
          f"leave their interval")
    assert out.sum() > 0


# ---------------------------------------------------------------------------
# closed forms
# ---------------------------------------------------------------------------
def _band(xy):
    """[..., N, L, 2] -> [..., 2L, N]."""
    a = np.moveaxis(np.asarray(xy), -3, -1)                         # [..., L, 2, N]
    return np.concatenate([a[..., 0, :], a[..., 1, :]], axis=-2)


def test_closed_forms():
    rng = np.random.default_rng(17)
    K, N = 20, 6
    pairs = np.ones((1, 1, N), bool)
    x = rng.standard_normal((K, 1, 1, N, L, 2))
    # a target far outside every draw: the most outlying point under both pre-ranks
    far = np.full((1, 1, N, L, 2), 60.0)
    R = rr.sample_ranks_ref(_band(x), far, pairs)
    assert np.all(R["r"] == K) and np.all(R["r_lo"] == K) and np.all(R["r_hi"] == K)
    # a target at the centre of a symmetric cross of draws: the most typical point
    cross = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
    xc = np.broadcast_to(cross[:, None, None, None, None, :], (4, 1, 1, N, L, 2))
    R = rr.sample_ranks_ref(_band(xc), np.zeros((1, 1, N, L, 2)), pairs)
    assert np.all(R["r"] == 0) and np.all(R["r_hi"] == 0)
    # log sigma = -200: sigma = 0, the K draws are the prediction itself.  The pooled points of a
    # step lie on one line (on one point where the target is the prediction too): every step is
    # degenerate, exactly so when the target is off along one axis only; r_traj = K
    head = np.zeros((3, L), np.float32)
    head[:2] = -200.0
    pred = rng.integers(-3, 4, (1, 1, 2 * L, N)).astype(np.float32)
    draws = np.stack([ref.gauss_sample(pred, head, (5 + k) & MASK64) for k in range(K)]).astype(np.float32)
    assert np.all(draws == pred)
    tg = rr.band_to_xy(pred).astype(np.float32).copy()
    tg[..., 0:5, 0] += 2.0
    tg[..., 5:10, 1] -= 3.0                                          # steps 10, 11: the target is the draws
    R = rr.sample_ranks_ref(draws, tg, pairs)
    assert R["deg"].all() and np.all(R["r"][..., :L] == -1) and np.all(R["r"][..., L] == K)
    per = np.zeros((1, 1, N, 16))
    per[..., :13] = R["r"]
    hist, tot = rr.hist_tot(per, pairs, K, 21)
    assert np.all(hist[:, :L] == 0) and hist[0, L, 20] == N and hist[0, L].sum() == N
    assert list(tot[0]) == [N, 12 * N, 0, K * N]


@pytest.mark.parametrize("K,B", [(20, 21), (20, 7), (255, 32)])
def test_bin_edges(K, B):
    """Every rank 0..K once: (K + 1) / B in each bin, bin floor(r B / (K + 1));
    the result class's shares, coverage edges and means on hand-made counts."""
    w = (K + 1) // B
    per = np.zeros((1, 1, K + 1, 16))
    per[0, 0, :, :13] = np.arange(K + 1)[:, None]
    pairs = np.ones((1, 1, K + 1), bool)
    hist, tot = rr.hist_tot(per, pairs, K, B)
    assert np.all(hist == w)
    for r in (0, w - 1, w, K - w, K - w + 1, K):
        one = np.zeros((1, 1, 1, 16))
        one[..., :13] = r
        h, _ = rr.hist_tot(one, np.ones((1, 1, 1), bool), K, B)
        assert h[0, 0, r * B // (K + 1)] == 1 and r * B // (K + 1) == r // w
    assert ranks.auto_bins(K) == {20: 21, 255: 32}[K]
    sr = ranks.SampleRanks(hist=torch.from_numpy(hist.astype(np.int32)), tot=torch.from_numpy(tot), per_ped=None,
                           k=K, bins=B)
    assert sr.pairs == K + 1 and sr.degenerate_share == 0.0
    assert sr.hist_steps.shape == (12, B) and sr.hist_pooled.shape == (B,) and sr.hist_traj.shape == (B,)
    assert sr.dev == 0.0 and sr.dev_final == 0.0 and sr.dev_traj == 0.0
    assert sr.mean == pytest.approx(0.5, abs=1e-15) and sr.mean_traj == pytest.approx(0.5, abs=1e-15)
    for p in (0.5, 0.9):
        nom, obs = sr.coverage(p)
        j = int(np.floor(p * B + 1e-9))
        assert nom == j / B <= p < (j + 1) / B and obs == pytest.approx(nom, abs=1e-12)
    # everything in the last bin: as far from uniform as it gets; no pair: NaN
    hist[:] = 0
    hist[:, :, B - 1] = K + 1
    sr = ranks.SampleRanks(hist=torch.from_numpy(hist.astype(np.int32)), tot=torch.from_numpy(tot), per_ped=None,
                           k=K, bins=B)
    assert sr.dev == pytest.approx(1.0 - 1.0 / B) and sr.coverage(0.9)[1] == 0.0
    empty = ranks.SampleRanks(hist=torch.zeros((2, 13, B), dtype=torch.int32),
                              tot=torch.zeros((2, 4), dtype=torch.int64), per_ped=None, k=K, bins=B)
    assert empty.pairs == 0 and all(np.isnan(v) for v in (empty.dev, empty.dev_traj, empty.mean, empty.mean_traj,
                                                          empty.degenerate_share, empty.coverage(0.5)[1]))


def test_python_argument_checks():
    for k in (3, 256):
        with pytest.raises(ValueError, match="4..255"):
            ranks.check_k_bins(k, None)
    for b in (4, 65, -1):
        with pytest.raises(ValueError, match="a divisor of k \\+ 1"):
            ranks.check_k_bins(20, b)
    assert ranks.check_k_bins(20, None) == (20, 21) and ranks.check_k_bins(20, 0) == (20, 21)
    assert ranks.check_k_bins(255, None) == (255, 32) and ranks.check_k_bins(255, 64) == (255, 64)
    assert ranks.check_k_bins(130, None) == (130, 1)                 # 131 is prime
    assert [ranks.auto_bins(k) for k in (4, 6, 8, 40, 64, 65)] == [5, 7, 9, 1, 13, 22]


# ---------------------------------------------------------------------------
# what the ranks are for: exchangeability
# ---------------------------------------------------------------------------
EXCH = (8, 8, 32)               # S, F, N: 2048 pairs


@pytest.mark.parametrize("which", rc.HEADS)
def test_exchangeability(which):
    """Targets = the oracle sampler's draw for seed + K: the K + 1 trajectories
    are exchangeable, so step 11's rank and the trajectory's are uniform on
    0..20.  Pearson's chi^2 over the 21 bins against the 0.999 quantile at 20
    degrees of freedom; the seeds are fixed, so the outcome is deterministic.
    The negative control: the same targets under draws of the head with its
    factor scaled by 3 (too wide: the target is too typical) must exceed it."""
    S, F, N = EXCH
    K, B, seed = 20, 21, 4242
    c = rc.inputs(rc.IDS.index("k20"))
    rng = np.random.default_rng(99)
    pred = rng.standard_normal((S, F, 2 * L, N)).astype(np.float32)
    pairs = np.ones((S, F, N), bool)
    draw = rc.sampler(which, c)
    tg = rr.band_to_xy(np.asarray(draw(pred, seed + K), np.float32))
    quant = rr.chi2_quantile(0.999, B - 1)
    assert abs(quant - 45.31) < 0.15
    stats = {}
    for label, by in (("same law", 1.0), ("three times too wide", 3.0)):
        dr = rc.sampler(which, rc.scaled(which, c, by))
        draws = np.stack([dr(pred, seed + k) for k in range(K)]).astype(np.float32)
        R = rr.sample_ranks_ref(draws, tg, pairs)
        assert not R["deg"].any()
        per = np.zeros((S, F, N, 16))
        per[..., :13] = R["r"]
        hist, tot = rr.hist_tot(per, pairs, K, B)
        h = hist.sum(axis=0)
        stats[label] = (rr.chi2(h[L - 1]), rr.chi2(h[L]), (tot[:, 2].sum() + 6.0 * S * F * N) / (21 * 12 * S * F * N))
        print(f"{which}, {label}: chi^2 step 11 {stats[label][0]:.2f}, trajectory {stats[label][1]:.2f} "
              f"(0.999 quantile {quant:.2f}), mean rank {stats[label][2]:.4f}")
    assert stats["same law"][0] < quant and stats["same law"][1] < quant
    assert stats["three times too wide"][0] > quant and stats["three times too wide"][1] > quant
    assert stats["three times too wide"][2] < 0.45                  # too wide: the target is too typical


# ---------------------------------------------------------------------------
# the evaluation's flags
# ---------------------------------------------------------------------------
def test_evaluation_flags():
    from multimodaltraj_2_amd import evaluate
    from multimodaltraj_2_amd.argParser import ArgsParser
    a = ArgsParser().parser.parse_args([])
    assert a.sample_ranks == 0 and a.rank_bins == 0
    a = ArgsParser().parser.parse_args(["--num_samples", "20", "--sample_ranks", "1", "--rank_bins", "7"])
    assert a.sample_ranks == 1 and a.rank_bins == 7
    with pytest.raises(SystemExit):
        ArgsParser().parser.parse_args(["--sample_ranks", "2"])
    assert evaluate.RANK_FIGURES == ("rank_dev", "rank_dev_final", "rank_dev_traj", "rank_mean",
                                     "rank_mean_traj", "rank_cov50", "rank_nom50", "rank_cov90", "rank_nom90",
                                     "rank_degenerate")
    assert evaluate.FULLCOV_RANK_FIGURES == tuple("fullcov_" + k for k in evaluate.RANK_FIGURES)
    assert evaluate.MIX_RANK_FIGURES == tuple("mix_" + k for k in evaluate.RANK_FIGURES)
    # refused before any data is read or any launch made
    for k, b, word in ((3, 0, "4 <= K <= 255"), (256, 0, "4 <= K <= 255"), (20, 4, "--rank_bins"),
                       (20, 65, "--rank_bins"), (255, 128, "--rank_bins")):
        a.num_samples, a.rank_bins = k, b
        with pytest.raises(ValueError, match=word):
            evaluate.evaluate_best_of_k(a, None, None, log=lambda s: None)
    # the figures of a result, in the stated order; the hand-made counts of test_bin_edges
    hist = np.full((1, 13, 7), 3, np.int32)
    tot = np.array([[21, 0, 12 * 210, 210]], np.int64)
    sr = ranks.SampleRanks(hist=torch.from_numpy(hist), tot=torch.from_numpy(tot), per_ped=None, k=20, bins=7)
    for prefix, names in (("", evaluate.RANK_FIGURES), ("fullcov_", evaluate.FULLCOV_RANK_FIGURES),
                          ("mix_", evaluate.MIX_RANK_FIGURES)):
        fig = evaluate.rank_figures(sr, prefix)
        assert tuple(fig) == names
        assert fig[prefix + "rank_dev"] == 0.0 and fig[prefix + "rank_mean"] == pytest.approx(0.5)
        assert fig[prefix + "rank_nom50"] == 3 / 7 and fig[prefix + "rank_cov50"] == pytest.approx(3 / 7)
        assert fig[prefix + "rank_nom90"] == 6 / 7 and fig[prefix + "rank_degenerate"] == 0.0
