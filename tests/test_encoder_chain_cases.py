"""CPU: the case table of tests/chain_cases.py covers what it claims, and its
inputs can tell a wrong chain kernel from a right one.  No project kernel
runs here: the perturbations below go into the float64 oracle's inputs only.

The bar: in the first frame of every build case's launch the oracle's Xe must
move by at least 1e-2 (100 x the GPU test's 1e-4) under each state- or
input-wiring error a cell could have, so that a kernel with that error cannot
pass.  (From the second frame on h is ~1/H everywhere and says nothing about
the wiring: tests/chain_cases.py.)"""
import numpy as np
import pytest

from multimodaltraj_2_amd import frame_step as fs
from multimodaltraj_2_amd.encoder_step import EncoderChain
from multimodaltraj_2_amd.helper import GridLSTMCell
from tests import chain_cases as cc

D = cc.D
BAR = 1e-2


def test_case_ids_are_unique():
    ids = [c.id for c in cc.CASES]
    assert len(ids) == len(set(ids))
    assert all(c.branch for c in cc.CASES)


def test_every_build_is_covered_with_and_without_peepholes():
    for peep in (True, False):
        assert {(c.H, c.u) for c in cc.BUILD_CASES if c.peep == peep} == cc.BUILDS
    assert len(cc.BUILD_CASES) == 24 and len(cc.BUILDS) == 12
    for c in cc.BUILD_CASES:
        assert (c.S, c.F, c.Nmax) == (6, 3, 17)
        assert c.n_frames == (0, 3, 0, 1, 2, 0) and c.n_active == (5, 17, 9, 0, 1, 3)
        assert c.h0_scale == 1.0 and not c.rel_scale
    # the edges run u 1 and u 4 at H 64 and 512
    for cases in (cc.CLAMP_CASES, cc.NONE_CASES, cc.NAN_CASES, cc.LOGIT_CASES):
        assert {(c.H, c.u) for c in cases} == set(cc.EDGE_BUILDS)
    for nmax in (1, 256):
        assert {(c.H, c.u) for c in cc.NMAX_CASES if c.Nmax == nmax} == set(cc.EDGE_BUILDS)
    assert {c.u for c in cc.REPEAT_CASES} == {1, 2, 4}
    assert cc.WIDE_H0_CASE.h0_scale == 10.0 and cc.WIDE_H0_CASE.frames[0] > 0


def test_sizes_and_frame_patterns_are_covered():
    assert {c.Nmax for c in cc.CASES} == {1, 17, 256}
    # n_active 0, 1 and Nmax on batches that run, at every Nmax above 1
    running = {(c.Nmax, n) for c in cc.CASES for n, nf in zip(c.n_active, c.frames) if nf > 0}
    assert {(17, 0), (17, 1), (17, 17), (1, 1), (256, 256)} <= running
    assert any(c.n_active == (256, 130) for c in cc.NMAX_CASES)
    # the n_frames patterns
    for c in cc.BUILD_CASES:
        nf = c.frames
        assert nf[0] == 0 and nf[-1] == 0 and any(n == 0 for n in nf[1:-1])   # leading, trailing, middle
        assert 1 in nf and any(n >= 3 for n in nf)        # `more` never true; cur 0, 1, 0
        first = next(s for s, n in enumerate(nf) if n > 0)
        assert nf[first + 1] == 0 and any(n > 0 for n in nf[first + 2:])      # pred pending over a skip
        assert any(a > 0 and b > 0 for a, b in zip(nf, nf[1:]))               # ... and over a boundary
    for c in cc.CLAMP_CASES:
        assert c.n_frames == (c.F + 3, -2) and c.frames == (c.F, 0)
        assert cc.clamped_twin(c).n_frames == (c.F, 0)
    for c in cc.NONE_CASES:
        assert not any(c.frames) and cc.reference(c)[1]["state"] is None
    for c in cc.NAN_CASES:
        assert 0 in c.frames and any(0 < n < c.F for n in c.frames)
        assert max(n for n, nf in zip(c.n_active, c.frames) if nf > 0) < c.Nmax
        assert max(cc.wo_twin(c).n_active) == 1


def first_frame(case):
    s = next(i for i, n in enumerate(case.frames) if n > 0)
    inp, _ = cc.reference(case)
    return inp, inp["X"][s, 0, :D].astype(np.float64), inp["h0"][:, :D].astype(np.float64)


@pytest.mark.parametrize("case", cc.BUILD_CASES, ids=lambda c: c.id)
def test_first_frame_tells_a_miswired_cell(case):
    u, K = case.u, case.K
    inp, x, st = first_frame(case)
    base = cc.cell_ref(case, inp, x, st)[0]
    blocks = st.reshape(D, K, 2, u)
    # (a) the c_time / m_time halves of every state block exchanged
    d_a = np.abs(cc.cell_ref(case, inp, x, blocks[:, :, ::-1, :].reshape(D, D))[0] - base).max()
    assert d_a >= BAR, d_a
    # (b) the unit order reversed inside every half
    if u > 1:
        d_b = np.abs(cc.cell_ref(case, inp, x, blocks[:, :, :, ::-1].reshape(D, D))[0] - base).max()
        assert d_b >= BAR, d_b
    # (c) the frequency chain: x block k - 1 zeroed moves output block k
    for k in range(1, K):
        xz = x.copy()
        xz[:, (k - 1) * case.fs:k * case.fs] = 0.0
        out = cc.cell_ref(case, inp, xz, st)[0]
        d_c = np.abs(out - base)[:, 2 * u * k:2 * u * (k + 1)].max()
        assert d_c >= BAR, (k, d_c)
    # and the state itself is O(1): the launch starts from h0 ~ N(0, 1)
    assert 0.5 <= st.std() <= 2.0


@pytest.mark.parametrize("case", cc.LOGIT_CASES, ids=lambda c: c.id)
def test_large_logit_batches_reach_both_paths_of_the_attention_tile(case):
    """Batch 1: the main path at its widest (the widest column spread of its
    frames in [40, 70], every prefix sum above the 1e-30 at which
    attn_tile_wave leaves it).  Batch 2: a prefix sum below 1e-30, the
    fallback's own condition.  Both with two orders of margin, so that the
    float32 rounding of A cannot move a frame across."""
    _, out = cc.reference(case)
    A = out["attn"]
    spread = max(cc.column_spread(A[1, f]) for f in range(case.F))
    assert 40.0 <= spread <= 70.0, spread
    assert min(cc.min_prefix(A[1, f]) for f in range(case.F)) >= 1e-28
    assert min(cc.min_prefix(A[0, f]) for f in range(case.F)) >= 1e-28
    assert all(cc.min_prefix(A[2, f]) <= 1e-32 for f in range(case.F))
    # Rel reaches attn alone: cost and pred stay O(1)
    assert np.abs(out["cost"]).max() < 50 and np.abs(out["pred"]).max() < 500


def test_wide_h0_needs_the_row_max_shift():
    inp, out = cc.reference(cc.WIDE_H0_CASE)
    assert np.abs(inp["h0"]).max() > 30.0          # exp() of the unshifted row would leave ~1e13
    assert np.isfinite(out["h"]).all() and np.isfinite(out["Xe"]).all()


def test_chain_ref_of_a_clamped_launch_is_its_twin():
    c = cc.CLAMP_CASES[0]
    a, b = cc.reference(c)[1], cc.chain_ref(cc.clamped_twin(c))
    for k in ("Xe", "attn", "cost", "pred", "state", "h"):
        assert np.array_equal(a[k], b[k])
    assert a["run"].sum() == c.F


# ---------------------------------------------------------------------------
# EncoderChain's constructor: the cells that map [D, D] to [D, D]
# ---------------------------------------------------------------------------
def cpu_cell(u, fsz, blocks):
    return GridLSTMCell(num_units=u, feature_size=fsz, frequency_skip=fsz, use_peepholes=True,
                        num_frequency_blocks=[blocks], device="cpu")


@pytest.mark.parametrize("u,fsz,blocks", [(1, 2, 8), (2, 4, 4), (4, 8, 2)])
def test_encoder_chain_accepts_the_three_cell_shapes(u, fsz, blocks):
    chain = EncoderChain(fs.init_params(4, seed=0, device="cpu"), cpu_cell(u, fsz, blocks))
    assert chain.cell.num_units == u and chain.cell.output_size == D


@pytest.mark.parametrize("u,fsz", [(2, 2), (1, 4), (4, 4)])
def test_encoder_chain_rejects_cells_that_do_not_map_16_to_16(u, fsz):
    params = fs.init_params(4, seed=0, device="cpu")
    with pytest.raises(ValueError):
        EncoderChain(params, cpu_cell(u, fsz, D // fsz))
