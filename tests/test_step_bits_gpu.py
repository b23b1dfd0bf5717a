"""The scene kernel's output bits stay where tests/golden/step_bits.json has
them: every launch of tests/step_bits_cases.py, the sha256 of the raw bytes
of each output array recomputed and compared (tools/make_step_bits.py wrote
the file with the library of the commit before the recurrence frame, the
frame head and the prediction item loop were re-registered; the same test
passing on that library shows the outputs are deterministic).

Two checks need no GPU: the table covers what it says, and the fallback
case's A, on the float64 oracle, has a column whose leading rows lie more
than 90 below its maximum, so attn_weights' running (max, sum) branch runs.
"""
import json
import os

import numpy as np
import pytest

from oracle import g2k_ref as ref
from tests import step_bits_cases as sb

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_bits.json")
with open(GOLDEN) as _f:
    WANT = json.load(_f)


def test_table_and_golden_agree():
    assert sorted(WANT) == sorted(sb.BY_ID)
    for c in sb.CASES:
        names = {"pred", "h", "metrics"} | ({"A", "cost"} if c.want_attn else set()) \
            | ({"grad"} if c.train else set())
        assert set(WANT[c.id]) == names, c.id
        assert c.S in (3, 4) or c.id == "fixed-frames"
        assert len(c.n_frames or c.n_active) == c.S
        assert all(0 <= n <= c.Nmax for n in c.n_active) and all(
            0 <= f <= c.F for f in c.n_frames or ())
        assert all(col < c.n_active[s] for s, col in c.masked), c.id


def test_table_covers_the_issue():
    C = sb.CASES
    fixed = [c for c in C if c.coresident and c.stride == 1 and c.F == 20 and c.H < 512
             and not c.train and c.split == 0]
    assert any(set(c.n_frames or ()) >= {0, 1, 2, 3, 19, 20} for c in fixed)
    assert {c.H for c in C} >= {64, 128, 256, 512}
    assert {c.H for c in fixed} >= {64, 128, 256}
    for n in (17, 32, 33):
        for layout in ("band", "ped"):
            assert any(c.Nmax == n and c.layout == layout and len(c.masked) == 2 for c in fixed) \
                or n == 32 and layout == "ped"
        seen = set().union(*(c.n_active for c in C if c.Nmax == n))
        assert seen >= {0, 1, 16, 17, n}, (n, seen)
    assert any(c.F == 21 for c in C)
    assert any(c.F == 40 and {32, 33} <= set(c.n_frames) for c in C)
    assert any(c.stride == 0 and c.targets_shared for c in C)
    assert any(c.split == 2 for c in C)
    assert {c.train for c in C} >= {"l2", "nll"}
    assert any(c.fallback for c in C)


def test_fallback_case_reaches_fallback():
    """On the float64 oracle: in every frame that runs, A has a column whose
    four leading rows lie more than 90 below that column's maximum (float32
    exp underflows to zero at -87.4 and flushes at -103.97: the prefix sums of
    those rows are below attn_weights' 1e-30), and a column whose maximum IS
    in the leading rows (the fast path's values are used there)."""
    c = sb.BY_ID["fixed-fallback"]
    b, nfr, mask = sb.inputs(c)
    w = sb.params_for(c).numpy()
    for s in range(c.S):
        _, _, _, ex = ref.scene_step(b.pos[s], b.vislet[s], b.G[s], w, b.targets[s],
                                     c.n_active[s], b.h0[s], n_frames=int(nfr[s]), keep=True)
        assert len(ex["A"]) == nfr[s]
        for A in ex["A"]:
            assert np.all(np.isfinite(A)) and np.abs(A).max() < 1e4
            below = A.max(axis=0) - A[:4].max(axis=0)          # per column
            assert below.max() > sb.FALLBACK_MIN_SPREAD, below.max()
            assert below.min() == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("case", sb.CASES, ids=lambda c: c.id)
def test_step_bits(gpu, case):
    got = sb.run_case(case, gpu)
    assert got == WANT[case.id], {k: (got[k][:12], WANT[case.id].get(k, "")[:12])
                                  for k in got if got[k] != WANT[case.id].get(k)}
