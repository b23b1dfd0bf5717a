"""CPU: the draw probe's table and reference (tests/draw_cases.py,
tests/draw_ref.py), no GPU.  Every row reaches what it claims, from integers
alone; the reference at a launch's own elements is the existing restatements of
the four samplers, float64 bit for bit; and the straddling rows can tell the
carry into the element's high word from its absence: with the high word held at
its step-0 value every member that straddles moves by far more than the GPU
test's bound."""
import numpy as np
import pytest

from oracle import g2k_ref as ref
from tests import coupled_ref, fullcov_ref, mixture_ref
from tests import draw_cases as dc
from tests import draw_ref as dr

E, L = dc.E, dc.L


@pytest.mark.parametrize("case", dc.CASES, ids=dc.IDS)
def test_rows_reach_what_they_claim(case):
    assert len(case.cols) == len(case.hi0) == len(case.cross) and 1 <= case.Nmax <= 256
    assert all(0 <= n < case.Nmax for n in case.cols) and len(case.cols) <= 64
    for n, hi0, cross in zip(case.cols, case.hi0, case.cross):
        assert dc.first_cross(case.e_scene + n, case.Nmax) == (hi0, cross), n
        last = case.e_scene + n + (L - 1) * case.Nmax
        assert last >> 32 == hi0 + (cross is not None)           # the high word moves at most once, by one
    assert dc.first_cross(case.e_scene, case.Nmax)[1] == case.shared
    # the reference's elements are these integers
    e = dr.elements(case.e_scene, case.cols, case.Nmax)
    assert e.dtype == np.uint64 and [[int(v) for v in r] for r in e] == [
        [case.e_scene + n + t * case.Nmax for t in range(L)] for n in case.cols]


def test_rows_cover_the_branches():
    by = {c.name: c for c in dc.CASES}
    assert by["below"].e_scene + 6 + 11 * 7 == E - 8
    assert by["step0"].e_scene + 3 == E and by["step0"].hi0[3:] == (1,) * 4
    # the coupled head's two sweeps straddle at different steps: members 3..6 against column 0
    for name in ("t1", "t6", "second"):
        assert all(s != by[name].shared for s in by[name].cross[3:]) and by[name].shared is not None
    # members 3..6 straddle, the shared sweep does not; and the reverse
    assert by["t11"].shared is None and by["t11"].cross[3] == 11
    assert by["step0"].shared == 1 and by["step0"].cross[4] is None
    assert by["second"].hi0 == (1,) * 7                            # the carry is hi0 + 1 = 2
    # a straddle at the first step that can have one, at the last, and in between; none at all
    crosses = {s for c in dc.CASES for s in c.cross}
    assert {1, 2, 6, 7, 11, None} <= crosses
    assert dc.STRADDLING == ["t1", "t6", "t11", "step0", "second", "n256", "n1"]
    assert dc.SEEDS == ((7 << 32) + 99, (1 << 64) - 1)


def test_reference_is_the_existing_restatements_bit_for_bit():
    """S 2, F 3, Nmax 7: at e_scene = (s F + f) 12 Nmax the probe's reference is
    gauss_sample, fullcov_ref.sample, mixture_ref.sample (draws and components)
    and coupled_ref.sample of the whole launch, np.array_equal in float64."""
    S, F, N = 2, 3, 7
    rng = np.random.default_rng(501)
    pred = rng.standard_normal((S, F, 2 * L, N)).astype(np.float32)
    cols = list(range(N))
    p = {h: dc.params(h) for h in dr.HEADS}
    for seed in (dc.SEEDS[0], 12345):
        want = {"per_step": ref.gauss_sample(pred, p["per_step"], seed),
                "fullcov": fullcov_ref.sample(pred, p["fullcov"], seed),
                "coupled": coupled_ref.sample(pred, p["coupled"], seed)}
        want["mix"], comp = mixture_ref.sample(pred, p["mix"], seed)
        assert len(np.unique(comp)) == 3                           # every live slot drawn from
        for s in range(S):
            for f in range(F):
                e_scene = (s * F + f) * L * N
                for h in dr.HEADS:
                    got, cm = dr.draw(h, p[h], dr.time_major(pred[s, f]), seed, e_scene, cols, N)
                    assert got.dtype == np.float64
                    if h == "mix":
                        # a component's members of one scene-frame are fewer rows of the product than the
                        # restatement's (the launch's): BLAS may sum them in another order
                        assert np.array_equal(cm, comp[s, f])
                        assert np.abs(got - dr.time_major(want[h][s, f])).max() <= 1e-13, (s, f)
                    else:
                        assert np.array_equal(got, dr.time_major(want[h][s, f])), (h, s, f)
        # the mixture exactly: the launch's members at once, in the restatement's order, so that each
        # component's product has the restatement's rows
        mu = np.concatenate([dr.time_major(pred[s, f]) for s in range(S) for f in range(F)])
        scenes = [(s * F + f) * L * N for s in range(S) for f in range(F) for _ in range(N)]
        got, cm = dr.mix(p["mix"], mu, seed, scenes, cols * (S * F), N)
        assert np.array_equal(cm, comp.reshape(-1))
        assert np.array_equal(got, np.concatenate([dr.time_major(want["mix"][s, f])
                                                   for s in range(S) for f in range(F)]))


@pytest.mark.parametrize("seed", dc.SEEDS, ids=dc.SEED_IDS)
@pytest.mark.parametrize("name", dc.STRADDLING)
def test_rows_tell_the_carry_from_its_absence(name, seed):
    """The draw with the element's high word held at its step-0 value differs
    from the right one by more than 1e-2 (the GPU test's bound is 1e-4 max(1,
    |ref|)) in some coordinate of every member that straddles, and in none of a
    member that does not; for the coupled head, each sweep on its own."""
    case = dc.CASES[dc.IDS.index(name)]
    mu = np.zeros((len(case.cols), 2 * L), np.float32)
    args = (mu, seed, case.e_scene, case.cols, case.Nmax)
    for h in dr.HEADS:
        right, _ = dr.draw(h, dc.params(h), *args)
        wrong, _ = dr.draw(h, dc.params(h), *args, carry=False, **({"shared_carry": True} if h == "coupled" else {}))
        moved = np.abs(right - wrong).max(axis=1)
        for i, cross in enumerate(case.cross):
            if cross is None:
                assert moved[i] == 0.0, (h, i)
            else:
                assert moved[i] > 1e-2, (h, i, moved[i])
                assert np.array_equal(right[i, :2 * cross], wrong[i, :2 * cross])     # the steps before it stand
    right, _ = dr.draw("coupled", dc.params("coupled"), *args)
    wrong, _ = dr.draw("coupled", dc.params("coupled"), *args, carry=True, shared_carry=False)
    moved = np.abs(right - wrong).max(axis=1)
    assert (moved == 0.0).all() if case.shared is None else (moved > 1e-2).all(), moved


def test_the_hash_separates_the_high_words():
    """The same low word under high words 0 and 1: different normals."""
    lo = np.array([5, 1 << 31, (1 << 32) - 1], np.uint64)
    for seed in dc.SEEDS:
        a = np.stack(dr.normals_at(seed, lo))
        b = np.stack(dr.normals_at(seed, lo + np.uint64(E)))
        assert (np.abs(a - b).max(axis=0) > 1e-2).all()
