"""The drawn-once sampled evaluations share one launch geometry
(csrc/g2k_drawn.h: drawn_geom): sample_scores, sample_ranks and sample_kin
report the same g, lanes, fc, c for the same shapes, sample_modes the same
with its own cap 64 // M on the pairs of a pass, and all of them what the
header's arithmetic says.  Host arithmetic only: no GPU."""
import itertools

from multimodaltraj_2_amd import kin, modes, ranks, scores

SHAPES = list(itertools.product((1, 3), (0, 1, 3, 20), (1, 16, 33, 256)))   # S, F, Nmax
KS = (4, 7, 8, 9, 20, 64, 255)       # in every family's range
MS = (1, 2, 3, 4, 5, 8, 20, 32)
SHARED = ("g", "lanes", "fc", "c")


def _expected(F, Nmax, K, cap=32):
    """drawn_geom, restated: 256 lanes, at most `cap` pairs and 4 passes."""
    g = min(256 // K, cap)
    fc = max(min(4 * g // Nmax, F), 1)
    return dict(g=g, lanes=K, fc=fc, c=-(-F // fc) if F > 0 else 1)


def _shared(geo):
    return {f: geo[f] for f in SHARED}


def test_one_geometry_field_list():
    assert scores.GEOM_FIELDS == modes.GEOM_FIELDS == ranks.GEOM_FIELDS == kin.GEOM_FIELDS
    assert scores.GEOM_FIELDS[:4] == SHARED


def test_scores_ranks_kin_agree():
    for (S, F, Nmax), K in itertools.product(SHAPES, KS):
        want = _expected(F, Nmax, K)
        for fn in (kin.sample_kin_geometry, ranks.sample_ranks_geometry, scores.sample_scores_geometry):
            assert _shared(fn(S, F, Nmax, K)) == want, (fn.__name__, S, F, Nmax, K)


def test_modes_agrees_up_to_its_cap():
    seen_capped = False
    for (S, F, Nmax), K, M in itertools.product(SHAPES, KS, MS):
        if M > K:
            continue
        got = _shared(modes.sample_modes_geometry(S, F, Nmax, K, M))
        if M <= 2:      # 64 // M >= 32: the family's own cap binds first
            assert got == _shared(scores.sample_scores_geometry(S, F, Nmax, K)), (S, F, Nmax, K, M)
        assert got["g"] == min(256 // K, 64 // M, 32), (S, F, Nmax, K, M)
        assert got == _expected(F, Nmax, K, cap=min(64 // M, 32)), (S, F, Nmax, K, M)
        seen_capped |= got["g"] == 64 // M < min(256 // K, 32)
    assert seen_capped          # the sweep reaches the branch where 64 // M binds
