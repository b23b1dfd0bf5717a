"""The inputs of the scene-rank tests (tests/test_scene_ranks.py checks every
geometry claim below on the CPU; tests/test_scene_ranks_gpu.py runs the kernels
on them): the smallest shapes that reach each path of scene_ranks_kernel's
geometry (csrc/g2k_scene_ranks.hip).  One workgroup owns a scene-frame and
walks its P compacted members in tiles of TM = 16 (K <= 31) or 8 (K >= 32); the
K + 1 items of a tile are made 256 / TM to a round; the K (K + 1) / 2 pair sums
are dealt to the 256 lanes, APT = ceil(K (K + 1) / 512) to a lane at most, the
25 (K + 1) residual sums AFT = ceil(25 (K + 1) / 256).  Head parameters as
tests/couples_cases.py, the scene-coupled head's block as
tests/coupled_cases.py; columns >= n_active, masked columns and frames >=
n_frames hold NaN, as do the factors above their diagonals.

Case k2 has four scenes, not two: the members of a scene are the same in every
frame it has (n_active and ped_mask are per scene), so P of 0, 1, 2 and 8 in
one launch takes four scenes.  Test helper, not a test module."""
import functools

import numpy as np

from tests import coupled_cases as cx
from tests import coupled_ref
from tests import fullcov_ref
from tests import mix_eval_ref as me
from tests.bestk_ref import MASK64, draw_seed, pair_mask
from tests.ranks_cases import SEED, sampler as _sampler

L = 12
HEADS = ("per_step", "fullcov", "mix", "coupled")

#  name      S  F  Nmax K   B   members per scene           n_frames   shared  tm  what it reaches
CASES = [
    # the minimum K (3 items, 3 pairs); P = 8, 2, 1 and 0; an empty scene; n_frames < F
    ("k2",     4, 2, 8,   2,  3,  [8, 2, 1, 0],               [2, 1, 2, 0], False, 16),
    # the evaluation's K (210 pairs: one a lane, 46 lanes without); masked columns; P = 27 (two tiles, a
    # partial last one), 17 (one more than a tile) and 16 (one full tile); n_frames < F
    ("k20",    3, 3, 32,  20, 7,  [27, 17, 16],               [3, 2, 1],    False, 16),
    # the maximum K: 8-member tiles, 2080 pairs (9 to a lane at most, the last round partial), 1625
    # sums (7 to a lane); P = 40: five full tiles
    ("k64",    1, 2, 40,  64, 13, [40],                       None,         False, 8),
    # dense: P = 256, sixteen tiles
    ("n256",   1, 1, 256, 5,  6,  [256],                      None,         False, 16),
    # G2K_STEP_TARGETS_SHARED on k20's shape
    ("shared", 3, 3, 32,  20, 7,  [27, 17, 16],               [3, 2, 1],    True,  16),
    # either side of the tile height's K boundary: the largest K with 16-member tiles (32 items: 512 of
    # the 520 slots), P one more than a tile; the smallest with 8-member tiles, P one more than a tile
    ("k31",    1, 1, 24,  31, 8,  [17],                       None,         False, 16),
    ("k32",    1, 2, 24,  32, 11, [9],                        None,         False, 8),
]
IDS = [c[0] for c in CASES]
# The rows run at the boundary seeds (tests/bestk_ref.BOUNDARY_SEEDS: draw 1's seed carries out of the low
# word), per (seed, head): k2, the smallest.  At W the coupled head's nine ranks of k2 (K = 2: each one of
# 0, 1, 2) happen to be the same with the carry dropped, so the integer outputs could not tell; that
# combination takes the next-smallest row, k20.
BOUNDARY = [(at, w, "k20" if (at, w) == ("W", "coupled") else "k2") for at in ("A", "W") for w in HEADS]
BOUNDARY_IDS = [f"{at}-{row}-{w}" for at, w, row in BOUNDARY]


def geometry(N, K):
    """What g2k_scene_ranks_geometry must report for Nmax = N and K."""
    tm = 16 if K <= 31 else 8
    pairs = K * (K + 1) // 2
    return dict(tm=tm, dr=256 // tm, tiles=-(-N // tm), w=1, pairs=pairs, apt=-(-pairs // 256),
                aft=-(-25 * (K + 1) // 256), lds_bytes=520 * 28 * 4 + 16 * 28 * 4 + 256 * 4 + 16)


@functools.lru_cache(maxsize=None)
def inputs(i):
    """Case i -> dict(pred, targets, head [3, 12], chol [24, 24], mix [8, 608],
    cpl [2, 24, 24], n_active, n_frames, ped_mask, members [S, F, N], K, B,
    seed, shared, tm), float32 / int32 / uint8 host arrays."""
    _, S, F, N, K, B, nmem, nfr, shared, tm = CASES[i]
    rng = np.random.default_rng(8400 + i)
    sx, sy = rng.uniform(0.1, 1.5, L), rng.uniform(0.1, 1.5, L)
    rho = rng.uniform(-0.9, 0.9, L)
    head = np.stack([np.log(sx), np.log(sy), np.arctanh(rho)]).astype(np.float32)
    Bf = fullcov_ref.block_factor(head)
    T = 0.7 ** np.abs(np.subtract.outer(np.arange(L), np.arange(L)))
    chol = np.linalg.cholesky(Bf @ np.kron(T, np.eye(2)) @ Bf.T).astype(np.float32)
    w = rng.uniform(0.2, 1.0, 3)
    bs = 1.5 * rng.standard_normal((3, 2 * L))
    mix = me.make_block(w, bs, [chol] * 3, me.SLOTS3)
    Lw, Lb = cx.factors(chol, i % 2 == 1, np.random.default_rng(9400 + i))
    cpl = np.stack([Lw, Lb]).astype(np.float32)
    up = np.triu_indices(2 * L, 1)
    cpl[:, up[0], up[1]] = np.nan
    chol_nan = chol.copy()
    chol_nan[up] = np.nan
    pred = rng.standard_normal((S, F, 2 * L, N)).astype(np.float32)
    Ft = 1 if shared else F
    mu = pred[:, :Ft].reshape(S, Ft, 2, L, N).transpose(0, 1, 4, 3, 2)        # [S, Ft, N, L, 2]
    sig = np.stack([sx, sy], axis=-1)
    tg = (mu + sig * rng.standard_normal((S, Ft, N, L, 2))).astype(np.float32)
    # the members: every case but the plain ones masks columns out below n_active
    n_active = np.zeros(S, np.int32)
    pm = np.ones((S, N), np.uint8)
    masked = IDS[i] in ("k20", "shared")
    for s, P in enumerate(nmem):
        out = min(3, N - P) if masked else 0                                  # masked-out columns below n_active
        n_active[s] = P + out
        if out:
            pm[s, rng.choice(np.arange(1, P + out), out, replace=False)] = 0
        pm[s, n_active[s]:] = rng.integers(0, 2, N - n_active[s])             # beyond n_active: anything
    if not masked:
        pm = None
    n_frames = None if nfr is None else np.array(nfr, np.int32)
    members = pair_mask(S, F, N, n_active, n_frames, pm)
    assert [int(m.sum(axis=1).max()) for m in members] == list(nmem)
    pred[~np.broadcast_to(members[:, :, None, :], pred.shape)] = np.nan       # never read: poison
    tg[~np.broadcast_to(members.any(axis=1)[:, None, :, None, None] if shared
                        else members[:, :, :, None, None], tg.shape)] = np.nan
    return dict(pred=pred, targets=np.ascontiguousarray(tg), head=head, chol=chol_nan, mix=mix, cpl=cpl,
                n_active=n_active, n_frames=n_frames, ped_mask=pm, members=members, K=K, B=B,
                seed=SEED + 70 + i, shared=shared, tm=tm)


def sampler(which, c):
    """(pred, seed) -> one joint draw [S, F, 24, N] of head ``which``: the
    checkers' restatement of the head's sampler."""
    if which == "coupled":
        return lambda pred, seed: coupled_ref.sample(pred, c["cpl"], seed & MASK64)
    return _sampler(which, c)


@functools.lru_cache(maxsize=None)
def oracle_draws(i, which, seed=None, carry=True):
    """[K, S, F, 24, N] float32: the restated sampler's draws for seeds seed +
    k (``seed`` None: the case's own), rounded to the sampler's fp32;
    ``carry=False``: tests/bestk_ref.draw_seed's."""
    c = inputs(i)
    draw = sampler(which, c)
    seed = c["seed"] if seed is None else seed
    with np.errstate(invalid="ignore"):
        d = [draw(c["pred"], draw_seed(seed, k, carry)) for k in range(c["K"])]
    return np.stack(d).astype(np.float32)


# ---------------------------------------------------------------------------
# the property: what the figures are for
# ---------------------------------------------------------------------------
PROP = dict(S=64, F=8, N=16, K=20, B=7, seed=4242, sigma=0.5, share=0.8, side=4.0, fit_seed=77, score_seed=78)


def property_n_active():
    """n_active [S] spread over 2..16."""
    return (2 + np.arange(PROP["S"]) % 15).astype(np.int32)


def property_check(score, label=""):
    """``score(kind)`` -> scene_ranks_ref.figures-like dict of the scoring
    targets under the K joint draws of the "coupled" head fitted on the other
    set and of the "fullcov" head fitted on the same data.  The thresholds sit
    between the calibrated and the independent law's figures (dev 0.03..0.08
    against 0.84, pit 0.49..0.52 against 0.97 / 0.024, typ dev against
    0.29..0.37) with a margin of about 1.5 on each side."""
    co, fc = score("coupled"), score("fullcov")
    for kind, v in (("coupled", co), ("fullcov", fc)):
        print(f"{label}{kind}: frames {v['frames']} es {v['es']:.4f} " + ", ".join(
            f"{g} dev {v[g]['dev']:.4f} pit {v[g]['pit']:.4f}" for g in ("typ", "loc", "spr")))
    for g in ("typ", "loc", "spr"):
        assert co[g]["dev"] <= 0.12, (g, co[g])
        assert 0.44 <= co[g]["pit"] <= 0.56, (g, co[g])
    assert fc["loc"]["dev"] >= 0.6 and fc["spr"]["dev"] >= 0.6
    assert fc["loc"]["pit"] >= 0.9 and fc["spr"]["pit"] <= 0.1 and fc["typ"]["dev"] >= 0.2
