"""float64 / uint64 restatement of the heads' device-side draw
(csrc/g2k_head_draw.h) at an arbitrary (seed, element): what
tests/probes/head_draw_probe.hip is held against.  The generator is
oracle.g2k_ref.gauss_sample's, formed on explicit 64-bit element indices instead
of an arange over a tensor, so an element may lie at or above 2^32; the heads on
top of it are those of tests/fullcov_ref.py, tests/mixture_ref.py and
tests/coupled_ref.py (tests/test_draw_probe.py: equal to them, float64 bit for
bit, where they can go).

A member is (e_scene, col): e_scene the scene-frame's column-0, step-0 element
((s F + f) 12 Nmax in a launch), col its column; its step-t element is e_scene
+ col + t Nmax.  Means and draws are time-major, [P, 24] with [2t + c].

``carry=False`` holds every element's high word at its sweep's step-0 value:
what a draw that dropped the carry into the high word would make.  Test helper,
not a test module."""
import numpy as np

from oracle import g2k_ref as ref
from tests import fullcov_ref as fr
from tests import mixture_ref as mr
from tests.coupled_ref import SALT

L, DIM = 12, 24
MASK32 = np.uint64(0xFFFFFFFF)
MASK64 = (1 << 64) - 1
HEADS = ("per_step", "fullcov", "mix", "coupled")


def elements(e_scene, cols, Nmax):
    """e [P, 12] uint64: member i's step-t element e_scene + cols[i] + t Nmax
    (``e_scene`` one integer, or one per member: members of several scene-frames)."""
    scenes = [int(v) for v in e_scene] if np.ndim(e_scene) else [int(e_scene)] * len(cols)
    assert len(scenes) == len(cols)
    e0 = [s + int(n) for s, n in zip(scenes, cols)]
    assert all(0 <= v and v + (L - 1) * int(Nmax) < 1 << 63 for v in e0)
    return np.array([[v + t * int(Nmax) for t in range(L)] for v in e0], np.uint64).reshape(len(e0), L)


def stream_key(seed, e, e_hi=None):
    """The element's 32-bit key: pcg(seed_lo ^ pcg(seed_hi ^ (e >> 32))) ^ (uint32)e;
    ``e_hi`` stands in for e >> 32 where given."""
    seed = int(seed) & MASK64
    e = np.asarray(e, np.uint64)
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    e_hi = e >> np.uint64(32) if e_hi is None else np.asarray(e_hi, np.uint64)
    return ref._pcg(lo ^ ref._pcg(hi ^ e_hi)) ^ (e & MASK32)


def normals_at(seed, e, e_hi=None):
    """(e1, e2) float64, each of e's shape: the elements' Box-Muller pairs under
    ``seed``, formed exactly as oracle.g2k_ref.gauss_sample forms them."""
    key = stream_key(seed, e, e_hi)
    h1, h2 = ref._pcg(2 * key + 1), ref._pcg(2 * key + 2)
    u1 = ((h1 >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    u2 = ((h2 >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    rad = np.sqrt(-2 * np.log(u1))
    return rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2)


def sweep_normals(seed, e_scene, cols, Nmax, carry=True):
    """z [P, 24]: z[2t], z[2t + 1] = step t's pair of every member's own sweep."""
    e = elements(e_scene, cols, Nmax)
    e_hi = None if carry else np.broadcast_to(e[:, :1] >> np.uint64(32), e.shape)
    e1, e2 = normals_at(seed, e, e_hi)
    z = np.empty((e.shape[0], DIM))
    z[:, 0::2], z[:, 1::2] = e1, e2
    return z


def per_step(head, mu, seed, e_scene, cols, Nmax, carry=True):
    """PerStepHead::draw: x = mu_x + sigma_x e1, y = mu_y + sigma_y (rho e1 +
    sqrt(1 - rho^2) e2)."""
    head = np.asarray(head, np.float64)
    mu = np.asarray(mu, np.float64)
    z = sweep_normals(seed, e_scene, cols, Nmax, carry)
    e1, e2 = z[:, 0::2], z[:, 1::2]
    sx, sy, rho = np.exp(head[0])[None], np.exp(head[1])[None], np.tanh(head[2])[None]
    out = np.empty_like(mu)
    out[:, 0::2] = mu[:, 0::2] + sx * e1
    out[:, 1::2] = mu[:, 1::2] + sy * (rho * e1 + np.sqrt(1 - rho * rho) * e2)
    return out


def fullcov(chol, mu, seed, e_scene, cols, Nmax, carry=True):
    """FullCovHead::draw: mu + L z."""
    return np.asarray(mu, np.float64) + sweep_normals(seed, e_scene, cols, Nmax, carry) @ fr.lower(chol).T


def mix_components(mix, seed, e_scene, cols):
    """MixHead::select: the first live m with u < cw[m], u from step 0's key
    hashed twice (tests/mixture_ref.selector_u and components)."""
    e0 = elements(e_scene, cols, 1)[:, 0]
    key0 = stream_key(seed, e0)
    h = ref._pcg((ref._pcg(key0) + np.uint64(mr.SEL_SALT)) & MASK32)
    u = ((h >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    assert u.dtype == np.float32
    cw, lv = mr.cum_weights(mix), mr.live(mix)
    comp = np.full(u.shape, np.flatnonzero(lv)[-1], np.int32)
    for m in range(mr.SLOTS - 1, -1, -1):
        if lv[m]:
            comp[u < cw[m]] = m
    return comp


def mix(block, mu, seed, e_scene, cols, Nmax, carry=True):
    """MixHead::draw -> (draws [P, 24], comp [P]): (mu + b_m, one f32 add) + L_m z."""
    block = np.asarray(block, np.float32)
    mu32 = np.asarray(mu, np.float32)
    comp = mix_components(block, seed, e_scene, cols)
    z = sweep_normals(seed, e_scene, cols, Nmax, carry)
    x = np.zeros(z.shape)
    for m in np.flatnonzero(mr.live(block)):
        sel = comp == m
        if not sel.any():
            continue
        a = (mu32[sel] + block[m, mr.OFF_B:mr.OFF_L][None]).astype(np.float64)
        x[sel] = a + z[sel] @ fr.lower(block[m, mr.OFF_L:].reshape(DIM, DIM)).T
    return x, comp


def shared_normals(seed, e_scene, Nmax, carry=True):
    """zc [1, 24] (one per member where e_scene is): the scene-frame's normals,
    column 0's sweep under seed ^ SALT."""
    return sweep_normals((int(seed) & MASK64) ^ SALT, e_scene, [0] * max(1, np.size(e_scene)), Nmax, carry)


def coupled(cpl, mu, seed, e_scene, cols, Nmax, carry=True, shared_carry=None):
    """CoupledHead::draw: mu + Lw z(seed; e0 + t Nmax) + Lb z(seed ^ SALT; e_scene
    + t Nmax); ``shared_carry`` (default: ``carry``) is the shared sweep's."""
    shared_carry = carry if shared_carry is None else shared_carry
    x = sweep_normals(seed, e_scene, cols, Nmax, carry) @ fr.lower(cpl[0]).T \
        + shared_normals(seed, e_scene, Nmax, shared_carry) @ fr.lower(cpl[1]).T
    return np.asarray(mu, np.float64) + x


def draw(which, params, mu, seed, e_scene, cols, Nmax, **kw):
    """-> (draws [P, 24] float64, comp [P] int32 or None) of head ``which``."""
    if which == "mix":
        return mix(params, mu, seed, e_scene, cols, Nmax, **kw)
    fn = {"per_step": per_step, "fullcov": fullcov, "coupled": coupled}[which]
    return fn(params, mu, seed, e_scene, cols, Nmax, **kw), None


def time_major(band):
    """pred[s, f] [24, N] (band layout: x rows, then y rows) -> mu [N, 24]."""
    band = np.asarray(band)
    mu = np.empty((band.shape[1], DIM), band.dtype)
    mu[:, 0::2], mu[:, 1::2] = band[:L].T, band[L:].T
    return mu
