"""GPU: the heads' device-side draw (csrc/g2k_head_draw.h) where a member's
elements straddle 2^32, through tests/probes/head_draw_probe.hip (compiled once
per session by tests/draw_probe.py).  No entry point can be called there — its
pred alone would be 34 GB — so the probe calls Head::draw itself, and three
tests hold it:

1. at a launch's own elements the probe's bits are the library samplers'
   (g2k_gauss_sample_f32, g2k_fullcov_sample_f32, g2k_mix_sample_f32,
   g2k_coupled_sample_f32): what the probe runs is what production runs;
2. on every row of tests/draw_cases.py, at both seeds, each head agrees with the
   float64 reference tests/draw_ref.py under the samplers' own bound, 1e-4
   max(1, |ref|) (tests/test_fullcov_gpu.py, test_mixture_gpu.py,
   test_coupled_head_gpu.py: a wrong stream word moves a normal by O(1)), the
   mixture's components exactly;
3. with unit parameters and zero means a draw is the element's two normals with
   no rounding step of its own, so the four heads — two different codings of
   the straddle — must give equal numbers, and the coupled head's shared sweep
   the per-step head's draw of column 0 under the salted seed.

Measured worst error over the bound in 2: per-step 0.0143, full covariance
0.0161, mixture 0.0164, coupled 0.0120 ("The draw streams' 2^32
boundaries as a tested table")."""
import ctypes

import numpy as np
import pytest
import torch

from tests import draw_cases as dc
from tests import draw_probe
from tests import draw_ref as dr
from tests.abi_arena import Arena, all_written
from tests.conftest import close
from tests.coupled_ref import SALT

pytestmark = pytest.mark.gpu
TOL = 1e-4                      # the heads' sampler tests' bound
L = dc.L


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _library_sample(which, pred, params, seed, dev):
    """The library sampler's draw of ``pred`` [S, F, 24, N] -> (out, comp or None), host arrays."""
    from multimodaltraj_2_amd import _lib, coupled, mixture
    S, F, _, N = pred.shape
    d = _lib.G2KDims(S, F, 8, 12, 16, 64, N, 8, 0)
    ar = Arena(dev)
    p, q = ar.put(pred, "pred"), ar.put(np.ascontiguousarray(params, np.float32), "params")
    out = ar.alloc(pred.shape, name="out")
    comp = ar.alloc((S, F, N), torch.int32, "comp") if which == "mix" else None
    sd = ctypes.c_uint64(seed)
    if which == "per_step":
        rc = _lib.load().g2k_gauss_sample_f32(ctypes.byref(d), p.data_ptr(), q.data_ptr(), sd, out.data_ptr(), None)
    elif which == "fullcov":
        rc = _lib.load().g2k_fullcov_sample_f32(ctypes.byref(d), p.data_ptr(), q.data_ptr(), sd, out.data_ptr(),
                                                None)
    elif which == "mix":
        rc = mixture.load().g2k_mix_sample_f32(ctypes.byref(d), p.data_ptr(), q.data_ptr(), sd, out.data_ptr(),
                                               comp.data_ptr(), None)
    else:
        rc = coupled.load().g2k_coupled_sample_f32(ctypes.byref(d), p.data_ptr(), q.data_ptr(), sd, out.data_ptr(),
                                                   None)
    assert rc == 0, (which, rc)
    torch.cuda.synchronize()
    ar.check_guards()
    assert all_written(out)
    return out.cpu().numpy(), None if comp is None else comp.cpu().numpy()


@pytest.mark.parametrize("which", dr.HEADS)
def test_probe_is_the_library_sampler_bit_for_bit(gpu, which):
    """S 2, F 3, Nmax 7, every scene-frame: the probe at e_scene = (s F + f) 12
    Nmax with every column and the scene-frame's means."""
    S, F, N = 2, 3, 7
    pred = np.random.default_rng(502).standard_normal((S, F, 2 * L, N)).astype(np.float32)
    params = dc.params(which)
    for seed in (dc.SEEDS[0], dc.SEEDS[1]):
        want, wcomp = _library_sample(which, pred, params, seed, gpu)
        for s in range(S):
            for f in range(F):
                got, comp = draw_probe.run(which, params, dr.time_major(pred[s, f]), seed, (s * F + f) * L * N,
                                           list(range(N)), N, gpu)
                assert np.array_equal(_bits(got), _bits(dr.time_major(want[s, f]))), (seed, s, f)
                if which == "mix":
                    assert np.array_equal(comp, wcomp[s, f])
        if which == "mix":
            assert len(np.unique(wcomp)) == 3


_WORST = {}


@pytest.mark.parametrize("seed", dc.SEEDS, ids=dc.SEED_IDS)
@pytest.mark.parametrize("case", dc.CASES, ids=dc.IDS)
def test_probe_matches_reference(gpu, case, seed):
    mu = np.random.default_rng(600 + dc.IDS.index(case.name)).standard_normal(
        (len(case.cols), 2 * L)).astype(np.float32)
    errs = {}
    for which in dr.HEADS:
        params = dc.params(which)
        got, comp = draw_probe.run(which, params, mu, seed, case.e_scene, case.cols, case.Nmax, gpu)
        want, wcomp = dr.draw(which, params, mu, seed, case.e_scene, case.cols, case.Nmax)
        errs[which] = close(got, want)
        _WORST[which] = max(_WORST.get(which, 0.0), errs[which] / TOL)
        if which == "mix":
            assert np.array_equal(comp, wcomp), (comp, wcomp)
    print(f"case {case.name} seed {seed:#x}: " + ", ".join(
        f"{h} err / bound {errs[h] / TOL:.3g} (worst so far {_WORST[h]:.3g})" for h in dr.HEADS))
    for which in dr.HEADS:
        assert np.isfinite(errs[which]) and errs[which] <= TOL, (which, errs[which])


@pytest.mark.parametrize("seed", dc.SEEDS, ids=dc.SEED_IDS)
@pytest.mark.parametrize("case", dc.CASES, ids=dc.IDS)
def test_the_straddle_codings_agree_exactly(gpu, case, seed):
    """Unit parameters, mu = 0: every head's output is the element's normals
    (fmaf(1, z, 0) and fmaf(0, z, a) are exact), so PerStepHead's 64-bit element
    per step and the other three heads' 32-bit carry test must give equal
    numbers, the controls ``below`` and ``above`` included; and with cpl = {0, I}
    every member is the shared sweep: the per-step draw of column 0 under seed ^
    G2K_COUPLED_SALT."""
    P = len(case.cols)
    mu = np.zeros((P, 2 * L), np.float32)
    out = {h: draw_probe.run(h, dc.unit_params(h), mu, seed, case.e_scene, case.cols, case.Nmax, gpu)[0]
           for h in dr.HEADS}
    z = dr.sweep_normals(seed, case.e_scene, case.cols, case.Nmax)
    assert close(out["per_step"], z) <= TOL                      # normals, not zeros
    for h in dr.HEADS[1:]:
        assert np.array_equal(out[h], out["per_step"]), h
    eye = np.eye(2 * L, dtype=np.float32)
    shared = draw_probe.run("coupled", np.stack([np.zeros_like(eye), eye]), mu, seed, case.e_scene, case.cols,
                            case.Nmax, gpu)[0]
    col0 = draw_probe.run("per_step", dc.unit_params("per_step"), mu[:1], seed ^ SALT, case.e_scene, [0],
                          case.Nmax, gpu)[0]
    assert close(col0, dr.shared_normals(seed, case.e_scene, case.Nmax)) <= TOL
    for i in range(P):
        assert np.array_equal(shared[i], col0[0]), i
