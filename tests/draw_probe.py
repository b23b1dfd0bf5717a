"""TEST INFRASTRUCTURE ONLY — builds and binds tests/probes/head_draw_probe.hip:
the heads' device-side draw (csrc/g2k_head_draw.h) at an arbitrary (seed,
element).  The probe is one translation unit compiled with the library's own
compiler and flags (multimodaltraj_2_amd.build), once per test session, into a
temporary directory that is removed at exit; it is not part of the library.  A
compile that fails raises: a test that got as far as asking for the probe has a
GPU, so that is an error, not a skip.  Test helper, not a test module."""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

from tests import draw_ref as dr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "probes", "head_draw_probe.hip")
WHICH = {h: i for i, h in enumerate(dr.HEADS)}
_vp = ctypes.c_void_p
_lib = None


def command(out):
    from multimodaltraj_2_amd import build
    return [build.HIPCC, *build.FLAGS, "-I" + build.CSRC, "-shared", "-o", out, SRC]


def load():
    """Compile (once per process) and return the ctypes handle."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401  (one HIP runtime per process, as multimodaltraj_2_amd._lib.load)
        tmp = tempfile.mkdtemp(prefix="g2k_draw_probe_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        out = os.path.join(tmp, "libhead_draw_probe.so")
        r = subprocess.run(command(out), capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"the draw probe does not compile:\n{' '.join(command(out))}\n{r.stderr}")
        lib = ctypes.CDLL(out)
        lib.head_draw_probe.restype = ctypes.c_int
        lib.head_draw_probe.argtypes = [ctypes.c_int, _vp, _vp, ctypes.c_uint64, ctypes.c_int64, _vp,
                                        ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]
        _lib = lib
    return _lib


def run(which, params, mu, seed, e_scene, cols, Nmax, device):
    """One launch -> (out [P, 24] float32, comp [P] int32 or None (the mixture
    head's), host arrays).  Every buffer is a guarded, poisoned
    tests/abi_arena.Arena block: the guards must stand, and out (and comp) must
    be written for every i < P."""
    import torch

    from tests.abi_arena import Arena, all_written
    lib = load()
    P = len(cols)
    mu = np.ascontiguousarray(mu, np.float32)
    assert mu.shape == (P, dr.DIM) and all(0 <= int(n) < Nmax for n in cols)
    ar = Arena(device)
    d_params = ar.put(np.ascontiguousarray(params, np.float32), "params")
    d_mu = ar.put(mu, "mu")
    d_cols = ar.put(np.asarray(cols, np.int32), "cols")
    out = ar.alloc((P, dr.DIM), name="out")
    comp = ar.alloc((P,), torch.int32, "comp") if which == "mix" else None
    rc = lib.head_draw_probe(WHICH[which], d_params.data_ptr(), d_mu.data_ptr(),
                             ctypes.c_uint64(int(seed) & dr.MASK64), ctypes.c_int64(int(e_scene)),
                             d_cols.data_ptr(), int(Nmax), P, out.data_ptr(),
                             None if comp is None else comp.data_ptr(), None)
    assert rc == 0, f"head_draw_probe({which}) returned {rc}"
    torch.cuda.synchronize()
    ar.check_guards()
    assert all_written(out) and (comp is None or all_written(comp))
    return out.cpu().numpy(), None if comp is None else comp.cpu().numpy()
