"""The C-ABI library loads, exports every symbol include/g2k_hip.h declares,
and rejects bad arguments before touching the GPU (runs on CPU)."""
import ctypes
import os
import re

import pytest

from multimodaltraj_2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2k_hip.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(g2k_[a-z0-9_]+)\s*\(", src)))


def test_header_and_binding_agree():
    assert sorted(_lib.SYMBOLS) == declared_functions()


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    for name in declared_functions():
        assert hasattr(lib, name), name
    assert lib.g2k_abi_version() == _lib.ABI_VERSION


def _dims(**kw):
    d = dict(S=2, F=20, T=8, L=12, D=16, H=128, Nmax=32, W=27, stride=1)
    d.update(kw)
    return _lib.G2KDims(**d)


@pytest.mark.parametrize("bad,code", [(dict(T=10), -4), (dict(D=10), -4), (dict(H=96), -4),
                                      (dict(H=384), -4),
                                      (dict(Nmax=0), -1), (dict(Nmax=300), -1), (dict(W=26), -1),
                                      (dict(stride=-1), -1), (dict(S=-1), -1)])
def test_step_rejects_bad_geometry(bad, code):
    lib = _lib.load()
    w = _lib.G2KWeights(*([ctypes.c_void_p(16)] * 7))
    p = ctypes.c_void_p(16)
    rc = lib.g2k_step_fused_f32(ctypes.byref(_dims(**bad)), ctypes.byref(w), p, p, p, p, p, None,
                                None, p, p, p, p, None, None, 5e-4, p, 1 << 30, None)
    assert rc == code
    assert lib.g2k_last_error()


def _split(x):
    return x << _lib.STEP_SPLIT_SHIFT


def test_step_rejects_null_and_sizes_the_split_workspace():
    lib = _lib.load()
    w = _lib.G2KWeights(*([ctypes.c_void_p(16)] * 7))
    p = ctypes.c_void_p(16)
    rc = lib.g2k_step_fused_f32(ctypes.byref(_dims()), ctypes.byref(w), None, p, p, p, p, None,
                                None, p, p, p, p, None, None, 5e-4, p, 1 << 30, None)
    assert rc == -1
    # one workgroup per scene (S >= 256 CUs, or G2K_STEP_SPLIT(1)): every
    # intermediate stays on chip
    assert lib.g2k_step_workspace_bytes(ctypes.byref(_dims(S=256))) == 0
    assert lib.g2k_step_workspace_bytes(ctypes.byref(_dims(flags=_split(1)))) == 0
    # split scenes: one 64-byte ticket line per 16 scenes + [S][X][8] partials
    # (S = 2: automatic X = min(4, 256 / S) = 4; S = 128: X = 2)
    assert lib.g2k_step_workspace_bytes(ctypes.byref(_dims())) == 64 + 2 * 4 * 8 * 4
    assert lib.g2k_step_workspace_bytes(ctypes.byref(_dims(S=128))) == 8 * 64 + 128 * 2 * 8 * 4
    assert lib.g2k_step_workspace_bytes(ctypes.byref(_dims(flags=_split(2)))) == 64 + 2 * 2 * 8 * 4
    assert lib.g2k_step_workspace_bytes(ctypes.byref(_dims(F=1))) == 0     # one frame: X = 1
    assert lib.g2k_step_workspace_bytes(ctypes.byref(_dims(T=9))) == -1
    assert 0 < lib.g2k_step_lds_bytes(ctypes.byref(_dims())) <= 160 * 1024
    # the split must name 0..4 workgroups, and X > 1 needs its workspace
    assert lib.g2k_step_workspace_bytes(ctypes.byref(_dims(flags=_split(5)))) == -1
    rc = lib.g2k_step_fused_f32(ctypes.byref(_dims(flags=_split(5))), ctypes.byref(w), p, p, p, p,
                                p, None, None, p, p, p, p, None, None, 5e-4, p, 1 << 30, None)
    assert rc == -1
    rc = lib.g2k_step_fused_f32(ctypes.byref(_dims()), ctypes.byref(w), p, p, p, p, p, None,
                                None, p, p, p, p, None, None, 5e-4, None, 0, None)
    assert rc == -1 and b"workspace" in lib.g2k_last_error()


def test_other_entry_points_validate():
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    assert lib.g2k_frame_recurrence_f32(ctypes.byref(_dims(H=100)), p, p, 3, None) == -4
    assert lib.g2k_ade_fde_f32(ctypes.byref(_dims(L=10)), p, p, p, None, None, 0, p, None) == -4
    assert lib.g2k_ade_fde_f32(ctypes.byref(_dims()), p, p, p, None, None, 7, p, None) == -1
    assert lib.g2k_infer_rlns_f32(None, p, 4, 4, None) == -1
    assert lib.g2k_eval_rln_ngh_f32(p, p, 4, 0, None) == -1
    assert lib.g2k_step_lds_bytes(ctypes.byref(_dims(T=9))) == 0


def test_zero_scenes_is_a_noop():
    lib = _lib.load()
    w = _lib.G2KWeights(*([ctypes.c_void_p(16)] * 7))
    p = ctypes.c_void_p(16)
    rc = lib.g2k_step_fused_f32(ctypes.byref(_dims(S=0)), ctypes.byref(w), p, p, p, p, p, None,
                                None, p, p, p, p, None, None, 5e-4, p, 0, None)
    assert rc == 0


def test_gridlstm_and_train_entry_points_validate():
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    # g2k_gridlstm_f32(in, ld_in, state, ld_state, W, b, peep, out, state_out, rows, K, fs, u, s)
    assert lib.g2k_gridlstm_f32(None, 16, p, 16, p, p, None, p, p, 4, 4, 4, 2, None) == -1
    assert lib.g2k_gridlstm_f32(p, 15, p, 16, p, p, None, p, p, 4, 4, 4, 2, None) == -1
    assert lib.g2k_gridlstm_f32(p, 16, p, 24, p, p, None, p, p, 4, 4, 4, 3, None) == -4
    # state_out aliases state with a wider pitch
    assert lib.g2k_gridlstm_f32(p, 16, p, 20, p, p, None, p, p, 4, 4, 4, 2, None) == -1
    assert lib.g2k_gridlstm_f32(p, 16, p, 16, p, p, None, p, p, 0, 4, 4, 2, None) == 0
    d = _dims()
    assert lib.g2k_grad_size(ctypes.byref(d)) == 24 * 32 + 496
    need = lib.g2k_grad_workspace_bytes(ctypes.byref(d))
    # one gradient row [P + 2] per workgroup (S X of them, the fused kernel's
    # output), the 64-byte line of the folded update's ticket, then the split
    # workspace (scene tickets, metric partials)
    assert need == 2 * 4 * (24 * 32 + 498) * 4 + 64 + 64 + 2 * 4 * 8 * 4
    one = lib.g2k_grad_workspace_bytes(ctypes.byref(_dims(flags=_split(1))))
    assert one == 2 * (24 * 32 + 498) * 4 + 64
    assert lib.g2k_train_workspace_bytes(ctypes.byref(d)) == need
    w = _lib.G2KWeights(*([p] * 7))
    rc = lib.g2k_step_grad_f32(ctypes.byref(d), ctypes.byref(w), p, p, p, p, p, None, None, 5e-4,
                               p, p, need - 4, None)
    assert rc == -1 and b"workspace" in lib.g2k_last_error()
    rc = lib.g2k_step_grad_f32(ctypes.byref(_dims(T=9)), ctypes.byref(w), p, p, p, p, p, None,
                               None, 5e-4, p, p, need, None)
    assert rc == -4
    assert lib.g2k_update_f32(None, None, p, 10, 0.1, 0.9, 10.0, None) == -1
    # the one-rank fused gradient + update: NULL params, short workspace
    rc = lib.g2k_step_grad_update_f32(ctypes.byref(d), ctypes.byref(w), p, p, p, p, p, None, None,
                                      5e-4, p, p, need, None, None, 5e-3, 0.95, 10.0, None)
    assert rc == -1 and b"params" in lib.g2k_last_error()
    rc = lib.g2k_step_grad_update_f32(ctypes.byref(d), ctypes.byref(w), p, p, p, p, p, None, None,
                                      5e-4, p, p, need - 4, p, None, 5e-3, 0.95, 10.0, None)
    assert rc == -1 and b"workspace" in lib.g2k_last_error()
    assert lib.g2k_update_f32(p, None, p, 0, 0.1, 0.9, 10.0, None) == 0
    # g2k_train_step_f32(d, w, pos, vis, G, tgt, nact, nfr, mask, h_in, h_out, pred, met, lam,
    #                    grad, ws, ws_bytes, params, ms, lr, decay, clip, stream)
    rc = lib.g2k_train_step_f32(ctypes.byref(d), ctypes.byref(w), p, p, p, p, p, None, None, p, p,
                                p, p, 5e-4, p, p, need - 4, None, None, 5e-3, 0.95, 10.0, None)
    assert rc == -1 and b"workspace" in lib.g2k_last_error()
    rc = lib.g2k_train_step_f32(ctypes.byref(d), ctypes.byref(w), p, p, p, p, p, None, None, None,
                                p, p, p, 5e-4, p, p, need, None, None, 5e-3, 0.95, 10.0, None)
    assert rc == -1
    rc = lib.g2k_train_step_f32(ctypes.byref(_dims(H=96)), ctypes.byref(w), p, p, p, p, p, None,
                                None, p, p, p, p, 5e-4, p, p, need, None, None, 5e-3, 0.95, 10.0,
                                None)
    assert rc == -4


def test_small_D_entry_points():
    """D in 1..16 for the class-level forward, the recurrence and the errors
    (sample.py's num_freq_blocks = 10); the fused step needs D = 16."""
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    w = _lib.G2KWeights(*([p] * 7))
    assert lib.g2k_frame_recurrence_f32(ctypes.byref(_dims(D=17)), p, p, 3, None) == -4
    assert lib.g2k_frame_recurrence_f32(ctypes.byref(_dims(D=10, S=0)), p, p, 3, None) == 0
    assert lib.g2k_mcr_forward_f32(ctypes.byref(_dims(D=0)), ctypes.byref(w), p, p, p, p, p, p, p,
                                   5e-4, None) == -4
    assert lib.g2k_mcr_forward_f32(ctypes.byref(_dims(D=10, S=0)), ctypes.byref(w), p, p, p, p, p,
                                   p, p, 5e-4, None) == 0


def test_context_conv_validates():
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    assert lib.g2k_context_conv_workspace_bytes(576, 720, 16) == (576 + 3 - 16) * 256 * 4
    assert lib.g2k_context_conv_workspace_bytes(10, 10, 16) == -1
    assert lib.g2k_context_conv_f32(p, 576, 720, 5, p, 16, 5e-4, p, None, p, 1 << 30, None) == -4
    assert lib.g2k_context_conv_f32(p, 576, 720, 3, p, 16, 5e-4, None, None, p, 1 << 30, None) == -1
    assert lib.g2k_context_conv_f32(p, 576, 720, 3, p, 16, 5e-4, p, None, p, 16, None) == -1


def test_encoder_chain_validates():
    """g2k_encoder_chain_f32 (ABI 8) rejects bad arguments before any device
    call; zero frames are a no-op."""
    lib = _lib.load()
    w = _lib.G2KWeights(*([ctypes.c_void_p(16)] * 7))
    p = ctypes.c_void_p(16)

    def call(d, fs=4, u=2, **null):
        a = dict(X=p, Rel=p, G=p, na=p, nf=p, W=p, b=p, peep=None, Xe=p, cs=p, attn=p, cost=p,
                 pred=p, h=p)
        a.update(null)
        return lib.g2k_encoder_chain_f32(ctypes.byref(d), ctypes.byref(w), a["X"], a["Rel"], a["G"],
                                         a["na"], a["nf"], a["W"], a["b"], a["peep"], fs, u, a["Xe"],
                                         a["cs"], a["attn"], a["cost"], a["pred"], a["h"], 0.0005,
                                         None)
    assert call(_dims(S=0)) == 0                          # nothing to run
    assert call(_dims(F=0)) == 0
    assert call(_dims(H=96)) == -4                        # unsupported hidden size
    assert call(_dims(D=10)) == -4                        # the chain needs D = 16
    assert call(_dims(), fs=4, u=1) == -4                 # feature_size must be 2 num_units
    assert call(_dims(), fs=8, u=3) == -4
    assert call(_dims(), h=None) == -1                    # required buffers
    assert call(_dims(), nf=None) == -1
    assert call(_dims(), h=ctypes.c_void_p(20)) == -1     # h 16-byte aligned
    assert lib.g2k_last_error()


def test_split_sizing_without_a_gpu_is_explicit():
    """ABI 9: the automatic split for a given CU count is host arithmetic
    (g2k_step_split_for_cus, no HIP call), and an explicit split makes the
    workspace size independent of any device (include/g2k_hip.h)."""
    import ctypes

    from multimodaltraj_2_amd import frame_step as fs
    lib = _lib.load()
    assert fs.split_for_cus(256, 20, cus=256) == 1
    assert fs.split_for_cus(128, 20, cus=256) == 2
    assert fs.split_for_cus(128, 20, cus=304) == 2
    assert fs.split_for_cus(64, 20, cus=256) == 4
    assert fs.split_for_cus(16, 20, cus=256) == 4          # at most kMaxSplit
    assert fs.split_for_cus(16, 3, cus=256) == 3           # at most F
    assert fs.split_for_cus(100, 20, cus=80) == 1
    assert fs.split_for_cus(128, 20, split=3, cus=256) == 3          # the request
    assert fs.split_for_cus(128, 20, coresident=True, cus=256) == 1  # launches in flight
    # loop-invariant launches (stride 0, shared targets; L2, Nmax <= 85): one frame's work
    inv = dict(stride=0, targets_shared=True, Nmax=32)
    assert fs.split_for_cus(128, 20, cus=256, **inv) == 1
    assert fs.split_for_cus(128, 20, split=2, cus=256, **inv) == 2          # the request stands
    assert fs.split_for_cus(128, 20, cus=256, stride=0, targets_shared=False, Nmax=32) == 2
    assert fs.split_for_cus(128, 20, cus=256, stride=1, targets_shared=True, Nmax=32) == 2
    assert fs.split_for_cus(128, 20, cus=256, stride=0, targets_shared=True, Nmax=128) == 2
    assert fs.split_for_cus(128, 20, cus=256, loss="nll", **inv) == 2
    d = _lib.G2KDims(128, 20, 8, 12, 16, 128, 32, 27, 1, 0)
    assert lib.g2k_step_split_for_cus(ctypes.byref(d), 0) == -1
    sizes = set()
    for x in (1, 2, 4):
        d = _lib.G2KDims(128, 20, 8, 12, 16, 128, 32, 27, 1, fs.step_flags(split=x))
        nb = lib.g2k_step_workspace_bytes(ctypes.byref(d))
        assert nb == (0 if x == 1 else (128 + 15) // 16 * 64 + 128 * x * 8 * 4)
        sizes.add(nb)
        tb = lib.g2k_train_workspace_bytes(ctypes.byref(d))
        P = lib.g2k_grad_size(ctypes.byref(d))
        assert tb == 128 * x * (P + 2) * 4 + 64 + nb       # one gradient row per workgroup
    assert len(sizes) == 3


def test_step_geometry_validates_and_agrees_with_the_planning_calls():
    """g2k_step_geometry (host arithmetic, no HIP call): rejects what the
    entry points reject, and its split / LDS bytes are g2k_step_split_for_cus's
    and g2k_step_lds_bytes's for the same dims."""
    from multimodaltraj_2_amd import frame_step as fs
    lib = _lib.load()
    out = (ctypes.c_int32 * len(_lib.GEOM_FIELDS))()

    def call(d, train=0, has_h=1, cus=256, o=out):
        return lib.g2k_step_geometry(ctypes.byref(d) if d is not None else None, train, has_h, cus, o)
    assert call(None) == -1
    assert call(_dims(), o=None) == -1
    assert call(_dims(), cus=0) == -1 and b"cus" in lib.g2k_last_error()
    assert call(_dims(stride=-1)) == -1
    assert call(_dims(T=9)) == -4
    assert call(_dims(Nmax=300)) == -1
    assert call(_dims(H=96)) == -4
    assert call(_dims(H=96), train=1, has_h=0) == 0        # gradient only: H is not read
    assert call(_dims(), train=0, has_h=0) == -1           # the forward step needs h_in
    assert call(_dims(flags=_split(5))) == -1
    assert call(_dims(flags=_lib.STEP_LOSS_NLL)) == -4     # a train-mode flag
    assert call(_dims(flags=_lib.STEP_LOSS_NLL), train=1) == 0
    assert call(_dims(flags=_lib.STEP_CORESIDENT), train=1) == -4
    # train mode keeps the whole scene's window-row gradient [(F-1) stride + 8][16] in LDS
    assert call(_dims(stride=200, W=19 * 200 + 8), train=1) == -3
    for S, cus in ((2, 256), (128, 256), (128, 80), (256, 256)):
        d = _dims(S=S)
        assert call(d, cus=cus) == 0
        g = dict(zip(_lib.GEOM_FIELDS, out))
        assert g["split"] == lib.g2k_step_split_for_cus(ctypes.byref(d), cus)
        assert (g["tpw"], g["np"], g["fc"], g["chunks"]) == (2, 12, 20, 1)
        assert g["variant"] == 0 and g["own0"] == 0 and g["dwo_seq"] == 0 and g["ped_major"] == 0
        assert g["lds_bytes"] == lib.g2k_step_lds_bytes(ctypes.byref(_dims(S=S, flags=_split(g["split"]))))
    g = fs.step_geometry(128, 20, 128, 32, train=True, split=2)
    assert (g["variant"], g["np"], g["own0"], g["split"]) == ("blk", 8, 8, 2)
    g = fs.step_geometry(128, 20, 512, 32, train=True, has_h_in=False, loss="nll", pred_layout="ped")
    assert (g["variant"], g["tpw"], g["np"], g["ped_major"]) == ("nll", 1, 8, 1)


def test_best_of_k_geometry_validates():
    """g2k_best_of_k_geometry (added after ABI 11: by symbol; host arithmetic,
    no HIP call): NULL dims / out and the sizes the evaluations reject are
    G2K_EINVAL; out[] is {KS, FC, C} of bestk_geom."""
    lib = _lib.load()
    assert lib.g2k_abi_version() == 11 and _lib.ABI_VERSION == 11
    out = (ctypes.c_int32 * len(_lib.BESTK_GEOM_FIELDS))(-7, -7, -7)

    def call(d, K=20, o=out):
        return lib.g2k_best_of_k_geometry(ctypes.byref(d) if d is not None else None, K, o)
    assert call(None) == -1 and b"dims is NULL" in lib.g2k_last_error()
    assert call(_dims(), o=None) == -1 and b"out is NULL" in lib.g2k_last_error()
    for bad in (dict(S=-1), dict(F=-1), dict(Nmax=0), dict(Nmax=257)):
        assert call(_dims(**bad)) == -1, bad
    for K in (0, -1, 4097):
        assert call(_dims(), K=K) == -1 and b"K=%d " % K in lib.g2k_last_error()
    assert list(out) == [-7, -7, -7]                       # a rejected call writes nothing
    # T, L, D, H and the flags are not looked at
    assert call(_dims(T=9, L=10, D=3, H=5, flags=_lib.STEP_TARGETS_SHARED)) == 0
    assert list(out) == [16, 1, 20]                        # 1280 slots: K = 20 stops KS at 16
    assert call(_dims(S=256)) == 0 and list(out) == [4, 2, 10]
    assert call(_dims(S=0)) == 0 and list(out) == [16, 1, 20]
    assert call(_dims(F=0), K=1) == 0 and list(out) == [1, 1, 1]


def test_loop_invariant_launches_hold_one_ring_slot():
    """Stride 0 with shared targets and one workgroup per scene
    (g2k_scene.hip frames_invariant): the forward forms one head per chunk,
    so its rings hold one slot — a smaller LDS carve-up than the same launch
    with per-frame targets, whose rings hold every frame of the chunk; train
    mode and split launches keep the general layout (host arithmetic, no
    GPU)."""
    from multimodaltraj_2_amd import frame_step as fs
    lib = _lib.load()

    def lds(F, shared, split, coresident=False, stride=0, W=8):
        d = _lib.G2KDims(128, F, 8, 12, 16, 128, 32, W, stride,
                         fs.step_flags(targets_shared=shared, split=split, coresident=coresident))
        return lib.g2k_step_lds_bytes(ctypes.byref(d))

    general, inv = lds(29, False, 1), lds(29, True, 1)
    assert general - inv == (29 - 1) * (16 * 16 + 24 * 8) * 4       # As and M slots
    assert lds(29, False, 1, coresident=True) - lds(29, True, 1, coresident=True) == general - inv
    assert lds(29, True, 2) == lds(29, False, 2)                     # split: general path
    assert lds(20, True, 1, stride=1, W=27) == lds(20, False, 1, stride=1, W=27)
    assert fs.step_coresidency(128, 29, 128, 32, 8, 0, True, True) == 2


# ---------------------------------------------------------------------------
# the probabilistic heads' entry points: every rejection, its status code and
# a distinguishing word of its message; the workspace sizes
# ---------------------------------------------------------------------------
_P = 16                        # a non-NULL pointer, 16-byte aligned (never dereferenced)
_EINVAL, _EUNSUPPORTED = -1, -4


def _err(lib):
    return lib.g2k_last_error() or b""


class _Call:
    """One entry point with named arguments that default to a valid call;
    ``rc(dims, name=value, ...)`` calls it with some replaced (``dims=None``:
    a NULL dims pointer)."""

    def __init__(self, lib, fn, order, **defaults):
        self.lib, self.fn, self.order, self.defaults = lib, getattr(lib, fn), order, defaults

    def rc(self, d, **kw):
        a = dict(self.defaults)
        assert set(kw) <= set(a), kw
        a.update(kw)
        return self.fn(ctypes.byref(d) if d is not None else None, *[a[n] for n in self.order])

    def rejects(self, code, word, d, **kw):
        rc = self.rc(d, **kw)
        msg = _err(self.lib)
        assert rc == code and word in msg, (self.fn.__name__, kw, rc, msg)


_MARGINAL = ("pred", "targets", "n_active", "n_frames", "ped_mask", "head", "seed", "K", "per_ped",
             "best", "out", "ws", "ws_bytes", "stream")
_JOINT = ("pred", "targets", "n_active", "n_frames", "ped_mask", "head", "seed", "K", "radius",
          "per_frame_f", "per_frame_i", "sums_f", "sums_i", "ws", "ws_bytes", "stream")


@pytest.mark.parametrize("fn,short,joint", [
    ("g2k_best_of_k_f32", b"best_of_k", False),
    ("g2k_fullcov_best_of_k_f32", b"fullcov_best_of_k", False),
    ("g2k_joint_eval_f32", b"joint_eval", True),
    ("g2k_fullcov_joint_eval_f32", b"fullcov_joint_eval", True)])
def test_sampled_evaluation_entry_points_validate(fn, short, joint):
    lib = _lib.load()
    d = _dims()
    need = getattr(lib, fn.replace("_f32", "_workspace_bytes"))(ctypes.byref(d))
    assert need > 0
    common = dict(pred=_P, targets=_P, n_active=_P, n_frames=None, ped_mask=None, head=_P, seed=7,
                  K=20, ws=_P, ws_bytes=need, stream=None)
    if joint:
        c = _Call(lib, fn, _JOINT, radius=0.1, per_frame_f=None, per_frame_i=None, sums_f=_P,
                  sums_i=_P, **common)
        required = ("pred", "targets", "n_active", "head", "sums_f", "sums_i")
    else:
        c = _Call(lib, fn, _MARGINAL, per_ped=_P, best=None, out=_P, **common)
        required = ("pred", "targets", "n_active", "head", "out")
    c.rejects(_EINVAL, b"dims is NULL", None)
    c.rejects(_EUNSUPPORTED, short + b" reads pred_path_band", _dims(flags=_lib.STEP_PRED_PED_MAJOR))
    assert _err(lib).startswith(short)
    c.rejects(_EINVAL, b"Nmax=0", _dims(Nmax=0))
    c.rejects(_EINVAL, b"Nmax=257", _dims(Nmax=257))
    c.rejects(_EINVAL, b"S=-1", _dims(S=-1))
    c.rejects(_EINVAL, b"F=-1", _dims(F=-1))
    c.rejects(_EINVAL, b"K=0 ", d, K=0)
    c.rejects(_EINVAL, b"K=4097 ", d, K=4097)
    if joint:
        for r in (-1.0, float("nan"), float("inf")):
            c.rejects(_EINVAL, b"radius=", d, radius=r)
        c.rejects(_EINVAL, b"K=0 ", d, K=0, radius=-1.0)           # K before the radius
        c.rejects(_EINVAL, b"radius=", d, radius=-1.0, pred=None)   # the radius before the pointers
    for name in required:
        c.rejects(_EINVAL, b"required buffer pointer is NULL", d, **{name: None})
    c.rejects(_EINVAL, b"required buffer", d, pred=None, targets=20)   # NULLs before alignment
    c.rejects(_EINVAL, b"targets must be 8-byte aligned", d, targets=20)
    if joint:
        c.rejects(_EINVAL, b"sums_i must be 8-byte aligned", d, sums_i=20)
        c.rejects(_EINVAL, b"targets", d, targets=20, sums_i=20)
        c.rejects(_EINVAL, b"sums_i", d, sums_i=20, ws=None)        # alignment before the workspace
        c.rejects(_EINVAL, b"4-byte aligned", d, ws=18)
        c.rejects(_EINVAL, b"4-byte aligned", _dims(S=0), ws=18, ws_bytes=0)   # ... an empty batch's too
    else:
        c.rejects(_EINVAL, b"per_ped must be 16-byte aligned", d, per_ped=24)
        c.rejects(_EINVAL, b"targets", d, targets=20, per_ped=24)
        c.rejects(_EINVAL, b"per_ped", d, per_ped=24, ws=None)
    c.rejects(_EINVAL, b"workspace of %d bytes needed (got %d)" % (need, need), d, ws=None)
    assert joint or _err(lib).endswith(b"(got %d)" % need)        # the marginal pair asks no alignment
    c.rejects(_EINVAL, b"workspace of %d bytes needed (got %d)" % (need, need - 4), d,
              ws_bytes=need - 4)
    # no scene: nothing to do, and no workspace needed; T and L are not looked at
    assert c.rc(_dims(S=0), ws=None, ws_bytes=0) == 0
    assert c.rc(_dims(S=0, T=9, L=10, D=3, H=5), ws=None, ws_bytes=0) == 0
    c.rejects(_EINVAL, b"K=0 ", _dims(S=0), K=0)                   # S = 0 is still validated
    c.rejects(_EINVAL, b"required buffer", _dims(S=0), head=None)


_STATS = ("pred", "targets", "n_active", "n_frames", "ped_mask", "head", "r2", "n_levels")


@pytest.mark.parametrize("fn,short,head,outs", [
    ("g2k_head_stats_f32", b"head_stats", b"head", ("stats",)),
    ("g2k_fullcov_stats_f32", b"fullcov_stats", b"chol", ("moments", "stats"))])
def test_stats_entry_points_validate(fn, short, head, outs):
    lib = _lib.load()
    size = getattr(lib, fn.replace("_f32", "_workspace_bytes"))
    d = _dims()                                                   # 1280 slots: more than one workgroup
    need = size(ctypes.byref(d), 4)
    assert need > 0 and size(ctypes.byref(_dims(S=1, F=1)), 4) == 0
    order = _STATS + outs + ("inside", "fit", "ws", "ws_bytes", "stream")
    c = _Call(lib, fn, order, pred=_P, targets=_P, n_active=_P, n_frames=None, ped_mask=None,
              head=_P, r2=_P, n_levels=4, inside=_P, fit=_P, ws=_P, ws_bytes=need, stream=None,
              **{o: _P for o in outs})
    c.rejects(_EINVAL, b"dims is NULL", None)
    c.rejects(_EUNSUPPORTED, short + b" reads pred_path_band", _dims(flags=_lib.STEP_PRED_PED_MAJOR))
    assert _err(lib).startswith(short)
    for bad in (dict(Nmax=0), dict(Nmax=257), dict(S=-1), dict(F=-1), dict(S=1 << 16, F=1 << 15)):
        c.rejects(_EINVAL, b"n_levels 0..32, S F < 2^31", _dims(**bad))
        assert size(ctypes.byref(_dims(**bad)), 4) == -1
    c.rejects(_EINVAL, b"n_levels=-1 ", d, n_levels=-1)
    c.rejects(_EINVAL, b"n_levels=33 ", d, n_levels=33)
    assert size(ctypes.byref(d), -1) == -1 and size(ctypes.byref(d), 33) == -1 and size(None, 4) == -1
    for name in ("pred", "targets", "n_active") + outs:
        c.rejects(_EINVAL, b"required buffer pointer is NULL", d, **{name: None})
    c.rejects(_EINVAL, head + b" is NULL: n_levels must be 0 and inside NULL", d, head=None)
    c.rejects(_EINVAL, head + b" is NULL", d, head=None, n_levels=0, r2=None)       # inside given
    c.rejects(_EINVAL, b"r2 is NULL with n_levels=4", d, r2=None)
    c.rejects(_EINVAL, head + b" is NULL", d, head=None, r2=None)                    # head before r2
    c.rejects(_EINVAL, b"targets must be 8-byte aligned", d, targets=20)
    c.rejects(_EINVAL, b"r2 is NULL", d, r2=None, targets=20)                        # r2 before alignment
    words = ", ".join(outs).encode() + b", inside and r2 must be 8-byte aligned"
    for name in outs + ("inside", "r2"):
        c.rejects(_EINVAL, words, d, **{name: 20})
    c.rejects(_EINVAL, b"targets", d, targets=20, stats=20)
    c.rejects(_EINVAL, b"workspace of %d bytes needed (got %d), 8-byte aligned" % (need, need), d,
              ws=None)
    c.rejects(_EINVAL, b"workspace of %d bytes needed (got %d), 8-byte aligned" % (need, need - 4), d,
              ws_bytes=need - 4)
    c.rejects(_EINVAL, b"8-byte aligned", d, ws=20)
    c.rejects(_EINVAL, b"stats", d, stats=20, ws=None)                               # before the workspace
    # one workgroup: no workspace; no scene: nothing to do; T and L are not looked at
    assert c.rc(_dims(S=0), ws=None, ws_bytes=0) == 0
    assert c.rc(_dims(S=0, T=9, L=10, D=3, H=5), ws=None, ws_bytes=0) == 0
    assert c.rc(_dims(S=0), head=None, r2=None, n_levels=0, inside=None, fit=None, ws=None,
                ws_bytes=0) == 0
    c.rejects(_EINVAL, b"required buffer", _dims(S=0), stats=None)


@pytest.mark.parametrize("fn", ["g2k_gauss_sample_f32", "g2k_fullcov_sample_f32"])
def test_sampler_entry_points_validate(fn):
    lib = _lib.load()
    c = _Call(lib, fn, ("pred", "head", "seed", "out", "stream"), pred=_P, head=_P, seed=3, out=_P,
              stream=None)
    c.rejects(_EINVAL, b"dims is NULL", None)
    c.rejects(_EUNSUPPORTED, b"flags must be 0", _dims(flags=_lib.STEP_PRED_PED_MAJOR))
    c.rejects(_EUNSUPPORTED, b"flags must be 0", _dims(flags=_lib.STEP_TARGETS_SHARED))
    c.rejects(_EUNSUPPORTED, b"T=9 L=12", _dims(T=9))
    c.rejects(_EUNSUPPORTED, b"T=8 L=10", _dims(L=10))
    c.rejects(_EINVAL, b"Nmax=0", _dims(Nmax=0))
    c.rejects(_EINVAL, b"Nmax=257", _dims(Nmax=257))
    c.rejects(_EINVAL, b"S=-1", _dims(S=-1))
    c.rejects(_EINVAL, b"F=-1", _dims(F=-1))
    c.rejects(_EINVAL, b"required buffer pointer is NULL", _dims(), pred=None)
    c.rejects(_EINVAL, b"required buffer pointer is NULL", _dims(), head=None)
    c.rejects(_EINVAL, b"out is NULL", _dims(), out=None)
    c.rejects(_EINVAL, b"out is NULL", _dims(S=0), out=None)
    assert c.rc(_dims(S=0)) == 0 and c.rc(_dims(F=0)) == 0


def test_sampled_evaluation_workspace_sizes():
    """The marginal evaluation keeps one row [8] of floats per (scene, frame)
    at most, the joint one a row [10] of int32 per unit: joint_kd_max units per
    scene-frame = as many as bring the launch to 2048 waves (Nmax <= 64) or 512
    workgroups (Nmax > 64), 8 at most.  The two heads share both."""
    lib = _lib.load()

    def sizes(stem, **kw):
        d = ctypes.byref(_dims(**kw))
        a = getattr(lib, "g2k_%s_workspace_bytes" % stem)(d)
        assert getattr(lib, "g2k_fullcov_%s_workspace_bytes" % stem)(d) == a, kw
        return a

    for S, F in [(2, 20), (1, 1), (3, 0), (0, 20), (256, 20), (7, 37)]:
        assert sizes("best_of_k", S=S, F=F) == S * max(F, 1) * 32
    # S F: far below the clamp, the last that still deals 8, the first that
    # deals fewer (2048 / 8 = 256, then ceil(2048 / 293) = 7; 512 / 8 = 64,
    # then ceil(512 / 74) = 7), the last that deals 2, one unit, no frame
    for S, F in [(2, 20), (1, 1), (256, 1), (257, 1), (1, 293), (64, 1), (13, 5), (74, 1),
                 (2047, 1), (2048, 1), (511, 1), (512, 1), (256, 20), (3, 0), (0, 20)]:
        for Nmax, fill in [(32, 2048), (64, 2048), (65, 512), (256, 512)]:
            sf = S * F
            kd = min(8, -(-fill // sf)) if sf > 0 else 1
            assert sizes("joint_eval", S=S, F=F, Nmax=Nmax) == S * max(F, 1) * kd * 40, (S, F, Nmax)
    assert sizes("joint_eval", S=257, F=1, Nmax=32) == 257 * 8 * 40      # the clamp holds here
    assert sizes("joint_eval", S=1, F=293, Nmax=32) == 293 * 7 * 40      # ... and not here
    for stem in ("best_of_k", "joint_eval"):
        for fn in ("g2k_%s_workspace_bytes" % stem, "g2k_fullcov_%s_workspace_bytes" % stem):
            assert getattr(lib, fn)(None) == -1
            assert getattr(lib, fn)(ctypes.byref(_dims(S=-1))) == -1
            assert getattr(lib, fn)(ctypes.byref(_dims(F=-1))) == -1
            assert getattr(lib, fn)(ctypes.byref(_dims(Nmax=0))) >= 0    # Nmax is not looked at
