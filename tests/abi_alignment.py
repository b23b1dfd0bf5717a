"""The pointer alignment every entry point of include/g2k_hip.h,
include/g2k_mix.h and include/g2k_scores.h accepts, as
data (tests/test_abi_alignment.py drives the validators with it on the CPU,
tests/test_abi_alignment_gpu.py runs every entry point at exactly these
minima against its 16-byte-aligned twin and the float64 oracle).

One ``Entry`` per entry point that takes device pointers, its parameters in
call order; one ``Arg`` per pointer, outputs and workspaces included, with the
minimum alignment in bytes the library accepts and ONE of three states:

  "a"  validated: the kernel needs (or the ABI has always asked) more than the
       element type's natural alignment and the validator returns G2K_EINVAL
       for less; ``where`` quotes the check;
  "b"  handled: the kernel branches on the pointer's alignment and has a path
       for the weaker case; ``where`` quotes the branch;
  "c"  natural: every access through the pointer is of the element's own
       width (4-byte loads, stores and LDS-DMA for fp32 / int32, bytes for the
       masks, 8 bytes for double / int64); nothing to validate.

A pointer below its element type's natural alignment is the caller's contract
everywhere (include/g2k_hip.h, conventions) and is never passed by a test,
except to a validator that is there to reject it: a ``void*`` workspace has no
natural alignment, so its "a" row is the only statement about it.

``where`` = (source file under csrc/, text of the check or branch); the text
is searched for, not a line number, so the row survives edits above it and
fails (test_every_quoted_check_is_in_the_source) when the check itself goes.
``cond`` = (label, dims that select the case, minimum, state, where): the
requirement under a condition on the dims, e.g. 16 when D == 16, else 4.
A claim is what the header that declares the entry point promises; it is never
edited to follow the library.

``accept``: how a call whose every pointer sits at its minimum shows that it
was accepted without any HIP call being reached with the made-up pointers:
"ok" = an empty batch returns G2K_OK; "size" = the entry point has no
HIP-free success (it zero-fills an output even for an empty batch), so the
call carries workspace_bytes = 0 and must get past every alignment check to
the size check that follows them ("... bytes needed").
"""
from __future__ import annotations

from dataclasses import dataclass, field

ABI, DATA, SCENE = "g2k_abi.hip", "g2k_data.hip", "g2k_scene.hip"
# the sampled evaluations' entry points are in the files of their kernels; the
# checks that their validators share are in one header
CHECKS, JOINT = "g2k_checks.h", "g2k_joint.hip"
ELEM_BYTES = {"f32": 4, "i32": 4, "u8": 1, "f64": 8, "i64": 8, "void": 1}

# the three alignment-dependent branches of the scene kernel
WIDE = (SCENE, "wide = (Nmax & 1) == 0 && (((uintptr_t)a.pos) & 15) == 0")
SEG = (SCENE, "if (((((uintptr_t)src) | lds_addr(dst)) & 15) == 0 && (n & 3) == 0)")
MASK = (SCENE, "(a.d.Nmax & 3) == 0 && (((uintptr_t)a.ped_mask) & 3) == 0")
# the validators' checks
TGT16 = (ABI, '!aligned16(targets)) return set_err(G2K_EINVAL, "targets must be 16-byte aligned")')
TGT8 = (ABI, '(((uintptr_t)targets) & 7) return set_err(G2K_EINVAL, "targets must be 8-byte aligned")')
POS8 = (ABI, '(((uintptr_t)pos & 7u) != 0) return set_err(G2K_EINVAL, "pos must be 8-byte aligned")')
H16 = (ABI, "if (!aligned16(h_in) || !aligned16(h_out))")
PRED16 = (ABI, "if ((d->flags & G2K_STEP_PRED_PED_MAJOR) && !aligned16(pred))")
WS4 = (ABI, "if (workspace && !aligned4(workspace))")
REC16 = (ABI, "if (d->D == kD && (!aligned16(A) || !aligned16(h)))")
CHAIN16 = (ABI, "if (!aligned16(h) || !aligned16(attn))")
SUMSI8 = (JOINT, 'if (((uintptr_t)sums_i) & 7) return set_err(G2K_EINVAL, "sums_i must be 8-byte aligned");')
DBL8 = (ABI, "if ((((uintptr_t)moments) | ((uintptr_t)stats) | ((uintptr_t)inside) | ((uintptr_t)r2)) & 7)")
STWS8 = (ABI, "if (workspace && (((uintptr_t)workspace) & 7))")
GATHER8 = (DATA, "if (((uintptr_t)xy & 7u) || ((uintptr_t)pos & 7u) || ((uintptr_t)targets & 7u))")
# g2k_mix_em_f32's own (each quote runs into a neighbouring line that only that
# entry point has, so the validators with the same check do not stand in for it)
EM_TGT8 = (ABI, 'if (!r.p) return set_err(G2K_EINVAL, "%s is NULL", r.name);\n'
                '  if (((uintptr_t)targets) & 7) return set_err(G2K_EINVAL, "targets must be 8-byte aligned");')
EM_DBL8 = (ABI, "if ((((uintptr_t)moments) | ((uintptr_t)resp) | ((uintptr_t)total)) & 7)")
EM_WS8 = (ABI, 'if (workspace && (((uintptr_t)workspace) & 7))\n'
               '    return set_err(G2K_EINVAL, "workspace must be 8-byte aligned");\n'
               "  const int64_t need = mix_em_ws_bytes(d);")
# the validators of the sampled evaluations (best-of-K, joint, KDE-NLL, scores):
# check_targets, check_per_ped and check_workspace, which each of them calls
# with the bytes of its rows' element (4: floats or int32)
S_TGT8 = (CHECKS, 'if (((uintptr_t)targets) & 7) return set_err(G2K_EINVAL, "targets must be 8-byte aligned");')
PERPED16 = (CHECKS, 'if (((uintptr_t)per_ped) & 15) return set_err(G2K_EINVAL, "per_ped must be 16-byte aligned");')
BK_WS4 = ("g2k_bestk.hip", "check_workspace(d, workspace, workspace_bytes, best_of_k_ws_bytes(d), 4)")
KDE_WS4 = ("g2k_kde.hip", "check_workspace(d, workspace, workspace_bytes, kde_nll_ws_bytes(d), 4)")
JT_WS4 = (JOINT, "check_workspace(d, workspace, workspace_bytes, joint_eval_ws_bytes(d), 4,")
SC_WS4 = ("g2k_scores.hip", "check_workspace(d, workspace, workspace_bytes, scores_ws_bytes(d), 4)")


@dataclass(frozen=True)
class Arg:
    name: str
    elem: str                      # ELEM_BYTES key
    min: int                       # bytes
    state: str                     # "a" | "b" | "c"
    where: tuple = ()              # (file, text) of the check ("a") or the branch ("b")
    cond: tuple = ()               # (label, dims, min, state, where) under a condition
    branch: tuple = ()             # an "a" row whose kernel ALSO branches above the minimum
    word: str = ""                 # what the rejection's message calls it (default: name)
    note: str = ""


@dataclass(frozen=True)
class Val:
    """A non-pointer parameter and the value the validator tests pass."""
    name: str
    value: object


@dataclass(frozen=True)
class Entry:
    name: str
    params: tuple                  # Arg | Val | "dims" | "weights", in call order
    dims: dict = field(default_factory=dict)     # g2k_dims of the validator tests' call
    weights: tuple = ()            # the g2k_weights members read, as Args
    accept: str = "ok"

    @property
    def args(self):
        return tuple(p for p in self.params + self.weights if isinstance(p, Arg))

    def conditions(self):
        return tuple(a.cond[0] for a in self.args if a.cond)


def c4(name, elem="f32", note=""):
    return Arg(name, elem, 4, "c", note=note)


STREAM = Val("stream", None)
BASE = dict(S=0, F=20, T=8, L=12, D=16, H=128, Nmax=32, W=27, stride=1, flags=0)

# --- the scene kernel's entry points ---------------------------------------
SCENE_WEIGHTS = tuple(Arg(n, "f32", 4, "b", SEG) for n in ("Wi", "Wii", "Wv", "bv", "Wr", "Wc", "Wo"))
HEAD = Arg("head", "f32", 4, "b", SEG, note="read with G2K_STEP_LOSS_NLL only (segment 10)")
STEP_IN = (
    Arg("pos", "f32", 8, "a", POS8, branch=WIDE,
        note="float2 window reads; the 16-byte LDS-DMA only when pos is 16-byte aligned and Nmax even"),
    Arg("vislet", "f32", 4, "b", SEG),
    Arg("G", "f32", 4, "b", SEG),
    Arg("targets", "f32", 16, "a", TGT16, note="bload4 of the 96-byte rows; float4 in the a9 errors"),
    c4("n_active", "i32", "one scalar dword load"),
    c4("n_frames", "i32", "one scalar dword load"),
    Arg("ped_mask", "u8", 1, "b", MASK),
)
H_IN = Arg("h_in", "f32", 16, "a", H16)
H_OUT = Arg("h_out", "f32", 16, "a", H16)
PRED = Arg("pred", "f32", 4, "c", note="band layout: range-checked 4-byte buffer stores",
           cond=("ped_major", dict(flags=1), 16, "a", PRED16))
STEP_WS = Arg("workspace", "void", 4, "a", WS4,
              note="scene tickets (int fetch-adds) at 0, float partials at a multiple of 64")
TRAIN_WS = Arg("workspace", "void", 4, "a", WS4,
               note="float gradient rows, then the int ticket line and the split workspace, all at "
                    "multiples of 4")
UPDATE = (c4("params"), c4("ms"), Val("lr", 5e-3), Val("decay", 0.95), Val("grad_clip", 10.0))

ENTRIES = (
    Entry("g2k_workspace_init", (Arg("workspace", "void", 1, "c", note="hipMemsetAsync"),
                                 Val("workspace_bytes", 0), STREAM)),
    Entry("g2k_step_fused_f32",
          ("dims", "weights") + STEP_IN + (H_IN, H_OUT, PRED, c4("metrics"), c4("A_out"), c4("cost_out"),
                                           Val("lambda", 5e-4), STEP_WS, Val("workspace_bytes", 1 << 30),
                                           STREAM),
          dims=BASE, weights=SCENE_WEIGHTS),
    Entry("g2k_train_step_f32",
          ("dims", "weights") + STEP_IN + (H_IN, H_OUT, PRED, c4("metrics"), Val("lambda", 5e-4),
                                           c4("grad"), TRAIN_WS, Val("workspace_bytes", 0)) + UPDATE
          + (STREAM,),
          dims=dict(BASE, S=2), weights=SCENE_WEIGHTS + (HEAD,), accept="size"),
    Entry("g2k_step_grad_f32",
          ("dims", "weights") + STEP_IN + (Val("lambda", 5e-4), c4("grad"), TRAIN_WS,
                                           Val("workspace_bytes", 0), STREAM),
          dims=dict(BASE, S=2), weights=SCENE_WEIGHTS + (HEAD,), accept="size"),
    Entry("g2k_step_grad_update_f32",
          ("dims", "weights") + STEP_IN + (Val("lambda", 5e-4), c4("grad"), TRAIN_WS,
                                           Val("workspace_bytes", 0)) + UPDATE + (STREAM,),
          dims=dict(BASE, S=2), weights=SCENE_WEIGHTS + (HEAD,), accept="size"),
    # --- the stand-alone ops ---
    Entry("g2k_mcr_forward_f32",
          ("dims", "weights", c4("X"), c4("Rel"), c4("G"), c4("n_active", "i32"), c4("A_out"),
           c4("cost_out"), c4("pred"), Val("lambda", 5e-4), STREAM),
          dims=dict(BASE, D=10), weights=tuple(c4(n) for n in ("Wv", "bv", "Wr", "Wc", "Wo"))),
    Entry("g2k_frame_embed_f32",
          ("dims", "weights", Arg("pos", "f32", 8, "a", POS8, note="float2 reads"), c4("vislet"),
           c4("n_active", "i32"), c4("X"), c4("Rel"), STREAM),
          dims=BASE, weights=(c4("Wi"), c4("Wii"))),
    Entry("g2k_frame_recurrence_f32",
          ("dims",
           Arg("A", "f32", 4, "c", note="D < 16: staged element by element",
               cond=("D16", dict(D=16), 16, "a", REC16)),
           Arg("h", "f32", 4, "c", cond=("D16", dict(D=16), 16, "a", REC16)),
           Val("frames", 3), STREAM),
          dims=dict(BASE, D=10)),
    Entry("g2k_ade_fde_f32",
          ("dims", c4("pred"), Arg("targets", "f32", 16, "a", TGT16, note="float4 t4 of error_terms"),
           c4("n_active", "i32"), c4("n_frames", "i32"), Arg("ped_mask", "u8", 1, "c"),
           Val("variant", 0), c4("out"), STREAM),
          dims=BASE),
    Entry("g2k_infer_rlns_f32", (c4("adj"), c4("out"), Val("rows", 0), Val("cols", 4), STREAM)),
    Entry("g2k_eval_rln_ngh_f32", (c4("adj"), c4("out"), Val("rows", 0), Val("cols", 4), STREAM)),
    Entry("g2k_gridlstm_f32",
          (c4("in"), Val("ld_in", 16), c4("state"), Val("ld_state", 16), c4("W"), c4("b"), c4("peep"),
           c4("out"), c4("state_out"), Val("rows", 0), Val("blocks", 4), Val("feature_size", 4),
           Val("num_units", 2), STREAM)),
    Entry("g2k_encoder_chain_f32",
          ("dims", "weights", c4("X"), c4("Rel"), c4("G"), c4("n_active", "i32"), c4("n_frames", "i32"),
           c4("cell_W"), c4("cell_b"), c4("cell_peep"), Val("feature_size", 4), Val("num_units", 2),
           c4("Xe"), c4("cell_state"), Arg("attn", "f32", 16, "a", CHAIN16), c4("cost"), c4("pred"),
           Arg("h", "f32", 16, "a", CHAIN16), Val("lambda", 5e-4), STREAM),
          dims=BASE, weights=tuple(c4(n) for n in ("Wv", "bv", "Wr", "Wc", "Wo"))),
    Entry("g2k_update_f32",
          (c4("params"), c4("ms"), c4("grad"), Val("n_params", 0), Val("lr", 5e-3), Val("decay", 0.95),
           Val("grad_clip", 10.0), STREAM)),
    Entry("g2k_context_conv_f32",
          (c4("img"), Val("Hh", 20), Val("Ww", 20), Val("C", 3), c4("filt"), Val("D", 16),
           Val("lambda", 5e-4), c4("out"), c4("G"),
           Arg("workspace", "void", 4, "a", WS4, note="float partial sums"),
           Val("workspace_bytes", 0), STREAM),
          accept="size"),
    # --- the heads ---
    Entry("g2k_nll_f32",
          ("dims", c4("pred"), Arg("targets", "f32", 8, "a", TGT8, note="float2 reads"),
           c4("n_active", "i32"), c4("n_frames", "i32"), Arg("ped_mask", "u8", 1, "c"), c4("head"),
           c4("out"), c4("dpred"), Arg("workspace", "void", 4, "a", WS4, note="float rows"),
           Val("workspace_bytes", 0), STREAM),
          dims=dict(BASE, S=1), accept="size"),
    Entry("g2k_gauss_sample_f32", ("dims", c4("pred"), c4("head"), Val("seed", 3), c4("out"), STREAM),
          dims=BASE),
    Entry("g2k_fullcov_sample_f32", ("dims", c4("pred"), c4("chol"), Val("seed", 3), c4("out"), STREAM),
          dims=BASE),
)


def _pairs(head, tgt8=TGT8):
    return ("dims", c4("pred"), Arg("targets", "f32", 8, "a", tgt8, note="float2 reads"),
            c4("n_active", "i32"), c4("n_frames", "i32"), Arg("ped_mask", "u8", 1, "c"), c4(head))


def _marginal(name, head):
    return Entry(name, _pairs(head, S_TGT8) + (
        Val("seed", 7), Val("K", 20), Arg("per_ped", "f32", 16, "a", PERPED16, note="float4 stores"),
        c4("best"), c4("out"), Arg("workspace", "void", 4, "a", BK_WS4, note="float rows"),
        Val("workspace_bytes", 1 << 30), STREAM), dims=BASE)


def _kde(name, head):
    return Entry(name, _pairs(head, S_TGT8) + (
        Val("seed", 7), Val("K", 20), Val("log_floor", -20.0),
        Arg("per_ped", "f32", 16, "a", PERPED16, note="float4 stores"), c4("out"),
        Arg("workspace", "void", 4, "a", KDE_WS4, note="float rows"), Val("workspace_bytes", 1 << 30),
        STREAM), dims=BASE)


def _joint(name, head):
    return Entry(name, _pairs(head, S_TGT8) + (
        Val("seed", 7), Val("K", 20), Val("radius", 0.1), c4("per_frame_f"), c4("per_frame_i", "i32"),
        c4("sums_f"), Arg("sums_i", "i64", 8, "a", SUMSI8),
        Arg("workspace", "void", 4, "a", JT_WS4, note="int32 rows"), Val("workspace_bytes", 1 << 30),
        STREAM), dims=BASE)


def _stats(name, head, moments):
    dbl = lambda n, e="f64": Arg(n, e, 8, "a", DBL8)     # noqa: E731
    return Entry(name, _pairs(head) + (dbl("r2"), Val("n_levels", 4))
                 + ((dbl("moments"),) if moments else ())
                 + (dbl("stats"), dbl("inside", "i64"), c4("fit"),
                    Arg("workspace", "void", 8, "a", STWS8, note="slices of doubles and int64 counts"),
                    Val("workspace_bytes", 1 << 30), STREAM), dims=BASE)


ENTRIES += (
    _marginal("g2k_best_of_k_f32", "head"),
    _marginal("g2k_fullcov_best_of_k_f32", "chol"),
    _joint("g2k_joint_eval_f32", "head"),
    _joint("g2k_fullcov_joint_eval_f32", "chol"),
    _kde("g2k_kde_nll_f32", "head"),
    _kde("g2k_fullcov_kde_nll_f32", "chol"),
    _stats("g2k_head_stats_f32", "head", False),
    _stats("g2k_fullcov_stats_f32", "chol", True),
    # --- the data path's device gather ---
    Entry("g2k_scene_gather_f32",
          (Arg("xy", "f32", 8, "a", GATHER8, note="float2 reads"), c4("vis"), Val("cols", 10),
           c4("pos_col", "i32"), c4("tgt_col", "i32"), c4("vis_off", "i32"), c4("n_active", "i32"),
           Val("S", 0), Val("F", 1), Val("Nmax", 4),
           Arg("pos", "f32", 8, "a", GATHER8, note="float2 stores"), c4("vislet"),
           Arg("targets", "f32", 8, "a", GATHER8, note="float2 stores"),
           Arg("ped_mask", "u8", 1, "c"), STREAM)),
)

# --- include/g2k_mix.h: the Gaussian-mixture head ---------------------------
def _dbl8(name):
    return Arg(name, "f64", 8, "a", EM_DBL8)


def _scores(name, head):
    return Entry(name, _pairs(head, S_TGT8) + (
        Val("seed", 7), Val("K", 5), Arg("per_ped", "f32", 16, "a", PERPED16, note="two float4 stores a pair"),
        c4("out"), Arg("workspace", "void", 4, "a", SC_WS4, note="float rows"),
        Val("workspace_bytes", 1 << 30), STREAM), dims=BASE)


ENTRIES += (
    Entry("g2k_mix_em_f32",
          _pairs("mix_in", EM_TGT8)[:-1] + (
              # "mix_in and mix_out must be 4-byte aligned" restates the natural
              # alignment (tests/test_mixture.py holds that check): state "c"
              c4("mix_in", note="w, b and the factors: 4-byte loads"), _dbl8("moments"), _dbl8("resp"),
              _dbl8("total"), c4("mix_out", note="4-byte stores; may be NULL"),
              Arg("workspace", "void", 8, "a", EM_WS8, note="the responsibilities and the workgroups' rows: doubles"),
              Val("workspace_bytes", 1 << 30), STREAM),
          dims=BASE),
    Entry("g2k_mix_sample_f32",
          ("dims", c4("pred"), c4("mix"), Val("seed", 3), c4("out"), c4("comp", "i32"), STREAM), dims=BASE),
    _marginal("g2k_mix_best_of_k_f32", "mix"),
    _joint("g2k_mix_joint_eval_f32", "mix"),
    _kde("g2k_mix_kde_nll_f32", "mix"),
    # --- include/g2k_scores.h: the sample scores of the three heads ---
    _scores("g2k_sample_scores_f32", "head"),
    _scores("g2k_fullcov_sample_scores_f32", "chol"),
    _scores("g2k_mix_sample_scores_f32", "mix"),
)

BY_NAME = {e.name: e for e in ENTRIES}

# entry points of the headers without a device pointer (planning calls, host
# arithmetic) or with host pointers only (g2k_walk.cpp: out of scope here)
NO_DEVICE_POINTERS = (
    "g2k_abi_version", "g2k_last_error", "g2k_step_lds_bytes", "g2k_step_workspace_bytes",
    "g2k_step_split", "g2k_step_split_for_cus", "g2k_step_geometry", "g2k_grad_size",
    "g2k_grad_workspace_bytes", "g2k_train_workspace_bytes", "g2k_nll_workspace_bytes",
    "g2k_best_of_k_workspace_bytes", "g2k_fullcov_best_of_k_workspace_bytes",
    "g2k_joint_eval_workspace_bytes", "g2k_fullcov_joint_eval_workspace_bytes",
    "g2k_kde_nll_workspace_bytes", "g2k_fullcov_kde_nll_workspace_bytes",
    "g2k_head_stats_workspace_bytes", "g2k_fullcov_stats_workspace_bytes", "g2k_best_of_k_geometry",
    "g2k_context_conv_workspace_bytes", "g2k_traj_create", "g2k_traj_destroy", "g2k_traj_next_step",
    "g2k_traj_sample_scenes",
    # include/g2k_mix.h, include/g2k_scores.h
    "g2k_mix_em_workspace_bytes", "g2k_mix_best_of_k_workspace_bytes", "g2k_mix_joint_eval_workspace_bytes",
    "g2k_mix_kde_nll_workspace_bytes", "g2k_sample_scores_workspace_bytes", "g2k_sample_scores_geometry")
