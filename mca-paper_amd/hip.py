"""ctypes binding of libmca_hip.so (C ABI declared in include/mca_hip.h).

The library holds every compute kernel of the step; there is NO fallback: if it is missing or a call
returns an error code, this module raises.  Tensors are passed as raw device pointers
(``tensor.data_ptr()``) plus the current HIP stream handle — PyTorch only owns the memory.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MCA_HIP_LIB") or os.path.join(_HERE, "libmca_hip.so")          # MCA_HIP_LIB: A/B against another build of the same ABI

_ERR = {-1: "bad argument", -2: "misaligned pointer / leading dimension", -3: "unsupported size", -4: "launch failed"}


class MCAHipError(RuntimeError):
    pass


class LossTerm(C.Structure):
    _fields_ = [("slot_a", C.c_int32), ("slot_b", C.c_int32), ("and_bits", C.c_uint32), ("or_bits", C.c_uint32)]


class CastDesc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("lds", C.c_int64), ("rows", C.c_int64), ("cols", C.c_int64),
                ("ldd", C.c_int64), ("rows_pad", C.c_int64), ("cols_pad", C.c_int64), ("transpose", C.c_int32), ("scale", C.c_float)]


MAX_MODALITIES = 16


class TnDesc(C.Structure):
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int64), ("B", C.c_void_p), ("ldb", C.c_int64), ("C", C.c_void_p), ("ldc", C.c_int64),
                ("N", C.c_int64), ("K", C.c_int64)]


class MaskDesc(C.Structure):
    _fields_ = [("mask", C.c_void_p), ("rowmask", C.c_void_p), ("elem_bytes", C.c_int32), ("n", C.c_int32), ("offset", C.c_int32),
                ("pad_", C.c_int32)]


class FiniteArgs(C.Structure):
    _fields_ = [("p", C.c_void_p * MAX_MODALITIES), ("n", C.c_int64 * MAX_MODALITIES), ("count", C.c_int32), ("pad_", C.c_int32)]


class PackMasksArgs(C.Structure):
    _fields_ = [("m", MaskDesc * MAX_MODALITIES), ("n_mod", C.c_int32), ("batch", C.c_int32), ("n_tokens", C.c_int32),
                ("n_fusion", C.c_int32)]


class ModalityDropArgs(C.Structure):
    _fields_ = [("p", C.c_float * MAX_MODALITIES), ("seed", C.c_uint64), ("sample0", C.c_int64), ("keep_one", C.c_int32),
                ("pad_", C.c_int32)]


class AttnFwdArgs(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("q_bstride", C.c_int64), ("q_ld", C.c_int64),
        ("k", C.c_void_p), ("v", C.c_void_p), ("kv_bstride", C.c_int64), ("kv_ld", C.c_int64),
        ("o", C.c_void_p), ("o_bstride", C.c_int64), ("o_ld", C.c_int64),
        ("lse", C.c_void_p), ("qmask", C.c_void_p), ("keyinfo", C.c_void_p), ("ktile_flags", C.c_void_p),
        ("q_ptr", C.c_void_p), ("q_kt", C.c_void_p), ("q_order", C.c_void_p),
        ("vmean", C.c_void_p),
        ("batch", C.c_int), ("heads", C.c_int), ("nq", C.c_int), ("nk", C.c_int), ("nk_pad", C.c_int),
        ("n_qtiles", C.c_int), ("n_ktiles", C.c_int), ("scale", C.c_float), ("flags", C.c_int),
        ("khot", C.c_void_p),
    ]


class AttnReadoutArgs(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("q_bstride", C.c_int64), ("q_ld", C.c_int64),
        ("k", C.c_void_p), ("kv_bstride", C.c_int64), ("kv_ld", C.c_int64),
        ("lse", C.c_void_p), ("qmask", C.c_void_p), ("keyinfo", C.c_void_p), ("ktile_flags", C.c_void_p),
        ("q_ptr", C.c_void_p), ("q_kt", C.c_void_p), ("q_order", C.c_void_p),
        ("batch", C.c_int), ("heads", C.c_int), ("nq", C.c_int), ("nk", C.c_int), ("nk_pad", C.c_int),
        ("n_qtiles", C.c_int), ("n_ktiles", C.c_int), ("scale", C.c_float), ("flags", C.c_int),
        ("n_groups", C.c_int), ("uniform_mass", C.c_void_p), ("mass", C.c_void_p), ("probs", C.c_void_p),
        ("row0", C.c_int), ("n_rows", C.c_int),
    ]


class TaskHeadArgs(C.Structure):
    """mca_task_head_args (include/mca_hip.h)"""
    _fields_ = [
        ("pooled", C.c_void_p), ("present", C.c_void_p), ("any_bits", C.c_uint32),
        ("b", C.c_int), ("R", C.c_int), ("D", C.c_int), ("slot", C.c_int),
        ("w", C.c_void_p), ("bias", C.c_void_p), ("L", C.c_int),
        ("labels", C.c_void_p), ("ld_labels", C.c_int64), ("loss_type", C.c_int),
        ("task_weight", C.c_float), ("base_weight", C.c_float),
        ("d_pooled_in", C.c_void_p), ("pred", C.c_void_p), ("loss", C.c_void_p), ("d_pooled", C.c_void_p),
        ("gw", C.c_void_p), ("gb", C.c_void_p), ("accumulate", C.c_int),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]


class ClassHeadArgs(C.Structure):
    """mca_class_head_args (include/mca_hip.h)"""
    _fields_ = [
        ("pooled", C.c_void_p), ("present", C.c_void_p), ("any_bits", C.c_uint32),
        ("b", C.c_int), ("R", C.c_int), ("D", C.c_int), ("slot", C.c_int),
        ("w", C.c_void_p), ("bias", C.c_void_p), ("C", C.c_int),
        ("labels", C.c_void_p), ("ld_labels", C.c_int64),
        ("class_weights", C.c_void_p), ("label_smoothing", C.c_float),
        ("task_weight", C.c_float), ("base_weight", C.c_float),
        ("d_pooled_in", C.c_void_p), ("pred", C.c_void_p), ("loss", C.c_void_p), ("d_pooled", C.c_void_p),
        ("gw", C.c_void_p), ("gb", C.c_void_p), ("accumulate", C.c_int),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]


ATTN_Q_PRESCALED = 1
ATTN_LAZY_REFERENCE = 2          # mca_attn_fwd: lazy softmax reference (include/mca_hip.h)


class AttnFp8Operands(C.Structure):
    _fields_ = [("q8", C.c_void_p), ("qs", C.c_void_p), ("k8", C.c_void_p), ("ks", C.c_void_p), ("v8t", C.c_void_p), ("vs", C.c_void_p),
                ("n_ktiles", C.c_int)]


class AttnFp8BwdOperands(C.Structure):
    _fields_ = [("q8", C.c_void_p), ("qs", C.c_void_p), ("k8", C.c_void_p), ("ks", C.c_void_p), ("v8", C.c_void_p), ("vs", C.c_void_p),
                ("do8", C.c_void_p), ("dos", C.c_void_p), ("n_ktiles", C.c_int)]


class AttnBwd2Args(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("q_bstride", C.c_int64), ("q_ld", C.c_int64),
        ("k", C.c_void_p), ("v", C.c_void_p), ("kv_bstride", C.c_int64), ("kv_ld", C.c_int64),
        ("d_o", C.c_void_p), ("o_bstride", C.c_int64), ("o_ld", C.c_int64),
        ("lse", C.c_void_p), ("delta", C.c_void_p), ("dvmean", C.c_void_p),
        ("dq", C.c_void_p), ("dq_bstride", C.c_int64), ("dq_ld", C.c_int64), ("dq_f32", C.c_int),
        ("dk", C.c_void_p), ("dv", C.c_void_p), ("dkv_bstride", C.c_int64), ("dkv_ld", C.c_int64),
        ("qmask", C.c_void_p), ("keyinfo", C.c_void_p), ("ktile_flags", C.c_void_p),
        ("q_ptr", C.c_void_p), ("q_kt", C.c_void_p), ("q_order", C.c_void_p), ("n_qtiles128", C.c_int), ("n_ktiles64", C.c_int),
        ("k_wg", C.c_void_p), ("k_qt", C.c_void_p), ("n_qtiles64", C.c_int), ("n_kblocks256", C.c_int),
        ("batch", C.c_int), ("heads", C.c_int), ("nq", C.c_int), ("nk", C.c_int), ("nk_pad", C.c_int),
        ("scale", C.c_float), ("flags", C.c_int),
        ("khot", C.c_void_p), ("qblk", C.c_void_p), ("kblock_keys", C.c_int),
    ]


class AttnBwd1Args(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("q_bstride", C.c_int64), ("q_ld", C.c_int64),
        ("k", C.c_void_p), ("v", C.c_void_p), ("kv_bstride", C.c_int64), ("kv_ld", C.c_int64),
        ("d_o", C.c_void_p), ("o_bstride", C.c_int64), ("o_ld", C.c_int64),
        ("q_hstride", C.c_int64), ("o_hstride", C.c_int64),
        ("rowc", C.c_void_p), ("dvmean", C.c_void_p),
        ("dq", C.c_void_p), ("dq_bstride", C.c_int64), ("dq_ld", C.c_int64),
        ("dk", C.c_void_p), ("dv", C.c_void_p), ("dkv_bstride", C.c_int64), ("dkv_ld", C.c_int64),
        ("dq_acc", C.c_void_p),
        ("keyinfo", C.c_void_p), ("ktile_flags", C.c_void_p), ("khot", C.c_void_p), ("qblk", C.c_void_p),
        ("qt_desc", C.c_void_p), ("kb_desc", C.c_void_p), ("kb_qt", C.c_void_p), ("visit", C.c_void_p),
        ("n_qtiles", C.c_int), ("n_kblocks", C.c_int), ("max_list", C.c_int), ("n_entries", C.c_int),
        ("batch", C.c_int), ("heads", C.c_int), ("n", C.c_int), ("nk_pad", C.c_int), ("n_ktiles64", C.c_int),
        ("scale", C.c_float), ("flags", C.c_int), ("split", C.c_int),
    ]


class AttnLayout(C.Structure):
    """mca_attn_layout: elements between the heads of q and of k | v where they are not the 64-column blocks of a row (0 = 64)"""
    _fields_ = [("q_hstride", C.c_int64), ("kv_hstride", C.c_int64)]


# the GEMM planners' structs (csrc/gemm_plan.h; filled by the mca_dbg_plan_gemm_* hooks)
class GemmPlan(C.Structure):
    _fields_ = [(f, C.c_int) for f in ("kernel", "grid_x", "grid_y", "block", "lds_bytes", "n", "tiles_n", "nwg", "tiles_k",
                                       "rows_per_split", "dbg")]


class NtProblem(C.Structure):
    _fields_ = [("M", C.c_int64), ("N", C.c_int64), ("K", C.c_int64), ("out_bf16", C.c_int), ("res_period", C.c_int64),
                ("C", C.c_uint64), ("bias", C.c_uint64), ("residual", C.c_uint64), ("ldc", C.c_int64), ("ldres", C.c_int64)]


class TnPartition(C.Structure):
    _fields_ = [(f, C.c_int) for f in ("tiles", "R", "unit", "n_full", "span", "own")]


class TnGroupPlan(C.Structure):
    _fields_ = [("grouped", C.c_int), ("launch", GemmPlan), ("part", TnPartition)]


class TnDetPlan(C.Structure):
    _fields_ = [("launch", GemmPlan), ("slots", C.c_int), ("slot_stride", C.c_int64), ("scratch_floats", C.c_int64)]


class TnGroupDetPlan(C.Structure):
    _fields_ = [("plan", TnGroupPlan), ("slots", C.c_int), ("slot_stride", C.c_int64), ("scratch_floats", C.c_int64)]


PLAN_NT, PLAN_LNRES, PLAN_GEGLU_FWD, PLAN_GEGLU_BWD, PLAN_GEGLU_FWD_SAVED, PLAN_GEGLU_BWD_SAVED = range(6)          # `entry` of mca_dbg_plan_gemm_nt
GK_SAVED = 64          # csrc/gemm_plan.h MCA_GK_SAVED: a saved-factor kernel's value is its unsaved sibling's + this
PLAN_RES_LNBWD = 6     # mca_gemm_nt_res_lnbwd
GK_NT_ROWS_LNBWD = 128          # csrc/gemm_plan.h MCA_GK_NT_ROWS_LNBWD: gemm_nt_rows_kernel
PLAN_RES_LNBWD_TALL = 7         # mca_gemm_nt_res_lnbwd_tall
GK_NT_ROWS160_LNBWD = 160       # csrc/gemm_plan.h MCA_GK_NT_ROWS160_LNBWD: gemm_nt_rows160_kernel
KNOB_ROWS_HEIGHT = 15           # csrc/gemm_plan.h MCA_KNOB_ROWS_HEIGHT: 1 = always 128 rows, 2 = always 160 (the tall entry point only)
GK_NT_PERSIST256_CB = 256       # csrc/gemm_plan.h MCA_GK_NT_PERSIST256_CB: the 256 x 256 kernel with the column-blocked store (mca_gemm_nt_cb)


# the LayerNorm planners' structs (csrc/ln_plan.h; filled by mca_dbg_plan_layernorm_fwd / _bwd).  Pointers travel as integers.
class LnFwdProblem(C.Structure):
    _fields_ = [("rows", C.c_int64), ("cols", C.c_int32), ("cols_pad", C.c_int32)] + \
               [(f, C.c_int64) for f in ("ldx", "ldy", "y_bstride", "ld_bf16", "period")] + \
               [(f, C.c_uint64) for f in ("x", "gamma", "beta", "rowmask", "add", "y", "y_bf16")]


class LnFwdPlan(C.Structure):
    _fields_ = [("form", C.c_int32), ("width", C.c_int32), ("grid_x", C.c_int64), ("passes", C.c_int64)]


class LnBwdProblem(C.Structure):
    _fields_ = [("rows", C.c_int64), ("cols", C.c_int32), ("pad_", C.c_int32)] + \
               [(f, C.c_int64) for f in ("ldy", "y_bstride", "period", "ldx", "lddx", "ld_bf16")] + \
               [(f, C.c_uint64) for f in ("dy", "x", "gamma", "rowmask", "dx", "dx_bf16", "dgamma", "dbeta", "dxsum")]


class LnBwdPlan(C.Structure):
    _fields_ = [("form", C.c_int32), ("width", C.c_int32)] + \
               [(f, C.c_int64) for f in ("grid_x", "grid_y", "rows_per_block", "slots", "passes")]


LN_NONE, LN_NARROW, LN_TRUNK, LN_GENERAL, LN_PARAMS = range(5)          # `form` of the LayerNorm plans

_P, _I64, _I, _F = C.c_void_p, C.c_int64, C.c_int, C.c_float

# name -> (restype, argtypes).  Must list EVERY symbol include/mca_hip.h declares (tests check this).
SIGNATURES = {
    "mca_version": (C.c_char_p, []),
    "mca_flag_to_host": (_I, [_P, _P, _P]),
    "mca_build_keyhot": (_I, [_P, _P, _I, _I, _P]),
    "mca_rows_copy_add": (_I, [_P, _I64, _P, _I64, _I64, _I, _I, _I, _P]),
    "mca_segment_mean_fwd": (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _P]),
    "mca_segment_mean_bwd": (_I, [_P, _P, _P, _P, _I, _P, _I, _I, _I, _P]),
    "mca_gemm_nt": (_I, [_P, _I64, _P, _I64, _P, _I64, _I, _P, _P, _I64, _I64, _I64, _I64, _I64, _P]),
    "mca_gemm_nt_cb": (_I, [_P, _I64, _P, _I64, _P, _I64, _I64, _I64, _I64, _P]),          # A, lda, B, ldb, C, cbs, M, N, K
    "mca_gemm_nt_geglu_bwd": (_I, [_P, _I64, _P, _I64, _P, _P, _I64, _I64, _I64, _I64, _P]),
    "mca_gemm_nt_lnres": (_I, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _P, _P, _I64, _I64, _I64, _P]),
    "mca_gemm_nt_geglu_fwd": (_I, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _I64, _I64, _I64, _P]),
    # saved-factor forms: the siblings' argument lists, s in the place of h
    "mca_gemm_nt_geglu_fwd_saved": (_I, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _I64, _I64, _I64, _P]),
    "mca_gemm_nt_geglu_bwd_saved": (_I, [_P, _I64, _P, _I64, _P, _P, _I64, _I64, _I64, _I64, _P]),
    # full-row GEMM + LayerNorm backward: A, lda, B, ldb, residual, ldres, x, ldx, mean, rstd, gamma, dx, lddx, dx_bf16, ld_bf16, dgamma, M, N, K
    "mca_gemm_nt_res_lnbwd": (_I, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _P, _P, _P, _I64, _P, _I64, _P, _I64, _I64, _I64, _P]),
    "mca_gemm_nt_res_lnbwd_tall": (_I, [_P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _P, _P, _P, _I64, _P, _I64, _P, _I64, _I64, _I64, _P]),
    "mca_geglu_fwd_saved": (_I, [_P, _P, _I64, _I, _P]),
    "mca_geglu_bwd_saved": (_I, [_P, _P, _P, _I64, _I, _P]),
    "mca_gemm_tn_acc": (_I, [_P, _I64, _P, _I64, _P, _I64, _I64, _I64, _I64, _P]),
    "mca_gemm_tn_acc_group": (_I, [_P, _I, _I64, _P]),
    "mca_layernorm_fwd": (_I, [_P, _I64, _P, _P, _P, _P, _I64, _P, _I64, _I64, _P, _I64, _I, _P, _P, _I64, _I, _F, _P]),
    "mca_layernorm_bwd": (_I, [_P, _I64, _I64, _I64, _P, _I64, _P, _P, _P, _P, _P, _I64, _P, _I64, _P, _P, _P, _I64, _I, _P]),
    "mca_geglu_fwd": (_I, [_P, _P, _I64, _I, _P]),
    "mca_geglu_bwd": (_I, [_P, _P, _P, _I64, _I, _P]),
    "mca_cast_pad_bf16": (_I, [_P, _I64, _I64, _I64, _P, _I64, _I64, _I64, _I, _P]),
    "mca_cast_pad_bf16_multi": (_I, [_P, _I, _P]),
    "mca_f32_to_bf16": (_I, [_P, _I64, _P, _I64, _I64, _I64, _F, _P]),
    "mca_bcast_rows": (_I, [_P, _I64, _P, _I64, _I64, _I64, _I64, _I, _P]),
    "mca_reduce_rows": (_I, [_P, _I64, _I64, _I64, _P, _I64, _I64, _I, _P]),
    "mca_embedding_renorm": (_I, [_P, _I64, _I, _F, _P]),
    "mca_embedding_lookup": (_I, [_P, _I64, _I, _F, _P, _I, _I64, _I64, _P, _P, _I64, _I64, _I, _P, _P, _I, _P]),
    "mca_embedding_scatter_add": (_I, [_P, _I64, _I64, _I64, _P, _I, _I64, _P, _I64, _I, _I64, _P]),
    "mca_tab_value_fwd": (_I, [_P, _P, _P, _P, _P, _I64, _I, _F, _F, _P]),
    "mca_tab_value_bwd": (_I, [_P, _I64, _P, _P, _P, _P, _I64, _I, _F, _P]),
    "mca_patch_ln_fwd": (_I, [_P, _I64, _I64, _I, _I, _I, _I, _I, _P, _P, _F, _F, _P, _P, _I64, _I, _P, _P, _P, _P]),
    "mca_patch_nd_ln_fwd": (_I, [_P, _I64, _I64, _I64, _I64, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _F, _F, _P, _P, _I64, _I, _P, _P, _P, _P]),
    "mca_pack_masks": (_I, [_P, _P, _P, _P]),
    "mca_pack_masks_drop": (_I, [_P, _P, _P, _P, _P, _P, _P]),
    "mca_counter_add": (_I, [_P, _I64, _P]),
    "mca_build_keyinfo": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "mca_attn_vmean": (_I, [_P, _I64, _I64, _P, _I, _I, _I, _P]),
    "mca_attn_vmean_if_needed": (_I, [_P, _I64, _I64, _P, _I, _I, _I, _P, _I, _P]),
    "mca_attn_fwd": (_I, [C.POINTER(AttnFwdArgs), _P]),
    # the _hm forms: head strides beside the unchanged structs (AttnLayout)
    "mca_attn_fwd_hm": (_I, [C.POINTER(AttnFwdArgs), C.POINTER(AttnLayout), _P]),
    "mca_attn_vmean_if_needed_hm": (_I, [_P, _I64, _I64, _I64, _P, _I, _I, _I, _P, _I, _P]),
    "mca_attn_bwd_onepass_hm": (_I, [C.POINTER(AttnBwd1Args), C.POINTER(AttnLayout), _P]),
    # o, o_bstride, o_ld, d_o, do_bstride, do_hstride, do_ld, lse, row_slot, rowc, dvmean, batch, heads, n, n_qtiles
    "mca_attn_bwd_prep_onepass_hm": (_I, [_P, _I64, _I64, _P, _I64, _I64, _I64, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "mca_attn_readout": (_I, [C.POINTER(AttnReadoutArgs), _P]),
    "mca_attn_quant_mxfp8": (_I, [_P, _I64, _I64, _P, _P, _I64, _I64, C.POINTER(AttnFp8Operands), _I, _I, _I, _P]),
    "mca_attn_fwd_fp8": (_I, [C.POINTER(AttnFwdArgs), C.POINTER(AttnFp8Operands), _P]),
    "mca_attn_bwd_prep": (_I, [_P, _P, _I64, _I64, _P, _P, _P, _I, _I, _I, _I, _P]),
    "mca_attn_bwd_onepass": (_I, [C.POINTER(AttnBwd1Args), _P]),
    "mca_attn_bwd_prep_onepass": (_I, [_P, _P, _I64, _I64, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I64, _I64, _P, _P, _P]),
    "mca_attn_bwd_dq": (_I, [C.POINTER(AttnBwd2Args), _P]),
    "mca_attn_bwd_dkv": (_I, [C.POINTER(AttnBwd2Args), _P]),
    "mca_attn_quant_bwd_mxfp8": (_I, [_P, _I64, _I64, _P, _P, _I64, _I64, _P, _I64, _I64, C.POINTER(AttnFp8BwdOperands), _I, _I, _I, _I, _P]),
    "mca_attn_bwd_dq_fp8": (_I, [C.POINTER(AttnBwd2Args), C.POINTER(AttnFp8BwdOperands), _P]),
    "mca_attn_bwd_dkv_fp8": (_I, [C.POINTER(AttnBwd2Args), C.POINTER(AttnFp8BwdOperands), _P]),
    "mca_contrastive_workspace_bytes": (_I64, [_I, _I]),
    "mca_contrastive_fwd_bwd": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "mca_contrastive_stream_workspace_bytes": (_I64, [_I, _I, _I, _I]),
    "mca_contrastive_stream_fwd_bwd": (_I, [_P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I64, _P]),
    "mca_grad_sqnorm": (_I, [_P, _I64, _P, _P]),
    "mca_adamw_step": (_I, [_P, _P, _P, _P, _I64, _F, _F, _F, _F, _F, _F, _F, _F, _P, _P, _P, _P]),
    "mca_adamw_hyper": (_I, [_P, _F, _F, _F, _P]),
    "mca_nonfinite_flag": (_I, [C.POINTER(FiniteArgs), _P, _I, _P]),
    "mca_rows_normalize_f32": (_I, [_P, _I64, _P, _I64, _I64, _I64, _P]),
    "mca_cosine_rank_f32": (_I, [_P, _I64, _P, _I64, _P, _I64, _I64, _I64, _P, _P, _P]),
    "mca_cosine_topk_workspace": (_I64, [_I64, _I64, _I]),
    "mca_cosine_topk_f32": (_I, [_P, _I64, _P, _I64, _P, _I64, _I64, _I64, _P, _P, _I, _P, _I64, _P, _I64, _P, _I64, _P]),
    "mca_pair_gauss_workspace": (_I64, [_I64]),
    "mca_pair_gauss_sum_f32": (_I, [_P, _I64, _I64, _I64, _F, _P, _I64, _P, _P, _P]),
    "mca_probe_nt_f32": (_I, [_P, _I64, _P, _P, _I64, _P, _P, _I64, _I64, _I64, _I64, _I, _F, C.c_uint64, _I64, _P]),
    "mca_probe_head_blocks": (_I64, [_I64]),
    "mca_probe_head_f32": (_I, [_P, _I64, _P, _I64, _P, _P, _I64, _P, _P, _I64, _I, _P, _P, _P, _F, _P, _P]),
    "mca_probe_tn_workspace": (_I64, [_I64, _I64, _I64]),
    "mca_probe_tn_f32": (_I, [_P, _I64, _P, _I64, _P, _I64, _I64, _I64, _P, _I64, _P, _P, _P]),
    "mca_probe_loss_accum": (_I, [_P, _I64, _I64, _P, _P]),
    "mca_task_head_workspace_bytes": (_I64, [_I, _I, _I]),
    "mca_task_head_fwd_bwd": (_I, [C.POINTER(TaskHeadArgs), _P]),
    "mca_probe_head_ce_f32": (_I, [_P, _I64, _P, _I64, _P, _P, _I64, _P, _I64, _P, _I64, _P, _P, _P, _F, _P, _P]),
    "mca_class_head_workspace_bytes": (_I64, [_I, _I, _I]),
    "mca_class_head_fwd_bwd": (_I, [C.POINTER(ClassHeadArgs), _P]),
    # deterministic forms: the plain form's arguments + (scratch, scratch_floats) before the stream, and their size queries
    "mca_gemm_tn_acc_det_scratch": (_I64, [_I64, _I64, _I64]),
    "mca_gemm_tn_acc_det": (_I, [_P, _I64, _P, _I64, _P, _I64, _I64, _I64, _I64, _P, _I64, _P]),
    "mca_gemm_tn_acc_group_det_scratch": (_I64, [C.POINTER(_I64), C.POINTER(_I64), _I, _I64, _I]),
    "mca_gemm_tn_acc_group_det": (_I, [_P, _I, _I64, _P, _I64, _P]),
    "mca_layernorm_bwd_det_scratch": (_I64, [_I64, _I]),
    "mca_layernorm_bwd_det": (_I, [_P, _I64, _I64, _I64, _P, _I64, _P, _P, _P, _P, _P, _I64, _P, _I64, _P, _P, _P, _I64, _I, _P, _I64, _P]),
    "mca_reduce_rows_det_scratch": (_I64, [_I64, _I64, _I]),
    "mca_reduce_rows_det": (_I, [_P, _I64, _I64, _I64, _P, _I64, _I64, _I, _P, _I64, _P]),
    "mca_tab_value_bwd_det_scratch": (_I64, [_I64, _I]),
    "mca_tab_value_bwd_det": (_I, [_P, _I64, _P, _P, _P, _P, _I64, _I, _F, _P, _I64, _P]),
    "mca_embedding_scatter_add_det_scratch": (_I64, [_I64]),
    "mca_embedding_scatter_add_det": (_I, [_P, _I64, _I64, _I64, _P, _I, _I64, _P, _I64, _I, _I64, _P, _I64, _P]),
}
# measurement hooks (include/mca_hip_debug.h): exported by the library, not part of the drop-in ABI
DEBUG_SIGNATURES = {
    "mca_debug_set": (_I, [_I, _I]),
    "mca_debug_reset": (_I, []),
    "mca_dbg_gemm_kernel_name": (C.c_char_p, [_I]),
    "mca_dbg_plan_gemm_nt": (_I, [_I, C.POINTER(NtProblem), _I, C.POINTER(GemmPlan)]),
    "mca_dbg_plan_gemm_nt_cb": (_I, [_I64, _I64, _I64, C.c_uint64, _I64, _I, C.POINTER(GemmPlan)]),          # M, N, K, C, cbs, cus
    "mca_dbg_plan_gemm_tn": (_I, [_I64, _I64, _I64, C.POINTER(GemmPlan)]),
    "mca_dbg_plan_gemm_tn_group": (_I, [C.POINTER(_I64), C.POINTER(_I64), _I, _I64, _I, C.POINTER(TnGroupPlan)]),
    "mca_dbg_plan_gemm_tn_det": (_I, [_I64, _I64, _I64, C.POINTER(TnDetPlan)]),
    "mca_dbg_plan_gemm_tn_group_det": (_I, [C.POINTER(_I64), C.POINTER(_I64), _I, _I64, _I, C.POINTER(TnGroupDetPlan)]),
    "mca_dbg_plan_layernorm_fwd": (_I, [C.POINTER(LnFwdProblem), C.POINTER(LnFwdPlan)]),
    "mca_dbg_plan_layernorm_bwd": (_I, [C.POINTER(LnBwdProblem), C.POINTER(LnBwdPlan)]),
    "mca_dbg_contrastive_layout": (_I, [_I, _I, C.POINTER(_I64)]),
    "mca_dbg_contrastive_stream_layout": (_I, [_I, _I, C.POINTER(_I64)]),
}

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load the shared library (built by ``__graft_entry__.build()`` / ``mca-paper_amd/build.py``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MCAHipError(
                f"{LIB_PATH} not found: the HIP extension is not built (run `python __graft_entry__.py build`). "
                "There is no CPU or eager fallback for the MCA step.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(DEBUG_SIGNATURES.items()):
            fn = getattr(l, name)          # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


_STREAM_CACHE = None     # set by the engine for the duration of a step (the stream does not change inside it)


def stream_ptr() -> int:
    if _STREAM_CACHE is not None:
        return _STREAM_CACHE
    return torch.cuda.current_stream().cuda_stream


class use_stream:
    """context manager: launch through an explicit stream handle (side-stream weight gradients)."""

    def __init__(self, handle: int):
        self.handle = handle

    def __enter__(self):
        global _STREAM_CACHE
        self.prev = _STREAM_CACHE
        _STREAM_CACHE = self.handle

    def __exit__(self, *exc):
        global _STREAM_CACHE
        _STREAM_CACHE = self.prev


class cached_stream:
    """context manager: query torch's current stream once and reuse the handle for every launch inside."""

    def __enter__(self):
        global _STREAM_CACHE
        self.prev = _STREAM_CACHE
        _STREAM_CACHE = torch.cuda.current_stream().cuda_stream

    def __exit__(self, *exc):
        global _STREAM_CACHE
        _STREAM_CACHE = self.prev


class knobs:
    """context manager for tests / tools: set measurement knobs (include/mca_hip_debug.h) and ALWAYS reset all of them on
    exit, so a failing test cannot leave the conservative kernels switched on for the rest of the process."""

    def __init__(self, **kv):
        self.kv = {int(k[1:]) if isinstance(k, str) else int(k): int(v) for k, v in kv.items()}

    def __enter__(self):
        for k, v in self.kv.items():
            lib().mca_debug_set(k, v)
        return self

    def __exit__(self, *exc):
        lib().mca_debug_reset()


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr()


def contrastive_layout(B: int, T: int) -> dict:
    """{region: (byte offset, bytes)} of mca_contrastive_fwd_bwd's workspace for region in G, stats, w (include/mca_hip_debug.h)"""
    out = (_I64 * 6)()
    check(lib().mca_dbg_contrastive_layout(B, T, out), "mca_dbg_contrastive_layout")
    return {"G": (out[0], out[1]), "stats": (out[2], out[3]), "w": (out[4], out[5])}


def contrastive_stream_layout(B: int, T: int) -> dict:
    """mca_contrastive_stream_fwd_bwd's tile constants TI, TJ, TK, DMAX and {region: (byte offset, bytes)} of its workspace for
    region in lse, erat, diag, red, w (include/mca_hip_debug.h)"""
    out = (_I64 * 14)()
    check(lib().mca_dbg_contrastive_stream_layout(B, T, out), "mca_dbg_contrastive_stream_layout")
    lay = {"TI": out[0], "TJ": out[1], "TK": out[2], "DMAX": out[3]}
    for k, name in enumerate(("lse", "erat", "diag", "red", "w")):
        lay[name] = (out[4 + 2 * k], out[5 + 2 * k])
    return lay


def check(rc: int, what: str):
    if rc != 0:
        raise MCAHipError(f"{what} failed: {_ERR.get(rc, rc)}")


# ---- optional live kernel timing (bench.py): HIP events recorded on the launch stream around selected entry points
PROFILE = None          # None or {"names": set, "records": {key: [(start, end, flops)]}}
_PROFILE_ON = True      # sampling switch: bench.py records only every n-th step to keep the event overhead < 1 %
_TAG = ""


def profile_enable(flag: bool):
    global _PROFILE_ON
    _PROFILE_ON = bool(flag)


def set_tag(tag: str):
    global _TAG
    _TAG = tag


def profile_start(names):
    global PROFILE
    PROFILE = {"names": set(names), "records": {}}


def profile_collect():
    """Resolve the events recorded so far into (launches, ms, flops) totals and release them (synchronises).  Called after
    every sampled step so that at most one step's worth of timing events is ever outstanding on the queue."""
    torch.cuda.synchronize()
    tot = PROFILE.setdefault("totals", {})
    for key, recs in PROFILE["records"].items():
        n, ms, fl = tot.get(key, (0, 0.0, 0.0))
        tot[key] = (n + len(recs), ms + sum(s.elapsed_time(e) for s, e, _ in recs), fl + sum(f for _, _, f in recs))
    PROFILE["records"] = {}


def profile_stop():
    """-> {key: (launches, total_ms, total_flops)} (synchronises)."""
    global PROFILE
    profile_collect()
    prof, PROFILE = PROFILE, None
    return prof["totals"]


def call(name: str, *args, flops: float = 0.0, profile_as: Optional[str] = None):
    """profile_as: the key this launch is timed and recorded under instead of its own name: another form of the same
    operation (the saved-factor GEGLU GEMMs) then stays in the row of the form it replaces, comparable across commits."""
    key = profile_as or name
    # (a deterministic form is timed wherever its plain form is asked for, under its own name)
    if PROFILE is not None and _PROFILE_ON and (key in PROFILE["names"] or (key.endswith("_det") and key[:-4] in PROFILE["names"])):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        check(getattr(lib(), name)(*args), name)
        e.record()
        PROFILE["records"].setdefault(key + ("/" + _TAG if _TAG else ""), []).append((s, e, flops))
        return
    check(getattr(lib(), name)(*args), name)
