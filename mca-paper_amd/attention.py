"""Host side of the attention launches: which backward form runs (ONE pure function, backward_plan), the operand records, the
builders that turn them into the argument structs of the C ABI (fwd_args, bwd2_args, bwd1_args, readout_args: pure, they read
only data_ptr(), stride() and integers, so they run on CPU tensors), the launch functions (launch_forward, backward_twopass,
backward_onepass) and the device copies of the tile schedules.  Imports without a GPU and without loading the library.

The layer attention's backward has three forms: the bf16 one-pass kernel (attention_bwd1.hip), the two-pass kernels with bf16
score recomputes (attention_bwd2.hip) and the two-pass kernels with fp8 score recomputes (attention_fp8.hip).  The pooling
attention (fp32 dq, nq != nk) always takes the bf16 two-pass form."""
from __future__ import annotations

import ctypes as C
from typing import Any, NamedTuple, Optional

import numpy as np
import torch

from . import hip
from .hip import AttnBwd1Args, AttnBwd2Args, AttnFwdArgs, AttnLayout, AttnReadoutArgs, call, stream_ptr

ONEPASS_MIN_WG = 192          # (sample, head) pairs from which the one-pass backward is the default: one workgroup per CU


class Plan(NamedTuple):
    form: str          # "onepass" | "fp8-twopass" | "bf16-twopass"
    split: int         # workgroups per (sample, head) of the one-pass kernel at this batch (sizes dq_acc whatever the form)


def backward_plan(*, attn_dtype: str, mask_product: bool, onepass_tables_fit: bool, onepass_want: Optional[bool], dkv_keys: int,
                  b: int, heads: int, n_kblocks: int, layer_attention: bool, dq_f32: bool) -> Plan:
    """The backward form of one attention launch.  onepass_want: MCA_DEBUG's onepass switch (None = by size).

    split: 1 where the batch gives every CU a (sample, head), else up to 4 (key blocks dealt round robin, partial dQ sums added by
    the call's second launch) - b = 8, 8 heads: 4 x 64 = 256 workgroups.
    One-pass wherever it applies (layer attention, bf16 dq, mask product, tables that fit the kernel's LDS) and the split fills
    the chip - also with fp8 operands: it is faster than the two-pass backward with fp8 score recomputes (LONG b = 128: 9.1
    against 10.5 ms per layer), so fp8 operands at a large batch mean the fp8 forward + the bf16 one-pass backward; the fp8
    two-pass backward remains for small batches (and onepass=0) and needs the mask product and 128-key dkv blocks."""
    wg = b * heads
    split = 1 if wg >= ONEPASS_MIN_WG else max(1, min(4, n_kblocks if onepass_tables_fit else 1, -(-256 // wg)))
    layer = layer_attention and not dq_f32
    if layer and mask_product and onepass_tables_fit:
        if bool(onepass_want) if onepass_want is not None else wg * split >= ONEPASS_MIN_WG:
            return Plan("onepass", split)
    if attn_dtype == "fp8" and layer and mask_product and dkv_keys == 128:
        return Plan("fp8-twopass", split)
    return Plan("bf16-twopass", split)


def describe(plan: Plan) -> str:
    """a plan as bench.py reports it (config.attention_backward)"""
    if plan.form == "onepass":
        return "bf16 one-pass" + (f" (key blocks split {plan.split} ways)" if plan.split > 1 else "")
    return {"fp8-twopass": "fp8 two-pass", "bf16-twopass": "bf16 two-pass"}[plan.form]


class AttnOperands(NamedTuple):
    """One attention's forward operands (bf16; strides and offsets in elements).  Built by FusionEngine.layer_attention /
    pool_attention, taken by attn_forward / attn_backward."""
    q: int                      # device pointer: q[sample * q_bstride + row * q_ld + head * 64 + d]
    q_bstride: int
    q_ld: int
    kv: torch.Tensor            # k and v are column blocks of one matrix: kv[(sample * nk + key) * kv_ld + k_off | v_off + ...]
    k_off: int
    v_off: int
    kv_ld: int
    o: torch.Tensor             # (b * nq, D) bf16
    lse: torch.Tensor           # (b, H, nq) fp32
    nq: int
    qmask: torch.Tensor
    qblk: torch.Tensor          # the query side of the mask product for the same mask
    sched_f: Any                # _Sched of the forward and dq pass
    sched_b: Any                # _Sched of the dkv pass
    layer: Optional[int]        # fusion layer (its fp8 operand cache); None: the pooling attention
    hstride: int = 0            # elements between the heads of q and of k | v; 0: the 64-column blocks of a row.  The head-major
                                # output of mca_gemm_nt_cb ([block][T][64], slabs cbs apart): q_bstride = nk * 64, q_ld = kv_ld = 64,
                                # k_off = H * cbs, v_off = 2 * H * cbs, hstride = cbs; only the _hm entry points take it


class AttnGrads(NamedTuple):
    """what the backward of an AttnOperands adds"""
    d_o: torch.Tensor           # (b * nq, D) bf16
    delta: torch.Tensor         # (b, H, nq) fp32, written by the prep launch
    dq: int                     # device pointer, strides as q
    dq_bstride: int
    dq_ld: int
    dq_f32: bool
    dkv: torch.Tensor           # dk and dv are column blocks of one matrix, as kv
    dk_off: int
    dv_off: int
    dkv_ld: int
    do_hstride: int = 0         # d_o written head-major by mca_gemm_nt_cb: d_o[(sample * nq + row) * 64 + head * do_hstride + d]


class AttnKeys(NamedTuple):
    """the key-side state every attention of one forward shares (the engine: from its workspace; a test: from its own tensors)"""
    keyinfo: torch.Tensor       # (batch, nk_pad) uint8, mca_build_keyinfo
    kflags: torch.Tensor        # (batch, key tiles) uint8
    khot: Optional[torch.Tensor]          # (batch, nk_pad, 16) bf16 one-hot operand of the mask product; None: element-wise mask
    nk: int
    nk_pad: int
    batch: int
    heads: int
    scale: float
    flags: int                  # hip.ATTN_Q_PRESCALED [| hip.ATTN_LAZY_REFERENCE]


class RowSource(NamedTuple):
    """where the one-pass backward reads q or dO: x[sample * bstride + head * hstride + row * ld + d], hstride 0 = the heads
    are the 64-column blocks of a row (the (b * n, heads * 64) matrices); the packed head-major copies: (H * n * 64, n * 64, 64)"""
    ptr: int
    bstride: int
    hstride: int
    ld: int


def _shared(a, ops, keys):
    """the fields AttnFwdArgs, AttnBwd2Args and AttnBwd1Args share.  k | v are column offsets (two bytes an element) into ONE
    matrix whose samples lie nk rows apart; khot / qblk stay null without the mask product."""
    a.q, a.q_bstride, a.q_ld = ops.q, ops.q_bstride, ops.q_ld
    kv = ops.kv.data_ptr()
    a.k, a.v, a.kv_bstride, a.kv_ld = kv + ops.k_off * 2, kv + ops.v_off * 2, keys.nk * ops.kv_ld, ops.kv_ld
    a.keyinfo, a.ktile_flags = keys.keyinfo.data_ptr(), keys.kflags.data_ptr()
    if keys.khot is not None:
        a.khot = keys.khot.data_ptr()
        if hasattr(a, "qblk"):
            a.qblk = ops.qblk.data_ptr()
    a.batch, a.heads, a.nk_pad, a.scale, a.flags = keys.batch, keys.heads, keys.nk_pad, keys.scale, keys.flags
    return a


def layout_args(ops: AttnOperands) -> AttnLayout:
    """the head strides of ops for the _hm entry points (zero: the plain entry points' layout)"""
    return AttnLayout(ops.hstride, ops.hstride)


def fwd_args(ops: AttnOperands, keys: AttnKeys, vmean: torch.Tensor) -> AttnFwdArgs:
    a, sched = _shared(AttnFwdArgs(), ops, keys), ops.sched_f
    a.o, a.o_bstride, a.o_ld = ops.o.data_ptr(), ops.nq * ops.o.stride(0), ops.o.stride(0)
    a.lse, a.qmask, a.vmean = ops.lse.data_ptr(), ops.qmask.data_ptr(), vmean.data_ptr()
    a.q_ptr, a.q_kt, a.q_order = sched.q_ptr.data_ptr(), sched.q_kt.data_ptr(), sched.q_order.data_ptr()
    a.nq, a.nk, a.n_qtiles, a.n_ktiles = ops.nq, keys.nk, sched.s.n_q, sched.s.n_k
    return a


def bwd2_args(ops: AttnOperands, grads: AttnGrads, keys: AttnKeys, dvmean: torch.Tensor, sched_b=None) -> AttnBwd2Args:
    """sched_b: the dkv pass's _Sched (default ops.sched_b); its key-block size goes into kblock_keys"""
    a, sched_f, sched_b, d_o = _shared(AttnBwd2Args(), ops, keys), ops.sched_f, sched_b or ops.sched_b, grads.d_o
    a.d_o, a.o_bstride, a.o_ld = d_o.data_ptr(), ops.nq * d_o.stride(0), d_o.stride(0)
    a.lse, a.delta, a.dvmean = ops.lse.data_ptr(), grads.delta.data_ptr(), dvmean.data_ptr()
    a.dq, a.dq_bstride, a.dq_ld, a.dq_f32 = grads.dq, grads.dq_bstride, grads.dq_ld, int(grads.dq_f32)
    dkv = grads.dkv.data_ptr()
    a.dk, a.dv, a.dkv_bstride, a.dkv_ld = dkv + grads.dk_off * 2, dkv + grads.dv_off * 2, keys.nk * grads.dkv_ld, grads.dkv_ld
    a.qmask = ops.qmask.data_ptr()
    a.q_ptr, a.q_kt, a.q_order = sched_f.q_ptr.data_ptr(), sched_f.q_kt.data_ptr(), sched_f.q_order.data_ptr()
    a.n_qtiles128, a.n_ktiles64 = sched_f.s.n_q, sched_f.s.n_k
    a.k_wg, a.k_qt, a.n_qtiles64, a.n_kblocks256 = sched_b.k_wg.data_ptr(), sched_b.k_qt.data_ptr(), sched_b.s.n_q, sched_b.s.n_k
    a.nq, a.nk, a.kblock_keys = ops.nq, keys.nk, sched_b.s.bk
    return a


def bwd1_args(ops: AttnOperands, grads: AttnGrads, keys: AttnKeys, sched: "_OnePassSched", rowc: torch.Tensor, dq_acc: torch.Tensor,
              dvmean: torch.Tensor, split: int, q: RowSource, d_o: RowSource) -> AttnBwd1Args:
    """the one-pass backward on the tables `sched`; q, d_o: where it reads them (the row-major matrices or the packed copies
    mca_attn_bwd_prep_onepass wrote)"""
    a = _shared(AttnBwd1Args(), ops, keys)
    a.q, a.q_bstride, a.q_hstride, a.q_ld = q
    a.d_o, a.o_bstride, a.o_hstride, a.o_ld = d_o
    a.rowc, a.dvmean, a.dq_acc = rowc.data_ptr(), dvmean.data_ptr(), dq_acc.data_ptr()
    a.dq, a.dq_bstride, a.dq_ld = grads.dq, grads.dq_bstride, grads.dq_ld
    dkv = grads.dkv.data_ptr()
    a.dk, a.dv, a.dkv_bstride, a.dkv_ld = dkv + grads.dk_off * 2, dkv + grads.dv_off * 2, keys.nk * grads.dkv_ld, grads.dkv_ld
    a.qt_desc, a.kb_desc, a.kb_qt, a.visit = sched.qt_desc.data_ptr(), sched.kb_desc.data_ptr(), sched.kb_qt.data_ptr(), sched.visit.data_ptr()
    a.n_qtiles, a.n_kblocks, a.max_list, a.n_entries = sched.n_qt, sched.n_kb, sched.max_list, sched.n_entries
    a.n, a.n_ktiles64, a.split = keys.nk, (keys.nk + 63) // 64, split
    return a


def readout_args(ops: AttnOperands, keys: AttnKeys, uniform_mass: torch.Tensor, mass: torch.Tensor,
                 probs: Optional[torch.Tensor] = None, row0: int = 0) -> AttnReadoutArgs:
    """mca_attn_readout on the operands of an attention whose forward has run (another lse: ops._replace(lse=...)); probs:
    (b, H, rows, nk) fp32, the probabilities of the query rows row0 .. row0 + rows"""
    a, sched = AttnReadoutArgs(), ops.sched_f
    a.q, a.q_bstride, a.q_ld = ops.q, ops.q_bstride, ops.q_ld
    a.k, a.kv_bstride, a.kv_ld = ops.kv.data_ptr() + ops.k_off * 2, keys.nk * ops.kv_ld, ops.kv_ld
    a.lse, a.qmask = ops.lse.data_ptr(), ops.qmask.data_ptr()
    a.keyinfo, a.ktile_flags = keys.keyinfo.data_ptr(), keys.kflags.data_ptr()
    a.q_ptr, a.q_kt, a.q_order = sched.q_ptr.data_ptr(), sched.q_kt.data_ptr(), sched.q_order.data_ptr()
    a.batch, a.heads, a.nq, a.nk, a.nk_pad = keys.batch, keys.heads, ops.nq, keys.nk, keys.nk_pad
    # (the readout has the textbook recurrence only: the forward's softmax form is not its business)
    a.n_qtiles, a.n_ktiles, a.scale, a.flags = sched.s.n_q, sched.s.n_k, keys.scale, keys.flags & hip.ATTN_Q_PRESCALED
    a.n_groups, a.uniform_mass, a.mass = uniform_mass.numel(), uniform_mass.data_ptr(), mass.data_ptr()
    if probs is not None:
        a.probs, a.row0, a.n_rows = probs.data_ptr(), row0, probs.shape[2]
    return a


def launch_forward(a: AttnFwdArgs, ops: AttnOperands, fp8=None):
    """mca_attn_fwd on fwd_args' struct; fp8 (hip.AttnFp8Operands): quantise q, k, v into it and run mca_attn_fwd_fp8"""
    flops = 4.0 * 64 * ops.sched_f.s.allowed_pairs * a.heads * a.batch
    hip.set_tag("pool" if a.nq != a.nk else "layer")
    if fp8 is not None:
        call("mca_attn_quant_mxfp8", a.q, a.q_bstride, a.q_ld, a.k, a.v, a.kv_bstride, a.kv_ld, C.byref(fp8), a.batch, a.heads, a.nk, stream_ptr())
        call("mca_attn_fwd_fp8", C.byref(a), C.byref(fp8), stream_ptr(), flops=flops)
    elif ops.hstride:
        call("mca_attn_fwd_hm", C.byref(a), C.byref(layout_args(ops)), stream_ptr(), flops=flops, profile_as="mca_attn_fwd")
    else:
        call("mca_attn_fwd", C.byref(a), stream_ptr(), flops=flops)
    hip.set_tag("")


def backward_twopass(ops: AttnOperands, grads: AttnGrads, keys: AttnKeys, dvmean: torch.Tensor, fp8=None, fp8_which: int = 0):
    """mca_attn_bwd_prep + the dkv and dq passes (attention_bwd2.hip): dq (bf16 or fp32) is WRITTEN, not accumulated.  fp8
    (hip.AttnFp8BwdOperands): the passes with fp8 score recomputes (attention_fp8.hip) after mca_attn_quant_bwd_mxfp8 has
    quantised the operands fp8_which names."""
    o, b, H = ops.o, keys.batch, keys.heads
    call("mca_attn_bwd_prep", o.data_ptr(), grads.d_o.data_ptr(), ops.nq * o.stride(0), o.stride(0), ops.lse.data_ptr(),
         grads.delta.data_ptr(), dvmean.data_ptr(), b, H, ops.nq, keys.nk, stream_ptr())
    a = bwd2_args(ops, grads, keys, dvmean)
    # algorithmic flops of the whole backward (2 x forward) split 3 : 5 over the passes by their share of the five
    # products a one-pass backward needs (dq pass: S, dP, dQ minus the recomputed S, dP counted once)
    flops = 8.0 * 64 * ops.sched_b.s.allowed_pairs * H * b
    hip.set_tag("pool" if ops.nq != keys.nk else "layer")
    if fp8 is not None:
        call("mca_attn_quant_bwd_mxfp8", a.q, a.q_bstride, a.q_ld, a.k, a.v, a.kv_bstride, a.kv_ld, a.d_o, a.o_bstride, a.o_ld,
             C.byref(fp8), fp8_which, b, H, keys.nk, stream_ptr())
        call("mca_attn_bwd_dkv_fp8", C.byref(a), C.byref(fp8), stream_ptr(), flops=flops * 0.6)
        call("mca_attn_bwd_dq_fp8", C.byref(a), C.byref(fp8), stream_ptr(), flops=flops * 0.4)
    else:
        call("mca_attn_bwd_dkv", C.byref(a), stream_ptr(), flops=flops * 0.6)
        call("mca_attn_bwd_dq", C.byref(a), stream_ptr(), flops=flops * 0.4)
    hip.set_tag("")


def backward_onepass(ops: AttnOperands, grads: AttnGrads, keys: AttnKeys, sched: "_OnePassSched", rowc: torch.Tensor,
                     dq_acc: torch.Tensor, dvmean: torch.Tensor, q_hm: torch.Tensor, do_hm: torch.Tensor, split: int):
    """one-pass backward of the layer attention (attention_bwd1.hip): dq, dk, dv bf16, every element written.  Its prep launch
    writes the row constants, dvmean and the head-major packed copies q_hm / do_hm the kernel reads."""
    n, H, b, o = keys.nk, keys.heads, keys.batch, ops.o
    call("mca_attn_bwd_prep_onepass", o.data_ptr(), grads.d_o.data_ptr(), n * o.stride(0), o.stride(0), ops.lse.data_ptr(),
         sched.row_slot.data_ptr(), rowc.data_ptr(), dvmean.data_ptr(), b, H, n, sched.n_qt, ops.q, ops.q_bstride, ops.q_ld,
         q_hm.data_ptr(), do_hm.data_ptr(), stream_ptr())
    a = bwd1_args(ops, grads, keys, sched, rowc, dq_acc, dvmean, split,
                  RowSource(q_hm.data_ptr(), H * n * 64, n * 64, 64), RowSource(do_hm.data_ptr(), H * n * 64, n * 64, 64))
    hip.set_tag("layer")
    call("mca_attn_bwd_onepass", C.byref(a), stream_ptr(), flops=8.0 * 64 * sched.s.allowed_pairs * H * b)
    hip.set_tag("")


def backward_onepass_hm(ops: AttnOperands, grads: AttnGrads, keys: AttnKeys, sched: "_OnePassSched", rowc: torch.Tensor,
                        dq_acc: torch.Tensor, dvmean: torch.Tensor, split: int):
    """backward_onepass on head-major operands (ops.hstride, grads.do_hstride: what mca_gemm_nt_cb wrote): the kernel reads q and
    dO in place, the prep launch writes the row constants and dvmean only.  Timed under the entry points it replaces."""
    assert ops.hstride and grads.do_hstride and ops.q_ld == 64 and ops.kv_ld == 64, "head-major operands only"
    n, H, b, o = keys.nk, keys.heads, keys.batch, ops.o
    call("mca_attn_bwd_prep_onepass_hm", o.data_ptr(), n * o.stride(0), o.stride(0), grads.d_o.data_ptr(), n * 64, grads.do_hstride, 64,
         ops.lse.data_ptr(), sched.row_slot.data_ptr(), rowc.data_ptr(), dvmean.data_ptr(), b, H, n, sched.n_qt, stream_ptr(),
         profile_as="mca_attn_bwd_prep_onepass")
    a = bwd1_args(ops, grads, keys, sched, rowc, dq_acc, dvmean, split, RowSource(ops.q, ops.q_bstride, ops.hstride, 64),
                  RowSource(grads.d_o.data_ptr(), n * 64, grads.do_hstride, 64))
    hip.set_tag("layer")
    call("mca_attn_bwd_onepass_hm", C.byref(a), C.byref(layout_args(ops)), stream_ptr(), flops=8.0 * 64 * sched.s.allowed_pairs * H * b,
         profile_as="mca_attn_bwd_onepass")
    hip.set_tag("")


def _dev(a: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


class _Sched:
    """device copies of a TileSchedule"""

    def __init__(self, s, device):
        self.s = s
        # tile index with the "structurally full" flag in bit 31: one scalar load per tile in the kernels
        pack = lambda idx, full: (idx.astype(np.uint32) | (full.astype(np.uint32) << 31)).view(np.int32)
        self.q_ptr, self.q_kt, self.q_order = _dev(s.q_ptr, device), _dev(pack(s.q_kt, s.q_full), device), _dev(s.q_order, device)
        self.k_ptr, self.k_qt, self.k_order = _dev(s.k_ptr, device), _dev(pack(s.k_qt, s.k_full), device), _dev(s.k_order, device)
        # per launch slot of the backward: {key block, first entry, number of entries, query tile of the first entry}
        wg = np.zeros((len(s.k_order), 4), np.int32)
        for i, kb in enumerate(s.k_order):
            lo, hi = int(s.k_ptr[kb]), int(s.k_ptr[kb + 1])
            wg[i] = (kb, lo, hi - lo, int(s.k_qt[lo]) if hi > lo else 0)
        self.k_wg = _dev(wg, device)


class _OnePassSched:
    """device copies of a structure.OnePassSchedule (mca_attn_bwd_onepass)"""

    def __init__(self, s, device):
        self.s = s
        self.qt_desc, self.kb_desc = _dev(s.qt_desc.astype(np.int32), device), _dev(s.kb_desc.astype(np.int32), device)
        self.kb_qt = _dev(s.kb_qt.astype(np.uint32).view(np.int32), device)
        self.visit, self.row_slot = _dev(s.visit.astype(np.uint8), device), _dev(s.row_slot.astype(np.int32), device)
        self.n_qt, self.n_kb, self.max_list = len(s.qt_desc), len(s.kb_desc), int(s.kb_desc[:, 3].max())
        self.n_entries = int(len(s.kb_qt))
        self.fits = self.n_qt < 256 and self.n_kb <= 64 and self.max_list + 6 <= 256 and self.n_entries + 4 * self.n_kb <= 768          # the kernel's LDS tables
