"""Host side of the attention launches: which backward form runs (ONE pure function, backward_plan), the operand records the
engine's launchers take, and the device copies of the tile schedules.  Imports without a GPU and without loading the library.

The layer attention's backward has three forms: the bf16 one-pass kernel (attention_bwd1.hip), the two-pass kernels with bf16
score recomputes (attention_bwd2.hip) and the two-pass kernels with fp8 score recomputes (attention_fp8.hip).  The pooling
attention (fp32 dq, nq != nk) always takes the bf16 two-pass form."""
from __future__ import annotations

from typing import Any, NamedTuple, Optional

import numpy as np
import torch

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
