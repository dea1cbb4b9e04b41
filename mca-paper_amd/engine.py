"""FusionEngine: drives the HIP kernels for one MCA/MMA training step (forward, loss, backward).

Data layout in HBM (b = per-GPU batch, N = tokens per sample, D = 512, H = 8, Ip = FF inner dim padded to
a multiple of 64):
  * parameters and gradients: two flat fp32 buffers ordered by BACKWARD COMPLETION (loss/pool first,
    encoders last) so that gradient buckets for the RCCL all-reduce are contiguous prefixes;
  * bf16 copies of every weight (plain and transposed, zero-padded to MFMA-friendly shapes), refreshed
    once per optimizer step;
  * residual stream fp32 (b*N, D) per layer (LayerNorm inputs are kept for the backward); every GEMM
    operand bf16; q|k|v packed as one (b*N, 3D) bf16 matrix written by a single fused QKV GEMM;
  * nothing of size N x N exists: the attention kernels recompute scores from q, k and a (b,H,N) fp32
    log-sum-exp.

Reference lines: forward model.py:448-478, layer algebra :117-122, pooling :470-473, loss :175-233,
encoders encoders.py:196-214 / :90-96, backward = autograd of those (train_accel_gpu.py:115).
"""
from __future__ import annotations

import os

import ctypes as C
import weakref
import math
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from . import attention, hip
from .attention import AttnGrads, AttnKeys, AttnOperands, _OnePassSched, _Sched, _dev
from .encoder_steps import FLAG_INDEX_RANGE, step_for
from .hip import AttnFp8BwdOperands, AttnFp8Operands, LossTerm, call, ptr, stream_ptr

LN_EPS = 1e-5
FWD_BQ, FWD_BK = 128, 64
BWD_BQ = 64          # query rows per step of the dK/dV pass (its key-block size: debug_options()['dkv_keys'])


FLAG_CACHE_MISMATCH = 8          # the engine's flag word (encoder_steps.FLAG_INDEX_RANGE lists bits 1, 2, 4): cached.CachedStep(verify=True)


def _pad_to(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def debug_options() -> dict:
    """The engine's A/B switches, all behind ONE environment variable: ``MCA_DEBUG=key=value,key=value``.  Production runs set
    none of them.  overlap_wgrad=0|1 (weight-gradient GEMMs on a side stream: default by size), group_wgrad=0 (one launch per
    weight gradient instead of one per layer), mask_mfma=0 (element-wise attention mask instead of the mask product),
    dkv_keys=256 (8-wavefront key blocks in the dK/dV pass), lazy_softmax=0 (the textbook running-maximum recurrence in the forward
    attention instead of MCA_ATTN_LAZY_REFERENCE, the default since round 5: -9 % on that kernel, statistically indistinguishable
    from the textbook form over 8 data seeds, profiles/r05_lazy_softmax_seed_study.txt), deterministic=1 (the fixed-order forms of
    the weight-gradient, LayerNorm-backward, row-reduction and table-gradient launches: FusionEngine.set_deterministic),
    geglu_saved=0 (the FF1 GEMM keeps h = [a | gate] and the backward evaluates gelu again, instead of the saved factors:
    FusionEngine.geglu_saved_factors), ln_rows=0 (the trunk LayerNorm backward as a launch of its own behind the data-gradient
    GEMM instead of in that GEMM's full-row epilogue: FusionEngine.fuse_ln_rows), ln_rows_tall=0 (that fused launch always with
    128-row tiles, mca_gemm_nt_res_lnbwd, instead of 160-row tiles where they save a round of workgroups:
    FusionEngine.ln_rows_tall), qkv_hm=0 (q | k | v and dO always as row-major
    matrices, with the one-pass backward's packed copies, instead of head-major from their GEMMs: FusionEngine.qkv_head_major).
    Kernel-level knobs: include/mca_hip_debug.h (hip.knobs)."""
    opts = {"overlap_wgrad": None, "group_wgrad": True, "mask_mfma": True, "dkv_keys": 128, "lazy_softmax": True,
            "onepass": None, "deterministic": False, "geglu_saved": True, "ln_rows": True, "ln_rows_tall": True,
            "qkv_hm": True}          # onepass=0|1: the one-pass attention backward (attention_bwd1.hip); default: by size
    for item in filter(None, os.environ.get("MCA_DEBUG", "").split(",")):
        k, _, v = item.partition("=")
        k = k.strip()
        if k not in opts:
            raise ValueError(f"MCA_DEBUG: unknown switch '{k}' (known: {sorted(opts)})")
        opts[k] = int(v) if k == "dkv_keys" else (v.strip() not in ("0", "", "false"))
    return opts


def _ln_bwd_args(dy, ldy, x, gamma, mean, rstd, rows, cols, dgamma, dbeta=None, rowmask=None, dx=None, dx_bf16=None,
                 y_bstride=0, period=0, dxsum=None):
    """mca_layernorm_bwd's arguments up to the stream"""
    return (ptr(dy), ldy, y_bstride, period, ptr(x), x.stride(0), ptr(gamma), ptr(mean), ptr(rstd),
            ptr(rowmask), ptr(dx), dx.stride(0) if dx is not None else 0, ptr(dx_bf16),
            dx_bf16.stride(0) if dx_bf16 is not None else 0, ptr(dgamma), ptr(dbeta), ptr(dxsum), rows, cols)


class FusionEngine:
    def __init__(self, model):
        self.model = model
        p0 = next(model.parameters())
        # EAO baseline (model.EAO): segments instead of fusion tokens, mean pooling instead of attentive pooling
        self.eao = model.attn_pool is None
        if p0.device.type != "cuda":
            raise hip.MCAHipError("the MCA step runs only on a HIP device: move the model to cuda first "
                                  "(there is no CPU fallback)")
        hip.lib()                                   # fail loudly if the extension is missing
        self.device = p0.device
        self.D, self.H, self.L = model.dim, model.heads, model.depth
        st = model.structure
        self.st = st
        self.N, self.R, self.F, self.M = st.n_tokens, st.n_return, st.num_fusion_tokens, st.n_modalities
        if self.D != self.H * 64:
            raise NotImplementedError("native path needs dim == heads * 64")
        self.I = model.layers[0].ff.inner_dim if self.L else int(self.D * 4 * 2 / 3)
        self.Ip = _pad_to(self.I, 64)
        self.scale = model.dim_head ** -0.5
        self.q_scale = self.scale * 1.4426950408889634          # folded into the forward bf16 copy of every to_q.weight
        self.attn_flags = hip.ATTN_Q_PRESCALED                  # (the kernels take pre-scaled q only)
        self.attn_dtype = "bf16"
        self.dbg = debug_options()                               # A/B switches: ONE environment variable, MCA_DEBUG
        if self.dbg["lazy_softmax"]:
            self.attn_flags |= hip.ATTN_LAZY_REFERENCE
        self.nk_pad = _pad_to(self.N, 256)
        # the attention mask as a matrix product (mca_build_keyhot): needs every key group id <= 14
        self.mask_mfma = int(self.st.kgroup.max()) <= 14 and self.dbg["mask_mfma"]
        self._flatten_parameters()
        self._build_static()
        # one step object per modality (encoder_steps.py): everything that depends on the encoder's kind, its bf16 weight copies included
        self.enc_steps = [step_for(self, name, mi, model.encoders[name]) for mi, name in enumerate(model.modality_types)]
        self._alloc_weights()
        self._ws: Dict[int, dict] = {}
        self._weights_version = -1
        self.grad_bucket_hook: Optional[Callable[[int, int], None]] = None   # (lo, hi) offsets ready
        self.gather_hook: Optional[Callable] = None                          # DP: pooled/present all-gather
        # Finite checks of the reference (encoders.py:197-213) without its host syncs: the kernels OR bits into one device
        # word; the host reads it once per step through a pinned mirror.  check_finite: True = raise inside the forward that
        # saw the bad values (one sync per forward, the reference's behaviour); "deferred" = no sync: poll_finite() /
        # assert_finite() raise afterwards, and FusedAdamW skips the update of a flagged step on the device; False = off.
        self.check_finite = True
        self.finite_flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._flag_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._flag_event: Optional[torch.cuda.Event] = None
        self.fuse_geglu_bwd = True
        # The FF1 epilogue stores the two factors of the GEGLU backward, s = [gelu(gate) | a * gelu'(gate)], where h = [a | gate]
        # would go (mca_gemm_nt_geglu_fwd_saved), and the fused backward only multiplies by them.  Read once per forward
        # (forward_trunk), and only with fuse_geglu_bwd: the unfused backward reads the true h.  What a layer's buffer holds is
        # recorded on its workspace (a["h_holds"]) and asserted by the backward.
        self.geglu_saved_factors = bool(self.dbg["geglu_saved"])
        self._mod_shifts = torch.arange(len(model.modality_types), dtype=torch.int32, device=self.device)
        self.fuse_ln_residual = True                # residual LayerNorm recomputed in the GEMM epilogue (large batches)
        # The trunk LayerNorm backward inside the data-gradient GEMM that produces its dy (mca_gemm_nt_res_lnbwd: a workgroup owns
        # whole rows, dy never reaches memory).  Where it applies: ln_rows_backward.
        self.fuse_ln_rows = bool(self.dbg["ln_rows"])
        # ... through the entry point that picks 160-row tiles where they save a round of workgroups: ln_rows_tall_form.
        self.ln_rows_tall = bool(self.dbg["ln_rows_tall"])
        # q | k | v and dO written head-major by their GEMMs (mca_gemm_nt_cb) and read in place by the attention kernels, where the
        # one-pass backward runs: qkv_head_major decides once per forward.  rows_only: a forward whose q | k are read afterwards
        # by code that takes row-major matrices only (the attention readout) keeps the row-major layout.
        self.rows_only = False
        # Weight-gradient GEMMs on a side stream, concurrent with the backward chain: None = by size (on below OVERLAP_ROWS_MAX
        # token rows).  Since the attention backward lost its atomics the main stream keeps every CU busy and the persistent
        # weight-gradient GEMMs of a second stream only take CUs from it (one box, alternating processes: 23.7 / 25.6 ms per
        # b = 32 step with the side stream, 22.17 / 22.16 without); at small batches (b = 8: the N = 512 GEMMs fill 160 of 256
        # CUs) the side stream still pays in the eager loop (8.7-8.8 against 9.5-10.2 ms).  MCA_DEBUG=overlap_wgrad=0|1 forces it.
        self.overlap_wgrad = self.dbg["overlap_wgrad"]
        self.group_wgrad = self.dbg["group_wgrad"]          # one weight-gradient launch per layer
        # Deterministic mode: every parameter gradient that is a sum over token rows is added in a fixed order
        # (the *_det entry points of include/mca_hip.h), so a step is the same bits every time.  Off by default.
        self._deterministic = bool(self.dbg["deterministic"])
        self._captured = weakref.WeakSet()                  # live graph.GraphedStep objects: they replay the mode they captured
        # Per-step modality dropout (set_modality_dropout): the settings, the step counter (one int64 word on the device, read by
        # mca_pack_masks_drop and advanced by mca_counter_add inside the step) and this process' data-parallel rank, which places
        # its local samples in the global batch (dp.DataParallelMCA.install)
        self._mdrop: Optional[dict] = None
        self._mdrop_counter: Optional[torch.Tensor] = None
        self.dropout_rank = 0

    # ------------------------------------------------------------------------------------------------
    # parameters -> one flat buffer (and one for gradients)
    # ------------------------------------------------------------------------------------------------
    def _flatten_parameters(self):
        m = self.model
        order: List[torch.nn.Parameter] = []
        marks: List[int] = []                        # bucket boundaries (indices into `order`)
        order += [m.loss.loss_fn.logit_scale]
        # the pooling key/value projection's gradient is reduced over all T token rows: it rides in the top layer's grouped
        # weight-gradient launch (_backward_layers_and_encoders) and therefore belongs to that layer's bucket
        pool_kv_late = not self.eao and self.L > 0
        if not self.eao:
            order += [m.return_tokens, m.attn_pool.to_out.weight, m.attn_pool.to_q.weight]
            if not pool_kv_late:
                order += [m.attn_pool.to_kv.weight]
        order += [m.norm.gamma]
        marks.append(len(order))
        if pool_kv_late:
            order += [m.attn_pool.to_kv.weight]
        for i in reversed(range(self.L)):
            ly = m.layers[i]
            order += [ly.ff.feedforward[2].weight, ly.ff.feedforward[0].weight, ly.attn.to_out.weight,
                      ly.attn.to_q.weight, ly.attn.to_kv.weight, ly.norm.gamma]
            marks.append(len(order))
        if not self.eao:
            order.append(m.fusion_tokens)
        for name in m.modality_types:
            order += list(m.encoders[name].parameters())
        marks.append(len(order))
        seen = {id(p) for p in order}
        for p in m.parameters():
            if id(p) not in seen:
                order.append(p)
        marks[-1] = len(order)
        offs, n = [], 0
        for p in order:
            n = _pad_to(n, 4)                        # keep every tensor 16-byte aligned
            offs.append(n)
            n += p.numel()
        total = _pad_to(n, 4)
        flat = torch.zeros(total, dtype=torch.float32, device=self.device)
        gflat = torch.zeros(total, dtype=torch.float32, device=self.device)
        self.param_views, self.grad_views = {}, {}
        for p, o in zip(order, offs):
            if p.dtype != torch.float32:
                raise TypeError("parameters must be fp32 (bf16 is used for GEMM operands only)")
            flat[o:o + p.numel()].copy_(p.data.reshape(-1))
            p.data = flat[o:o + p.numel()].view(p.shape)
            self.grad_views[id(p)] = gflat[o:o + p.numel()].view(p.shape)
        self.flat, self.gflat = flat, gflat
        self.param_order, self.param_offsets = order, offs
        self.bucket_bounds = [offs[i] if i < len(offs) else total for i in marks]
        self.bucket_bounds[-1] = total
        self.n_params = total

    def grad_of(self, p) -> torch.Tensor:
        return self.grad_views[id(p)]

    # ------------------------------------------------------------------------------------------------
    def _build_static(self):
        st, dev = self.st, self.device
        self.kgroup = _dev(st.kgroup.astype(np.uint8), dev)
        self.qmask_attn = _dev(st.qmask_attn.astype(np.uint32).view(np.int32), dev)
        self.qmask_pool = _dev(st.qmask_pool.astype(np.uint32).view(np.int32), dev)
        # query side of the mask product (mca_hip.h, mca_build_keyhot): qblk[i][g] = group g visible ? 0 : -32768, slot 15 blocked
        def qblk_of(qm):
            bits = (qm.astype(np.uint32)[:, None] >> np.arange(16, dtype=np.uint32)[None, :]) & 1
            bits[:, 15] = 0
            return torch.from_numpy(np.where(bits == 1, 0.0, -32768.0).astype(np.float32)).to(torch.bfloat16).to(dev).contiguous()
        self.qblk_attn, self.qblk_pool = qblk_of(st.qmask_attn), qblk_of(st.qmask_pool)
        self.sched_attn_f = _Sched(st.attn_schedule(FWD_BQ, FWD_BK), dev)
        # key-block size of the dkv pass: 128 (4 wavefronts, two independent workgroups per CU) is 3 % faster than 256 (8 wavefronts,
        # one workgroup per CU) at N = 2538 and equal at N = 6088
        dkv_keys = self.dbg["dkv_keys"]
        self.dkv_keys = dkv_keys
        self.sched_attn_b2 = _Sched(st.attn_schedule(BWD_BQ, dkv_keys), dev)
        # one-pass backward of the layer attention: needs the mask product and tables that fit the kernel's LDS
        self.sched_onepass = None
        if self.mask_mfma and self.dbg["onepass"] is not False:
            sc = _OnePassSched(st.attn_onepass_schedule(aligned=True), dev)
            self.sched_onepass = sc if sc.fits else None
        if self.eao:
            self.seg_start = _dev(st.seg_start, dev)
        else:
            self.sched_pool_f = _Sched(st.pool_schedule(FWD_BQ, FWD_BK), dev)
            self.sched_pool_b2 = _Sched(st.pool_schedule(BWD_BQ, dkv_keys), dev)
        terms = self.model.loss_terms
        arr = (LossTerm * len(terms))()
        for i, t in enumerate(terms):
            arr[i] = LossTerm(t.slot_a, t.slot_b, t.and_bits, t.or_bits)
        self.n_terms = len(terms)
        self.loss_terms_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        self.offsets = np.concatenate([[0], np.cumsum(st.token_dims)]).astype(int).tolist()

    # ------------------------------------------------------------------------------------------------
    # bf16 weight copies
    # ------------------------------------------------------------------------------------------------
    def _alloc_weights(self):
        D, Ip, dev = self.D, self.Ip, self.device
        bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=dev)
        self.wl = []
        for _ in range(self.L):
            self.wl.append(dict(qkv=bf(3 * D, D), qkvT=bf(D, 3 * D), o=bf(D, D), oT=bf(D, D),
                                w1=bf(2 * Ip, D), w1T=bf(D, 2 * Ip), w2=bf(D, Ip), w2T=bf(Ip, D)))
        self.wp = dict(q=bf(D, D), qT=bf(D, D), kv=bf(2 * D, D), kvT=bf(D, 2 * D), o=bf(D, D), oT=bf(D, D))

    def _cast(self, src: torch.Tensor, dst: torch.Tensor, transpose=False, dst_row0=0, dst_col0=0, scale=0.0):
        """dst[dst_row0:, dst_col0:] (bf16) <- src (fp32 2-D), zero padding untouched (buffers start zeroed).  Only
        RECORDS the copy: all of them run as one multi-tensor launch (the parameter / copy addresses never change)."""
        r, c = src.shape
        d = dst[dst_row0:, dst_col0:]
        rp, cp = (c, r) if transpose else (r, c)
        self._cast_list.append(hip.CastDesc(ptr(src), ptr(d), src.stride(0), r, c, dst.stride(0), rp, cp, int(transpose), float(scale)))

    @property
    def deterministic(self) -> bool:
        return self._deterministic

    def set_deterministic(self, on: bool):
        """Deterministic mode on / off from the next step on.  A captured step replays the launches of the mode it was captured
        in, so the mode cannot change while a GraphedStep of this engine is alive."""
        on = bool(on)
        if on == self._deterministic:
            return
        if len(self._captured):
            raise RuntimeError("set_deterministic: a GraphedStep captured with deterministic="
                               f"{self._deterministic} is alive and would go on replaying that mode; delete it first")
        self._deterministic = on
        if on:
            for ws in self._ws.values():
                if isinstance(ws, dict) and "T" in ws:
                    self._alloc_det_scratch(ws)

    @property
    def modality_dropout(self) -> Optional[dict]:
        """the active per-step modality dropout, {"rates": {name: p}, "seed", "keep_one"}, or None"""
        s = self._mdrop
        return None if s is None else dict(rates=dict(s["rates"]), seed=s["seed"], keep_one=s["keep_one"])

    def modality_dropout_step(self) -> int:
        """the device step counter of the modality dropout: the t of the next draw.  Synchronises (tests, resume)."""
        return 0 if self._mdrop_counter is None else int(self._mdrop_counter.item())

    def set_modality_dropout(self, rates, seed: int = 42, keep_one: bool = True, step: int = 0):
        """Per-step modality dropout, drawn on the device inside the step (mca_pack_masks_drop, include/mca_hip.h): every training
        forward with a loss drops modality `name` of a sample with probability rates[name] (names not given: 0), a fresh draw per
        (global sample, modality, step); keep_one rescues one modality of a sample that would lose all it has.  Eval, no_loss and
        model.eval() forwards never drop and do not advance the step.  rates None or all zero switches it off.  `step` sets the
        device counter (a resumed run passes its optimizer step count).  A captured step holds the launches and their by-value
        arguments, so nothing here can change while a GraphedStep of this engine is alive."""
        names = list(self.model.modality_types)
        rates = dict(rates or {})
        for k in rates:
            if k not in names:
                raise KeyError(f"set_modality_dropout: unknown modality '{k}' (known: {names})")
        p = {n: float(rates.get(n, 0.0)) for n in names}
        for n, v in p.items():
            if not 0.0 <= v <= 1.0:          # (NaN fails both comparisons)
                raise ValueError(f"set_modality_dropout: rate of '{n}' is {v}, not in [0, 1]")
        on = any(v > 0.0 for v in p.values())
        if on and not self.can_forward_backward():
            raise NotImplementedError("set_modality_dropout needs native encoders (a torch encoder writes its padding itself)")
        if len(self._captured):
            raise RuntimeError("set_modality_dropout: a GraphedStep of this engine is alive and would go on replaying the "
                               "launches it captured; delete it first")
        if on and self._mdrop_counter is None:
            self._mdrop_counter = torch.zeros(1, dtype=torch.int64, device=self.device)          # allocated once: the capture holds its address
        if self._mdrop_counter is not None:
            self._mdrop_counter.fill_(int(step))
        self._mdrop = dict(rates=p, seed=int(seed) & 0xFFFFFFFFFFFFFFFF, keep_one=bool(keep_one)) if on else None

    def set_attention_dtype(self, dtype: str):
        """'bf16' (default) or 'fp8' (BASELINE configs[4]): the fusion layers' forward attention computes Q K^T and P V on the
        block-scaled fp8 matrix instruction from MX-fp8 copies of q, k, v (one quantisation pass per layer,
        mca_attn_quant_mxfp8), and their backward recomputes S = Q K^T and dP = dO V^T on it (mca_attn_quant_bwd_mxfp8 +
        mca_attn_bwd_dq_fp8 / mca_attn_bwd_dkv_fp8; the three gradient products stay bf16; needs the mask product and
        128-key dkv blocks, else the backward keeps bf16 recomputes).  Pooling attention stays bf16."""
        if dtype not in ("bf16", "fp8"):
            raise ValueError(dtype)
        self.attn_dtype = dtype

    def _fp8_operands(self, ws, b, layer):
        """MX-fp8 forward operands: q8 / k8 (+ scales) PER LAYER (the backward's score recomputes read them again: 2 x 1.03 bytes
        per q / k element and layer, 4 GB at configs[4]'s b = 128), one shared V^T set (forward only)"""
        key = ("fp8", layer)
        if key not in ws:
            nt = (self.N + 63) // 64
            u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=self.device)
            if "fp8v" not in ws:
                ws["fp8v"] = dict(v8t=u8(b, self.H, nt, 64, 64), vs=u8(b, self.H, nt, 64, 2))
            bufs = dict(q8=u8(b, self.H, nt * 64, 64), qs=u8(b, self.H, nt * 64, 2), k8=u8(b, self.H, nt * 64, 64), ks=u8(b, self.H, nt * 64, 2),
                        **ws["fp8v"])
            f = AttnFp8Operands()
            f.q8, f.qs, f.k8, f.ks, f.v8t, f.vs = (bufs[k].data_ptr() for k in ("q8", "qs", "k8", "ks", "v8t", "vs"))
            f.n_ktiles = nt
            ws[key] = (bufs, f)
        return ws[key]

    def _fp8_bwd_operands(self, ws, b, layer):
        """MX-fp8 backward operands of a layer: q8 / k8 are the arrays its forward wrote (same bits as a re-quantisation), v and
        dO (quantised along d) share one set of buffers across layers.  -> (operands, which-mask for mca_attn_quant_bwd_mxfp8)"""
        key = ("fp8b", layer)
        if key not in ws:
            nt = (self.N + 63) // 64
            u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=self.device)
            if "fp8bv" not in ws:
                ws["fp8bv"] = {**{k: u8(b, self.H, nt * 64, 64) for k in ("v8", "do8")}, **{k: u8(b, self.H, nt * 64, 2) for k in ("vs", "dos")}}
            fwd = self._fp8_operands(ws, b, layer)[0]
            bufs = {**{k: fwd[k] for k in ("q8", "qs", "k8", "ks")}, **ws["fp8bv"]}
            f = AttnFp8BwdOperands()
            for k in ("q8", "qs", "k8", "ks", "v8", "vs", "do8", "dos"):
                setattr(f, k, bufs[k].data_ptr())
            f.n_ktiles = nt
            ws[key] = (bufs, f)
        # q8 / k8 hold this step's q, k only if THIS forward quantised them (a forward run in bf16 leaves them stale)
        fresh = ws.get(("fp8gen", layer)) == ws["gen"]
        return ws[key][1], (0b1100 if fresh else 0b1111)

    def backward_plan(self, ws, b, nq, dq_f32=False) -> attention.Plan:
        """attention.backward_plan for an attention with nq query rows at batch b: the ONLY place the engine decides the backward
        form.  The mask product is a property of the workspace (ws = None: of the workspace this engine would build); the
        MCA_DEBUG switch is read now, not at construction."""
        sc = self.sched_onepass
        return attention.backward_plan(
            attn_dtype=self.attn_dtype, mask_product=self.mask_mfma if ws is None else ws.get("khot") is not None,
            onepass_tables_fit=sc is not None, onepass_want=self.dbg["onepass"], dkv_keys=self.dkv_keys, b=b, heads=self.H,
            n_kblocks=sc.n_kb if sc is not None else 1, layer_attention=nq == self.N, dq_f32=dq_f32)

    def backward_form(self, b) -> str:
        """what the layer attention's backward runs at batch b (reported by bench.py)"""
        return attention.describe(self.backward_plan(None, b, self.N))

    def fp8_backward_on(self, ws, nq) -> bool:
        return self.backward_plan(ws, ws["b"], nq).form == "fp8-twopass"

    def invalidate_weights(self):
        """Call after writing parameters through an alias autograd's version counters cannot see (``p.data.op_()``, a raw
        pointer): the bf16 GEMM-weight copies are rebuilt by the next forward."""
        self._weights_version = -1

    def _param_version(self) -> int:
        # every Parameter is a view of `flat` with its OWN version counter (p.data = flat[...]): load_state_dict, p.copy_,
        # torch.optim steps and dist.broadcast(p) bump the parameter's counter, FusedAdamW / broadcast(flat) bump flat's
        return self.flat._version + sum(p._version for p in self.param_order)

    def refresh_weights(self, force=False):
        v = self._param_version()
        if not force and v == self._weights_version:
            return
        if getattr(self, "_cast_table", None) is not None:
            call("mca_cast_pad_bf16_multi", ptr(self._cast_table), self._cast_n, stream_ptr())
            self._weights_version = v
            return
        self._cast_list = []
        m, D, I, Ip = self.model, self.D, self.I, self.Ip
        for i, ly in enumerate(m.layers):
            w = self.wl[i]
            # forward copy of W_q carries scale * log2(e): q.k comes out of the QKV GEMM as the log2-domain logit (the
            # transposed copies used by the backward data-gradient GEMMs stay unscaled: mca_hip.h, MCA_ATTN_Q_PRESCALED)
            self._cast(ly.attn.to_q.weight.data, w["qkv"], scale=self.q_scale)
            self._cast(ly.attn.to_kv.weight.data, w["qkv"], dst_row0=D)
            self._cast(ly.attn.to_q.weight.data, w["qkvT"], transpose=True)
            self._cast(ly.attn.to_kv.weight.data, w["qkvT"], transpose=True, dst_col0=D)
            self._cast(ly.attn.to_out.weight.data, w["o"])
            self._cast(ly.attn.to_out.weight.data, w["oT"], transpose=True)
            w1 = ly.ff.feedforward[0].weight.data
            self._cast(w1[:I], w["w1"])
            self._cast(w1[I:], w["w1"], dst_row0=Ip)
            self._cast(w1[:I], w["w1T"], transpose=True)
            self._cast(w1[I:], w["w1T"], transpose=True, dst_col0=Ip)
            w2 = ly.ff.feedforward[2].weight.data
            self._cast(w2, w["w2"])
            self._cast(w2, w["w2T"], transpose=True)
        ap = m.attn_pool
        if ap is not None:
            self._cast(ap.to_q.weight.data, self.wp["q"], scale=self.q_scale); self._cast(ap.to_q.weight.data, self.wp["qT"], transpose=True)
            self._cast(ap.to_kv.weight.data, self.wp["kv"]); self._cast(ap.to_kv.weight.data, self.wp["kvT"], transpose=True)
            self._cast(ap.to_out.weight.data, self.wp["o"]); self._cast(ap.to_out.weight.data, self.wp["oT"], transpose=True)
        for s in self.enc_steps:
            s.casts()
        arr = (hip.CastDesc * len(self._cast_list))(*self._cast_list)
        self._cast_n = len(self._cast_list)
        self._cast_table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
        call("mca_cast_pad_bf16_multi", ptr(self._cast_table), self._cast_n, stream_ptr())
        self._weights_version = v

    # ------------------------------------------------------------------------------------------------
    # workspaces for a given local batch size
    # ------------------------------------------------------------------------------------------------
    def workspace(self, b: int) -> dict:
        if b in self._ws:
            return self._ws[b]
        D, N, H, Ip, R, dev = self.D, self.N, self.H, self.Ip, self.R, self.device
        T = b * N
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        bf = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=dev)
        u8 = lambda *s: torch.empty(*s, dtype=torch.uint8, device=dev)
        ws = dict(b=b, T=T, gen=0)
        ws["ln_rows_tall"] = {}          # K -> the fused LayerNorm-backward GEMM of (T, D, K) takes the 160-row entry point (ln_rows_tall_form)
        ws["x"] = [f32(T, D) for _ in range(self.L + 1)]
        ws["layers"] = [dict(x1=f32(T, D), m1=f32(T), r1=f32(T), m2=f32(T), r2=f32(T), xn_b=bf(T, D), qkv=bf(T, 3 * D),
                             o=bf(T, D), lse=f32(b, H, N), x1n_b=bf(T, D), h=bf(T, 2 * Ip), g=bf(T, Ip),
                             # backward operands of the weight-gradient GEMMs: one set PER LAYER, so those GEMMs can run
                             # on a side stream without write-after-read hazards against the next layer's backward
                             dxo_b=bf(T, D), dx1_b=bf(T, D), dh=bf(T, 2 * Ip), dqkv=bf(T, 3 * D),
                             h_holds=None,          # "h" = [a | gate] or "s" = the saved GEGLU factors: set by forward_trunk
                             qkv_hm=False)          # qkv holds [3 H][T][64] (mca_gemm_nt_cb) instead of (T, 3 D): set by forward_trunk
                        for _ in range(self.L)]
        ws["xn"], ws["x1n"] = f32(T, D), f32(T, D)
        ws["mf"], ws["rf"] = f32(T), f32(T)
        ws["t_b"], ws["kvp"] = (None, None) if self.eao else (bf(T, D), bf(T, 2 * D))          # operands of the attentive pooling
        ws["rt_b"], ws["qp"], ws["op"], ws["lse_p"] = bf(R, D), bf(R, D), bf(b * R, D), f32(b, H, R)
        ws["pooled"] = f32(b * R, D)
        if self.eao:
            ws["seg_counts"] = torch.zeros(b, R, dtype=torch.int32, device=dev)
        ws["vmean"], ws["dvmean"], ws["delta"], ws["delta_p"] = torch.zeros(b, D, dtype=torch.float32, device=dev), f32(b, D), f32(b, H, N), f32(b, H, R)
        ws["keyinfo"], ws["kflags"] = u8(b, self.nk_pad), u8(b, (N + 63) // 64)
        ws["khot"] = bf(b, self.nk_pad, 16) if self.mask_mfma else None
        ws["padding"] = u8(b, N)
        ws["present"] = torch.zeros(b, dtype=torch.int32, device=dev)
        ws["present_native"] = torch.zeros(b, dtype=torch.int32, device=dev)
        ws["dropped"] = torch.zeros(b, dtype=torch.int32, device=dev)          # the modality dropout's drop bits (set_modality_dropout)
        # backward
        ws["dxa"], ws["dxb"], ws["dx_b"] = f32(T, D), f32(T, D), bf(T, D)
        ws["dg"] = bf(T, Ip)
        # dO = dx1 Wo: (T, D), or [H][T][64] where the layer's q | k | v are head-major (ws["do_hm"] says which it holds).  64 rows of
        # zeros behind it: the one-pass kernel reads whole 64-row tiles, the last head's last one past its rows
        ws["do_buf"] = torch.zeros(T * D + 64 * 64, dtype=torch.bfloat16, device=dev)
        ws["do"], ws["do_hm"] = ws["do_buf"][:T * D].view(T, D), False
        ws["dpool_b"], ws["dop"], ws["dqp32"], ws["dqp_sum"], ws["dqp_b"] = bf(b * R, D), bf(b * R, D), f32(b * R, D), f32(R, D), bf(R, D)
        ws["dkvp"], ws["drt"] = (None if self.eao else bf(T, 2 * D)), f32(R, D)
        sc = self.sched_onepass
        if sc is not None:          # the one-pass attention backward's buffers, dq_acc sized by the split of this batch
            rc = f32(b, H, sc.n_qt + 1, 2, 64)          # (+ the null tile)
            rc[:, :, :, 0] = float("-inf"); rc[:, :, :, 1] = 0.0          # positions past a tile's rows: -inf | 0 (written once; the prep kernel only touches real rows)
            ws["rowc"] = rc
            ws["dq_acc"] = f32(b * H * self.backward_plan(ws, b, N).split * (sc.n_qt + 1) * 4096)          # (+ the null tile's slot)
            # (the head-major packed copies of q and dO, for a backward on row-major operands: _packed_copies, on first use)
        ws["enc"] = {s.name: s.workspace(b, f32, bf, u8) for s in self.enc_steps}
        ws["side"], ws["side_events"] = torch.cuda.Stream(device=dev), []          # side stream of the weight-gradient GEMMs
        if self._deterministic:
            self._alloc_det_scratch(ws)
        self._ws[b] = ws
        return ws

    # ------------------------------------------------------------------------------------------------
    # deterministic mode: scratch and the *_det launches
    # ------------------------------------------------------------------------------------------------
    def _det_need(self, b: int) -> int:
        """floats of scratch the largest deterministic launch of a b-sample backward needs: the library's size queries over
        every call site of _backward_part and _backward_layers_and_encoders (grouped AND single forms of the weight gradients,
        so the figure holds whatever group_wgrad says) and over every encoder step's det_shapes()"""
        L, D, I, R, F, N, T = hip.lib(), self.D, self.I, self.R, self.F, self.N, b * self.N
        shapes = dict(tn=[(b * R, D, D), (R, D, D), (T, 2 * D, D), (T, D, I), (T, I, D), (T, D, D), (T, 3 * D, D)],
                      ln=[(T, D)], rr=[(b * R, R), (R, R)] + ([(b * F, F)] if F else []), tab=[], emb=[])
        for s in self.enc_steps:
            for kind, more in s.det_shapes(b).items():
                shapes[kind] += more
        need = max(L.mca_gemm_tn_acc_det_scratch(*t) for t in shapes["tn"])
        members = [(3 * D, D), (I, D), (I, D), (D, I), (D, D)]
        for ms in (members, members + [(2 * D, D)]):
            Ns, Ks = (C.c_int64 * len(ms))(*[m[0] for m in ms]), (C.c_int64 * len(ms))(*[m[1] for m in ms])
            need = max(need, L.mca_gemm_tn_acc_group_det_scratch(Ns, Ks, len(ms), T, 0))
        need = max([need] + [L.mca_layernorm_bwd_det_scratch(r, c) for r, c in shapes["ln"]]
                   + [L.mca_reduce_rows_det_scratch(r, p, D) for r, p in shapes["rr"]]
                   + [L.mca_tab_value_bwd_det_scratch(r, D) for r in shapes["tab"]]
                   + [L.mca_embedding_scatter_add_det_scratch(r) for r in shapes["emb"]])
        return int(need)

    def _alloc_det_scratch(self, ws):
        """One region per stream: the weight-gradient GEMMs run on the workspace's side stream beside main-stream LayerNorm
        launches when overlap_on(ws).  Calls on one stream share their region: stream order puts a call's reduce launch before
        the next call's partial stores."""
        if "det" not in ws:
            n = max(self._det_need(ws["b"]), 1)
            ws["det"] = {k: torch.empty(n, dtype=torch.float32, device=self.device) for k in ("main", "side")}

    def _det_scratch(self, ws, need: int):
        reg = ws["det"]["side" if hip._STREAM_CACHE is not None and hip._STREAM_CACHE == ws["side"].cuda_stream else "main"]
        assert need <= reg.numel(), f"deterministic scratch: a launch needs {need} floats, the workspace holds {reg.numel()}"
        return reg

    def _sum_launch(self, ws, name, args, scratch_query, flops=0.0):
        """The one launcher of the six entry points whose result depends on the order of a sum (mca_gemm_tn_acc,
        mca_gemm_tn_acc_group, mca_layernorm_bwd, mca_reduce_rows, mca_tab_value_bwd, mca_embedding_scatter_add).  args: the plain form's arguments up to
        the stream.  Deterministic mode launches <name>_det: the same arguments + (scratch, scratch_floats) before the stream
        (hip.py), the scratch sized by <name>_det_scratch(*scratch_query()): the query's arguments are built in that mode only."""
        if not self._deterministic:
            return call(name, *args, stream_ptr(), flops=flops)
        s = self._det_scratch(ws, getattr(hip.lib(), name + "_det_scratch")(*scratch_query()))
        call(name + "_det", *args, ptr(s), s.numel(), stream_ptr(), flops=flops)

    def _tn(self, ws, A, B, Cgrad, R, N, K):
        """Cgrad[N,K] += A[R,N]^T B[R,K]"""
        self._sum_launch(ws, "mca_gemm_tn_acc", (ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(Cgrad), Cgrad.stride(0), R, N, K),
                         lambda: (R, N, K), flops=2.0 * R * N * K)

    def _tn_group(self, ws, members, R):
        """members: [(A, B, Cgrad, N, K)]: Cgrad[N,K] += A[R,N]^T B[R,K] for every member, one launch (mca_gemm_tn_acc_group)"""
        n = len(members)
        arr = (hip.TnDesc * n)()
        fl = 0.0
        for d, (A, B, Cg, N, K) in zip(arr, members):
            d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.N, d.K = ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(Cg), Cg.stride(0), N, K
            fl += 2.0 * R * N * K
        i64s = lambda k: (C.c_int64 * n)(*[m[k] for m in members])
        self._sum_launch(ws, "mca_gemm_tn_acc_group", (C.byref(arr), n, R), lambda: (i64s(3), i64s(4), n, R, 0), flops=fl)

    def _ln_bwd(self, ws, dy, ldy, x, gamma, mean, rstd, rows, cols, dgamma, **optional):
        """optional: dbeta, rowmask, dx, dx_bf16, y_bstride, period, dxsum (_ln_bwd_args)"""
        self._sum_launch(ws, "mca_layernorm_bwd", _ln_bwd_args(dy, ldy, x, gamma, mean, rstd, rows, cols, dgamma, **optional),
                         lambda: (rows, cols))

    def _reduce_rows(self, ws, src, lds, src_bstride, period, dst, ldd, rows, cols):
        """src, dst: device addresses"""
        self._sum_launch(ws, "mca_reduce_rows", (src, lds, src_bstride, period, dst, ldd, rows, cols),
                         lambda: (rows, period, cols))

    # ------------------------------------------------------------------------------------------------
    # thin kernel wrappers
    # ------------------------------------------------------------------------------------------------
    @staticmethod
    def gemm_nt(A, B, C, M, N, K, bias=None, residual=None, res_period=0):
        """C[M,N] = A[M,K] B[N,K]^T (+bias) (+residual)."""
        if hip.PROFILE is not None:          # live timing (bench.py): one key per problem shape, so an average is over equal launches
            hip.set_tag(f"{M}x{N}x{K}{'' if C.dtype == torch.bfloat16 else ' f32'}{' +res' if residual is not None else ''}")
        call("mca_gemm_nt", ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(C), C.stride(0), int(C.dtype == torch.bfloat16),
             ptr(bias), ptr(residual), residual.stride(0) if residual is not None else 0, res_period, M, N, K, stream_ptr(),
             flops=2.0 * M * N * K)
        if hip.PROFILE is not None:
            hip.set_tag("")

    @staticmethod
    def ln_fwd(x, gamma, rows, cols, mean, rstd, beta=None, rowmask=None, add=None, period=0, y=None, ldy=0, y_bstride=0,
               y_bf16=None, cols_pad=0):
        call("mca_layernorm_fwd", ptr(x), x.stride(0), ptr(gamma), ptr(beta), ptr(rowmask), ptr(add), period,
             ptr(y), ldy, y_bstride, ptr(y_bf16), y_bf16.stride(0) if y_bf16 is not None else 0, cols_pad,
             ptr(mean), ptr(rstd), rows, cols, LN_EPS, stream_ptr())

    @staticmethod
    def ln_bwd(*args, **optional):
        """the plain launch with _ln_bwd_args' parameters, callable without an engine (tools/bench_ln.py); the engine's own launches
        go through _ln_bwd"""
        call("mca_layernorm_bwd", *_ln_bwd_args(*args, **optional), stream_ptr())

    def qkv_head_major(self, ws) -> bool:
        """Whether this forward's QKV GEMMs write q | k | v head-major ([3 H][T][64], mca_gemm_nt_cb) for the attention kernels to read
        in place - and the backward's dx1 Wo GEMM dO likewise - instead of the (T, 3 D) matrix: where the layer attention's
        backward is the one-pass kernel (its prep launch then copies nothing), on bf16 operands, for GEMM shapes the column-blocked
        store exists for under the current knobs, and unless the forward is read out afterwards (rows_only) or MCA_DEBUG=qkv_hm=0.
        Decided once per forward; what a layer's buffer holds is recorded as a["qkv_hm"]."""
        if not self.dbg["qkv_hm"] or self.rows_only or self.attn_dtype != "bf16" or ws.get("present_cur") is None:
            return False          # (present_cur: mean(V) has its head-major form in the presence-bit entry point only)
        T, D = ws["T"], self.D
        if self.backward_plan(ws, ws["b"], self.N).form != "onepass":
            return False
        pl = hip.GemmPlan()
        return all(hip.lib().mca_dbg_plan_gemm_nt_cb(T, n, D, 0, T * 64, 1, C.byref(pl)) == 0 for n in (3 * D, D))

    @staticmethod
    def gemm_nt_cb(A, B, Cbuf, M, N, K):
        """C = A B^T (bf16) as [N / 64][M][64] (mca_gemm_nt_cb), timed in the row of the mca_gemm_nt launch it replaces"""
        if hip.PROFILE is not None:
            hip.set_tag(f"{M}x{N}x{K}")
        call("mca_gemm_nt_cb", ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(Cbuf), M * 64, M, N, K, stream_ptr(), flops=2.0 * M * N * K,
             profile_as="mca_gemm_nt")
        if hip.PROFILE is not None:
            hip.set_tag("")

    def _packed_copies(self, ws):
        """q_hm, do_hm: the packed copies mca_attn_bwd_prep_onepass writes for a one-pass backward on ROW-MAJOR q and dO (+ 64 rows:
        the kernel reads whole 64-row tiles, the last one past its rows).  Allocated on first use: a step that keeps q | k | v and
        dO head-major never needs them."""
        if "q_hm" not in ws:
            n = (ws["b"] * self.H * self.N + 64) * 64
            ws["q_hm"], ws["do_hm_copy"] = (torch.zeros(n, dtype=torch.bfloat16, device=self.device) for _ in range(2))
        return ws["q_hm"], ws["do_hm_copy"]

    def _to_row_major(self, ws, i):
        """Layer i's q | k | v and dO back into their row-major matrices, in place.  Only where the backward form changed between a
        head-major forward and the backward (MCA_DEBUG / engine.dbg switched in between, as the A/B tests do): never in a step."""
        a, T, H = ws["layers"][i], ws["T"], self.H
        if a["qkv_hm"]:
            a["qkv"].copy_(a["qkv"].view(3 * H, T, 64).permute(1, 0, 2).reshape(T, 3 * H * 64))
            a["qkv_hm"] = False
        if ws["do_hm"]:
            ws["do"].copy_(ws["do"].view(H, T, 64).permute(1, 0, 2).reshape(T, H * 64))
            ws["do_hm"] = False

    def layer_attention(self, ws, i):
        """-> (AttnOperands, AttnGrads) of fusion layer i: q | k | v and dq | dk | dv are the column blocks of the packed (T, 3D)
        qkv / dqkv matrices; q | k | v (a["qkv_hm"]) and dO (ws["do_hm"]) head-major where their GEMMs wrote them so"""
        D, N, H, T, a = self.D, self.N, self.H, ws["T"], ws["layers"][i]
        if a["qkv_hm"]:          # [3 H][T][64]: q, k, v are slabs 0, H, 2 H; a (sample, head) is N contiguous 64-element rows
            ops = AttnOperands(a["qkv"].data_ptr(), N * 64, 64, a["qkv"], H * T * 64, 2 * H * T * 64, 64, a["o"], a["lse"], N, self.qmask_attn,
                               self.qblk_attn, self.sched_attn_f, self.sched_attn_b2, i, T * 64)
        else:
            ops = AttnOperands(a["qkv"].data_ptr(), N * 3 * D, 3 * D, a["qkv"], D, 2 * D, 3 * D, a["o"], a["lse"], N, self.qmask_attn,
                               self.qblk_attn, self.sched_attn_f, self.sched_attn_b2, i)
        return ops, AttnGrads(ws["do"], ws["delta"], a["dqkv"].data_ptr(), N * 3 * D, 3 * D, False, a["dqkv"], D, 2 * D, 3 * D,
                              T * 64 if ws["do_hm"] else 0)

    def pool_attention(self, ws):
        """-> (AttnOperands, AttnGrads) of the attentive pooling: one (R, D) q for every sample, k | v packed as (T, 2D), dq fp32"""
        D, R = self.D, self.R
        return (AttnOperands(ws["qp"].data_ptr(), 0, D, ws["kvp"], 0, D, 2 * D, ws["op"], ws["lse_p"], R, self.qmask_pool,
                             self.qblk_pool, self.sched_pool_f, self.sched_pool_b2, None),
                AttnGrads(ws["dop"], ws["delta_p"], ws["dqp32"].data_ptr(), R * D, D, True, ws["dkvp"], 0, D, 2 * D))

    def attn_keys(self, ws) -> AttnKeys:
        """the key-side state of this workspace's forward (read at every call: a test may take ws["khot"] away between two)"""
        return AttnKeys(ws["keyinfo"], ws["kflags"], ws.get("khot"), self.N, self.nk_pad, ws["b"], self.H, self.scale, self.attn_flags)

    def attn_forward(self, ops, ws):
        N, b = self.N, ws["b"]
        a = attention.fwd_args(ops, self.attn_keys(ws), ws["vmean"])
        # mean(V) is the output of fully masked rows only: samples with every modality present have none and are skipped
        if ops.hstride:
            assert ws.get("present_cur") is not None and self.attn_dtype == "bf16", "head-major q | k | v: the engine's own bf16 forward only"
            call("mca_attn_vmean_if_needed_hm", a.v, a.kv_bstride, a.kv_ld, ops.hstride, ws["vmean"].data_ptr(), b, N, self.H,
                 ptr(ws["present_cur"]), (1 << self.M) - 1, stream_ptr(), profile_as="mca_attn_vmean_if_needed")
        elif ws.get("present_cur") is not None:
            call("mca_attn_vmean_if_needed", a.v, a.kv_bstride, a.kv_ld, ws["vmean"].data_ptr(), b, N, self.H, ptr(ws["present_cur"]),
                 (1 << self.M) - 1, stream_ptr())
        else:
            call("mca_attn_vmean", a.v, a.kv_bstride, a.kv_ld, ws["vmean"].data_ptr(), b, N, self.H, stream_ptr())
        f = None
        if self.attn_dtype == "fp8" and ops.nq == N:
            f = self._fp8_operands(ws, b, ops.layer)[1]
            ws[("fp8gen", ops.layer)] = ws["gen"]
        attention.launch_forward(a, ops, f)

    def attn_backward(self, ops, grads, ws):
        """The attention backward in the form backward_plan names.  The layer attention at a batch that gives every CU a
        (sample, head) takes the one-pass form."""
        b, keys = ws["b"], self.attn_keys(ws)
        plan = self.backward_plan(ws, b, ops.nq, grads.dq_f32)
        if ops.hstride or grads.do_hstride:
            # head-major operands are the one-pass kernel's alone, q | k | v and dO together.  Anything else - the plan changed since
            # the forward, or these records are older than such a change - goes back to the row-major matrices first
            a = ws["layers"][ops.layer]
            if plan.form != "onepass" or not (a["qkv_hm"] and ws["do_hm"]):
                self._to_row_major(ws, ops.layer)
                ops, grads = self.layer_attention(ws, ops.layer)
        if plan.form == "onepass":
            sc = self.sched_onepass
            assert ws["dq_acc"].numel() >= b * self.H * plan.split * (sc.n_qt + 1) * 4096, "dq_acc of this workspace is too small for the split"
            if ops.hstride:
                assert ops.hstride == grads.do_hstride == ws["T"] * 64 and ws["layers"][ops.layer]["qkv_hm"] and ws["do_hm"], \
                    f"layer {ops.layer}: q | k | v and dO are not both head-major as the forward recorded"
                attention.backward_onepass_hm(ops, grads, keys, sc, ws["rowc"], ws["dq_acc"], ws["dvmean"], plan.split)
            else:
                attention.backward_onepass(ops, grads, keys, sc, ws["rowc"], ws["dq_acc"], ws["dvmean"], *self._packed_copies(ws), plan.split)
        elif plan.form == "fp8-twopass":
            attention.backward_twopass(ops, grads, keys, ws["dvmean"], *self._fp8_bwd_operands(ws, b, ops.layer))
        else:
            attention.backward_twopass(ops, grads, keys, ws["dvmean"])

    # ------------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------------
    def _encode(self, batch, ws, need_grad: bool, drop: bool = False, sample0: Optional[int] = None, advance: bool = True):
        """encoders + packing (model.py:455-466): writes ws['x'][0] (b, N, D), ws['padding'] (b, N) and ws['present'] (b,)
        int32 (bit i = modality i has a valid token in that sample); returns modality_sample_mask {name: (b,) bool}.
        drop: draw this step's modality dropout while packing (set_modality_dropout) and advance its step counter; the (b, M)
        drop matrix is left in ws['dropped_cur'] (None when nothing was drawn).  sample0: the global index of the batch's first
        sample in the draw (default: this rank's rows of the data-parallel batch); advance False leaves the step counter alone (the
        chunks of a gradient-cached step, cached.py, draw at one counter value)."""
        m, D, N, b = self.model, self.D, self.N, ws["b"]
        x0 = ws["x"][0]
        ws["foreign"] = {}
        # ---- masks of every native modality in ONE launch: padding, the encoders' row masks, presence bits
        pk = hip.PackMasksArgs()
        keep = []                         # keeps converted mask tensors alive until the launch is enqueued
        native_idx = []
        for step in self.enc_steps:
            if not step.native:
                continue
            name, mi, n, off = step.name, step.mi, step.n, step.off
            am = step.attention_mask(batch[name], ws)
            if am.dtype == torch.bool or am.dtype == torch.uint8:
                eb = 1
            elif am.dtype == torch.int64:
                eb = 8
            else:
                am, eb = am.to(torch.bool), 1
            if not am.is_contiguous():
                am = am.contiguous()
            if am.shape != (b, n):
                raise AssertionError(f"{name}: attention_mask {tuple(am.shape)} != {(b, n)}")
            keep.append(am)
            d = pk.m[len(native_idx)]
            d.mask, d.elem_bytes, d.n, d.offset = am.data_ptr(), eb, n, off
            d.rowmask = step.row_mask(ws)
            native_idx.append(mi)
        foreign = len(native_idx) != len(m.modality_types)
        if native_idx:
            pk.n_mod, pk.batch, pk.n_tokens, pk.n_fusion = len(native_idx), b, N, (0 if foreign else self.F)
        ws["dropped_cur"] = None
        if drop:          # (every encoder is native: set_modality_dropout refuses anything else)
            s, da = self._mdrop, hip.ModalityDropArgs()
            for k, mi in enumerate(native_idx):
                da.p[k] = s["rates"][m.modality_types[mi]]
            da.seed, da.sample0, da.keep_one = s["seed"], (self.dropout_rank * b if sample0 is None else int(sample0)), int(s["keep_one"])
            call("mca_pack_masks_drop", C.byref(pk), C.byref(da), ptr(self._mdrop_counter), ptr(ws["padding"]), ptr(ws["present_native"]),
                 ptr(ws["dropped"]), stream_ptr())
            if advance:
                call("mca_counter_add", ptr(self._mdrop_counter), 1, stream_ptr())
            ws["dropped_cur"] = ((ws["dropped"][:, None] >> self._mod_shifts) & 1).to(torch.bool)
        elif native_idx:
            call("mca_pack_masks", C.byref(pk), ptr(ws["padding"]), ptr(ws["present_native"]), stream_ptr())
        present = ws["present"]
        if not foreign:
            present = ws["present_native"]          # bit k = k-th modality: the native list IS the modality list
        else:
            present.zero_()
            for k, mi in enumerate(native_idx):
                present |= ((ws["present_native"] >> k) & 1) << mi
        for step in self.enc_steps:
            step.forward(batch[step.name], ws, need_grad)
        if self.F:
            call("mca_bcast_rows", ptr(m.fusion_tokens.data), D, x0.data_ptr() + (N - self.F) * D * 4, D, N * D, self.F,
                 b * self.F, D, stream_ptr())
            if foreign:
                ws["padding"].view(b, N)[:, N - self.F:] = 0
        if self.eao:
            # the token block and the padding bytes of a modality, replicated into every combination segment that holds it
            pad2 = ws["padding"].view(b, N)
            for src, dst, n in self.st.copies:
                call("mca_rows_copy_add", x0.data_ptr() + src * D * 4, N * D, x0.data_ptr() + dst * D * 4, N * D, n, D, b, 0, stream_ptr())
                pad2[:, dst:dst + n].copy_(pad2[:, src:src + n])
        ws["present_cur"] = present
        bits = ((present[:, None] >> self._mod_shifts) & 1).to(torch.bool)          # (b, M): one small op for every modality
        return {name: bits[:, mi] for mi, name in enumerate(m.modality_types)}

    def ln_in_gemm(self, T: int) -> bool:
        """the residual LayerNorm recomputed in the out-proj / FF2 GEMM epilogues: what mca_gemm_nt_lnres accepts"""
        return self.fuse_ln_residual and T >= 2048 and self.D % 128 == 0 and self.D >= 512 and self.Ip >= 512

    def ln_rows_backward(self, T: int) -> bool:
        """The rule for the fused data-gradient GEMM + LayerNorm backward (mca_gemm_nt_res_lnbwd) in place of the pair mca_gemm_nt +
        mca_layernorm_bwd: the large-batch path (ln_in_gemm) of the MCA model at the one width the full-row kernel is built for, and
        never in deterministic mode, whose LayerNorm backward adds dgamma in a fixed order (mca_layernorm_bwd_det).  All three
        data-gradient shapes of the step (K = 2 Ip, 3 D, 2 D) take it: profiles/ln_rows_fusion.md has each against its pair."""
        return self.fuse_ln_rows and self.ln_in_gemm(T) and self.D == 512 and not self._deterministic and not self.eao

    def ln_rows_tall_form(self, ws, K: int) -> bool:
        """Whether the fused launch of this workspace's (T, D, K) shape goes to mca_gemm_nt_res_lnbwd_tall: where that entry point's
        plan for this device's CU count is the 160-row kernel (csrc/gemm_plan.h, mca_nt_rows_height: T = 81,216 and 40,608 on 256
        CUs; never b = 2 or b = 8), and unless MCA_DEBUG=ln_rows_tall=0.  The plan is asked once per workspace and shape, with the
        CU count given, so no device is touched."""
        if not self.ln_rows_tall:
            return False
        tall = ws["ln_rows_tall"]
        if K not in tall:
            pl = hip.GemmPlan()
            cus = torch.cuda.get_device_properties(self.device).multi_processor_count
            rc = hip.lib().mca_dbg_plan_gemm_nt(hip.PLAN_RES_LNBWD_TALL, C.byref(hip.NtProblem(M=ws["T"], N=self.D, K=K)), cus, C.byref(pl))
            tall[K] = rc == 0 and pl.kernel == hip.GK_NT_ROWS160_LNBWD
        return tall[K]

    def _gemm_ln_bwd(self, A, B, K, residual, x, gamma, mean, rstd, dgamma, dx, dx_bf16, ws):
        """dx (fp32, may be the residual), dx_bf16, dgamma += : the LayerNorm backward of dy = A B^T (+ residual) in one launch; timed
        under the row of the GEMM it replaces, whichever tile height runs (ln_rows_tall_form)"""
        D, T = self.D, ws["T"]
        if hip.PROFILE is not None:
            hip.set_tag(f"{T}x{D}x{K} f32{' +res' if residual is not None else ''}")
        call("mca_gemm_nt_res_lnbwd_tall" if self.ln_rows_tall_form(ws, K) else "mca_gemm_nt_res_lnbwd",
             ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(residual), residual.stride(0) if residual is not None else 0,
             ptr(x), x.stride(0), ptr(mean), ptr(rstd), ptr(gamma), ptr(dx), dx.stride(0), ptr(dx_bf16), dx_bf16.stride(0), ptr(dgamma),
             T, D, K, stream_ptr(), flops=2.0 * T * D * K, profile_as="mca_gemm_nt")
        if hip.PROFILE is not None:
            hip.set_tag("")

    def forward_trunk(self, ws):
        """fusion layers + final norm + attentive pooling -> ws['pooled'] (b*R, D)."""
        m, D, N, H, Ip, R, b, T = self.model, self.D, self.N, self.H, self.Ip, self.R, ws["b"], ws["T"]
        call("mca_build_keyinfo", ptr(ws["padding"]), ptr(self.kgroup), ptr(ws["keyinfo"]), ptr(ws["kflags"]), b, N,
             self.nk_pad, stream_ptr())
        if ws["khot"] is not None:
            call("mca_build_keyhot", ptr(ws["keyinfo"]), ptr(ws["khot"]), b, self.nk_pad, stream_ptr())
        # T >= 2048: the residual LayerNorm(x) is recomputed inside the out-proj / FF2 GEMM epilogues from x and the saved row
        # statistics (mca_gemm_nt_lnres): the LayerNorm kernels then write the bf16 GEMM operand only
        ln_in_gemm = self.ln_in_gemm(T)
        saved = self.geglu_saved_factors and self.fuse_geglu_bwd
        ff1 = "mca_gemm_nt_geglu_fwd_saved" if saved else "mca_gemm_nt_geglu_fwd"
        qkv_hm = self.qkv_head_major(ws)
        for i, ly in enumerate(m.layers):
            w, a = self.wl[i], ws["layers"][i]
            xin, xout = ws["x"][i], ws["x"][i + 1]
            g = ly.norm.gamma
            self.ln_fwd(xin, g, T, D, a["m1"], a["r1"], y=None if ln_in_gemm else ws["xn"], ldy=D, y_bf16=a["xn_b"], cols_pad=D)
            a["qkv_hm"] = qkv_hm
            (self.gemm_nt_cb if qkv_hm else self.gemm_nt)(a["xn_b"], w["qkv"], a["qkv"], T, 3 * D, D)
            self.attn_forward(self.layer_attention(ws, i)[0], ws)
            if ln_in_gemm:
                call("mca_gemm_nt_lnres", ptr(a["o"]), D, ptr(w["o"]), D, ptr(a["x1"]), D, ptr(xin), D, ptr(a["m1"]), ptr(a["r1"]),
                     ptr(g.data), T, D, D, stream_ptr(), flops=2.0 * T * D * D)
            else:
                self.gemm_nt(a["o"], w["o"], a["x1"], T, D, D, residual=ws["xn"])
            self.ln_fwd(a["x1"], g, T, D, a["m2"], a["r2"], y=None if ln_in_gemm else ws["x1n"], ldy=D, y_bf16=a["x1n_b"], cols_pad=D)
            # h = x1n @ W1^T and g = GEGLU(h) in one pass (h, or the backward's factors s in its place, is kept for the
            # backward, not read back here)
            a["h_holds"] = "s" if saved else "h"
            call(ff1, ptr(a["x1n_b"]), D, ptr(w["w1"]), D, ptr(a["h"]), 2 * Ip, ptr(a["g"]), Ip, Ip, T, D,
                 stream_ptr(), flops=2.0 * T * 2 * Ip * D, profile_as="mca_gemm_nt_geglu_fwd")
            if ln_in_gemm:
                call("mca_gemm_nt_lnres", ptr(a["g"]), Ip, ptr(w["w2"]), Ip, ptr(xout), D, ptr(a["x1"]), D, ptr(a["m2"]), ptr(a["r2"]),
                     ptr(g.data), T, D, Ip, stream_ptr(), flops=2.0 * T * D * Ip)
            else:
                self.gemm_nt(a["g"], w["w2"], xout, T, D, Ip, residual=ws["x1n"])
        xl = ws["x"][self.L]
        if self.eao:
            # final norm (fp32 out), then the mean of every segment's un-padded rows (model.py:563-570, 255-276)
            self.ln_fwd(xl, m.norm.gamma, T, D, ws["mf"], ws["rf"], y=ws["xn"], ldy=D)
            call("mca_segment_mean_fwd", ptr(ws["xn"]), ptr(ws["padding"]), ptr(self.seg_start), R, ptr(ws["pooled"]),
                 ptr(ws["seg_counts"]), b, N, D, stream_ptr())
            return ws["pooled"]
        self.ln_fwd(xl, m.norm.gamma, T, D, ws["mf"], ws["rf"], y_bf16=ws["t_b"], cols_pad=D)
        self.gemm_nt(ws["t_b"], self.wp["kv"], ws["kvp"], T, 2 * D, D)
        call("mca_f32_to_bf16", ptr(m.return_tokens.data), D, ptr(ws["rt_b"]), D, R, D, 1.0, stream_ptr())
        self.gemm_nt(ws["rt_b"], self.wp["q"], ws["qp"], R, D, D)
        self.attn_forward(self.pool_attention(ws)[0], ws)
        self.gemm_nt(ws["op"], self.wp["o"], ws["pooled"], b * R, D, D, residual=m.return_tokens.data, res_period=R)
        return ws["pooled"]

    # ------------------------------------------------------------------------------------------------
    # loss (+ its gradient w.r.t. the local pooled block and the temperature)
    # ------------------------------------------------------------------------------------------------
    def loss_fwd_bwd(self, pooled_all, present_all, b_local, row0):
        B, R, D, T = pooled_all.shape[0], self.R, self.D, self.n_terms
        dev = self.device
        nbytes = hip.lib().mca_contrastive_workspace_bytes(B, T)
        key = ("lossws", B)
        if key not in self._ws:
            self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = dict(term_loss=torch.empty(T, dtype=torch.float32, device=dev), loss=torch.empty(1, dtype=torch.float32, device=dev),
                   d_pooled=torch.empty(b_local, R, D, dtype=torch.float32, device=dev),
                   d_logit=torch.empty(1, dtype=torch.float32, device=dev))
        ls = self.model.loss.loss_fn.logit_scale
        call("mca_contrastive_fwd_bwd", ptr(pooled_all), ptr(present_all), ptr(self.loss_terms_dev), T, ptr(ls.data), B, b_local,
             row0, R, D, ptr(out["term_loss"]), ptr(out["loss"]), ptr(out["d_pooled"]), ptr(out["d_logit"]),
             ptr(self._ws[key]), stream_ptr())
        return out

    # ------------------------------------------------------------------------------------------------
    # the pieces of a gradient-cached step (cached.py): nothing above calls them
    # ------------------------------------------------------------------------------------------------
    def loss_kernel_for(self, B: int, choice: str = "auto") -> str:
        """"dense" or "stream" for a bank of B rows.  auto: the streaming kernel wherever the dense workspace would be more than eight
        times the streaming one, about T B^2 against 9 T B floats: from B = 68 (14 terms) to 74 (one term) on.  That lies below the size from which
        the streaming kernel measured faster (it ties the dense one at B = 256, profiles/cached_step.md), so the workspace rule alone
        decides and no timing threshold is kept.  Dense where the streaming kernel refuses the width."""
        if choice not in ("auto", "dense", "stream"):
            raise ValueError(f"loss_kernel is '{choice}', not one of auto, dense, stream")
        lay = hip.contrastive_stream_layout(B, self.n_terms)
        if self.D > lay["DMAX"]:
            if choice == "stream":
                raise hip.MCAHipError(f"the streaming loss kernel takes D <= {lay['DMAX']}, the model has D = {self.D}")
            return "dense"
        if choice != "auto":
            return choice
        L = hip.lib()
        big = L.mca_contrastive_workspace_bytes(B, self.n_terms) > 8 * L.mca_contrastive_stream_workspace_bytes(B, self.n_terms, self.R, self.D)
        return "stream" if big else "dense"

    def loss_fwd_bwd_bank(self, bank, present_all, kernel: str):
        """The loss over a caller-owned (B, R, D) bank as ONE rank of B rows (b_local = B, row0 = 0) with the kernel named: "dense"
        (mca_contrastive_fwd_bwd) or "stream" (mca_contrastive_stream_fwd_bwd).  -> loss_fwd_bwd's dict, d_pooled (B, R, D)."""
        B, R, D, T = bank.shape[0], self.R, self.D, self.n_terms
        if kernel == "dense":
            return self.loss_fwd_bwd(bank, present_all, B, 0)
        dev, L = self.device, hip.lib()
        nbytes = L.mca_contrastive_stream_workspace_bytes(B, T, R, D)
        key = ("lossws_stream", B)
        if key not in self._ws:
            self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = dict(term_loss=torch.empty(T, dtype=torch.float32, device=dev), loss=torch.empty(1, dtype=torch.float32, device=dev),
                   d_pooled=torch.empty(B, R, D, dtype=torch.float32, device=dev),
                   d_logit=torch.empty(1, dtype=torch.float32, device=dev))
        ls = self.model.loss.loss_fn.logit_scale
        call("mca_contrastive_stream_fwd_bwd", ptr(bank), ptr(present_all), ptr(self.loss_terms_dev), T, ptr(ls.data), B, B, 0, R, D,
             ptr(out["term_loss"]), ptr(out["loss"]), ptr(out["d_pooled"]), ptr(out["d_logit"]), ptr(self._ws[key]), nbytes, stream_ptr())
        return out

    def forward_chunk(self, batch, sample0: int):
        """Forward of one chunk to its pooled tokens, without the loss and repeatable: in training mode the modality dropout (if set)
        is drawn for global samples sample0 .. sample0 + b - 1 at the current step counter, which is NOT advanced, so a second call
        draws the same masks; the finite flags are OR-ed into the device word and nothing here clears it.  Native encoders only
        (can_forward_backward()): their forward always leaves in the workspace what backward(ws, ...) needs, as forward_backward
        relies on.  -> (ws, pooled (b, R, D) view of the workspace, modality_sample_mask)."""
        m = self.model
        b = next(iter(batch[m.modality_types[0]].values())).shape[0]
        if self.check_finite:
            self._flag_inputs(batch)
        self.refresh_weights()
        ws = self.workspace(b)
        ws["gen"] += 1
        sample_mask = self._encode(batch, ws, False, drop=self._mdrop is not None and m.training, sample0=sample0, advance=False)
        pooled = self.forward_trunk(ws).view(b, self.R, self.D)
        if self.check_finite:
            self._flag_tensors([pooled], 2)
        return ws, pooled, sample_mask

    def advance_modality_dropout(self):
        """the step counter of the modality dropout + 1, by a kernel: once per gradient-cached step, as a plain step does"""
        if self._mdrop is not None and self.model.training:
            call("mca_counter_add", ptr(self._mdrop_counter), 1, stream_ptr())

    def publish_flags(self):
        """the finite / index flag word to its pinned mirror, with the event poll_finite() and assert_finite() wait for"""
        if self.check_finite:
            call("mca_flag_to_host", ptr(self.finite_flag), self._flag_host.data_ptr(), stream_ptr())
            self._flag_event = torch.cuda.Event()
            self._flag_event.record()

    # ------------------------------------------------------------------------------------------------
    # backward
    # ------------------------------------------------------------------------------------------------
    def _on_side(self, fn, slot: int, ws: dict):
        """Run fn() on the workspace's side stream, ordered after everything enqueued so far on the current stream."""
        if not self.overlap_on(ws):
            fn()
            return
        side, events = ws["side"], ws["side_events"]
        while len(events) <= slot:
            events.append(torch.cuda.Event())
        ev = events[slot]
        ev.record()
        with torch.cuda.stream(side), hip.use_stream(side.cuda_stream):
            side.wait_event(ev)
            fn()

    OVERLAP_ROWS_MAX = 40960

    def overlap_on(self, ws) -> bool:
        """weight-gradient GEMMs of this workspace on its side stream?"""
        if self.overlap_wgrad is None:
            return ws["T"] < self.OVERLAP_ROWS_MAX
        return bool(self.overlap_wgrad)

    def _bucket_ready(self, idx):
        if self.grad_bucket_hook is not None:
            lo = 0 if idx == 0 else self.bucket_bounds[idx - 1]
            self.grad_bucket_hook(lo, self.bucket_bounds[idx])

    def backward(self, ws, d_pooled, d_logit_scale=None, accumulate=False):
        """d_pooled: (b, R, D) fp32 gradient of the objective w.r.t. the pooled tokens.  Writes every parameter
        gradient into the flat gradient buffer."""
        if not accumulate:
            self.gflat.zero_()
        if d_logit_scale is not None:
            self.grad_of(self.model.loss.loss_fn.logit_scale).add_(d_logit_scale.reshape(()))
        self._backward_part(ws, d_pooled, self._bucket_ready)
        if self.overlap_on(ws):
            torch.cuda.current_stream().wait_stream(ws["side"])          # every weight gradient is in before clip / AdamW

    def _backward_part(self, ws, d_pooled, bucket_ready):
        m, D, N, H, Ip, I, R, b, T = self.model, self.D, self.N, self.H, self.Ip, self.I, self.R, ws["b"], ws["T"]
        G = self.grad_of
        dpool = d_pooled.reshape(b * R, D).contiguous()
        ap = m.attn_pool
        # Weight-gradient GEMMs (mca_gemm_tn_acc) only feed the optimizer: they are issued on a side stream, ordered after
        # the kernel that produced their operand, and run concurrently with the rest of the backward chain (their
        # operands live in per-layer buffers, so nothing overwrites them).  slot = unique id of the call site.
        # Deterministic mode, ordering audit.  A *_det launch adds into its gradient tensor with a plain read-modify-write, so two
        # launches into one tensor must be ordered.  The tensors that receive more than one launch's contribution per backward:
        #   m.norm.gamma / ly.norm.gamma (both LayerNorms of a layer), return_tokens (two mca_reduce_rows), fusion_tokens, the
        #   encoder norms' gamma / beta and the Linear biases fed by dxsum, the embedding table, linear1.weight / bias
        #     - all launched from this thread on the CURRENT stream: stream order;
        #   every weight matrix (one launch each; feedforward[0].weight two launches into disjoint row blocks, or two members
        #   of one grouped launch) - all on the side stream when overlap_on(ws), else on the current stream: stream order.
        # No tensor gets contributions from both streams, and neighbours in the flat buffer never share an element.
        # backward(accumulate=True): backward() ends with current.wait_stream(side) and every side launch waits for an event
        # recorded on the current stream, so the second backward's launches follow the first's on either stream.  Nothing has
        # to be added for deterministic mode; the scratch regions are per stream for the same reason (_alloc_det_scratch).
        side = self._on_side
        tn = lambda *a: self._tn(ws, *a)
        slot = [0]

        def on_side(fn):
            side(fn, slot[0], ws); slot[0] += 1

        if self.eao:
            return self._backward_part_eao(ws, dpool, bucket_ready, on_side)
        # pooled = op @ Wo^T + return_tokens
        self._reduce_rows(ws, ptr(dpool), D, R * D, R, ptr(G(m.return_tokens)), D, b * R, D)
        call("mca_f32_to_bf16", ptr(dpool), D, ptr(ws["dpool_b"]), D, b * R, D, 1.0, stream_ptr())
        self.gemm_nt(ws["dpool_b"], self.wp["oT"], ws["dop"], b * R, D, D)
        on_side(lambda: tn(ws["dpool_b"], ws["op"], G(ap.to_out.weight), b * R, D, D))
        # pooling attention
        self.attn_backward(*self.pool_attention(ws), ws)
        ws["dqp_sum"].zero_()
        self._reduce_rows(ws, ptr(ws["dqp32"]), D, R * D, R, ptr(ws["dqp_sum"]), D, b * R, D)
        call("mca_f32_to_bf16", ptr(ws["dqp_sum"]), D, ptr(ws["dqp_b"]), D, R, D, 1.0, stream_ptr())
        self.gemm_nt(ws["dqp_b"], self.wp["qT"], ws["drt"], R, D, D)                 # d return_tokens via to_q
        self._reduce_rows(ws, ptr(ws["drt"]), D, R * D, R, ptr(G(m.return_tokens)), D, R, D)
        on_side(lambda: tn(ws["dqp_b"], ws["rt_b"], G(ap.to_q.weight), R, D, D))
        pool_kv = (ws["dkvp"], ws["t_b"], G(ap.to_kv.weight), 2 * D, D)
        if not (self.L > 0 and self.group_wgrad and T >= 4096):          # else: a member of the top layer's grouped launch
            on_side(lambda pk=pool_kv: tn(pk[0], pk[1], pk[2], T, 2 * D, D))
            pool_kv = None
        dx, dx_other = ws["dxa"], ws["dxb"]
        top = ws["layers"][self.L - 1]["dxo_b"] if self.L else ws["dx_b"]
        if self.ln_rows_backward(T):
            self._gemm_ln_bwd(ws["dkvp"], self.wp["kvT"], 2 * D, None, ws["x"][self.L], m.norm.gamma, ws["mf"], ws["rf"], G(m.norm.gamma),
                              dx_other, top, ws)
        else:
            self.gemm_nt(ws["dkvp"], self.wp["kvT"], dx, T, D, 2 * D)                    # d (final-normed tokens), fp32
            self._ln_bwd(ws, dx, D, ws["x"][self.L], m.norm.gamma, ws["mf"], ws["rf"], T, D, G(m.norm.gamma), dx=dx_other, dx_bf16=top)
        dx, dx_other = dx_other, dx
        on_side(lambda: bucket_ready(0))
        self._backward_layers_and_encoders(ws, dx, dx_other, bucket_ready, on_side, extra_top=pool_kv)

    def _backward_part_eao(self, ws, dpool, bucket_ready, on_side):
        """EAO: d pooled (b, segments, D) -> mean-pool backward -> final norm backward -> the shared layer / encoder chain."""
        m, D, N, R, b, T = self.model, self.D, self.N, self.R, ws["b"], ws["T"]
        dx, dx_other = ws["dxa"], ws["dxb"]
        call("mca_segment_mean_bwd", ptr(dpool), ptr(ws["padding"]), ptr(self.kgroup), ptr(ws["seg_counts"]), R, ptr(dx), b, N, D,
             stream_ptr())
        top = ws["layers"][self.L - 1]["dxo_b"] if self.L else ws["dx_b"]
        self._ln_bwd(ws, dx, D, ws["x"][self.L], m.norm.gamma, ws["mf"], ws["rf"], T, D, self.grad_of(m.norm.gamma), dx=dx_other, dx_bf16=top)
        dx, dx_other = dx_other, dx
        on_side(lambda: bucket_ready(0))
        self._backward_layers_and_encoders(ws, dx, dx_other, bucket_ready, on_side)

    def _backward_layers_and_encoders(self, ws, dx, dx_other, bucket_ready, on_side, extra_top=None):
        m, D, N, H, Ip, I, R, b, T = self.model, self.D, self.N, self.H, self.Ip, self.I, self.R, ws["b"], ws["T"]
        G = self.grad_of
        tn = lambda *a: self._tn(ws, *a)
        for bi, i in enumerate(reversed(range(self.L))):
            ly, w, a = m.layers[i], self.wl[i], ws["layers"][i]
            g = ly.norm.gamma
            dxo, dx1, dh, dqkv = a["dxo_b"], a["dx1_b"], a["dh"], a["dqkv"]
            below = ws["layers"][i - 1]["dxo_b"] if i > 0 else ws["dx_b"]
            # x_out = g @ W2^T + x1n            (dx = d x_out fp32, dxo = its bf16 copy)
            # The five weight gradients of the layer reduce over the same T rows: grouped into one launch after the layer's
            # attention backward (52 tiles of 256 x 256 -> 5 row splits instead of 21-32 per gradient: a quarter of the fp32 atomic
            # traffic; the launch's balanced row partition fills all CUs for any tile count, gemm.hip struct tn_group).
            grouped = self.group_wgrad and T >= 4096
            if not grouped:
                on_side(lambda dxo=dxo, a=a, ly=ly: tn(dxo, a["g"], G(ly.ff.feedforward[2].weight), T, D, I))
            # the layer's buffer holds what this backward is about to read it as: a flag switched between forward and backward
            # would otherwise hand the saved factors to a kernel that takes them for h, or the other way round
            saved = self.geglu_saved_factors and self.fuse_geglu_bwd
            assert a["h_holds"] == ("s" if saved else "h"), \
                f"layer {i}: the forward left {a['h_holds']!r} in the GEGLU buffer; geglu_saved_factors / fuse_geglu_bwd changed since"
            if self.fuse_geglu_bwd:
                # dh = GEGLU'(h) * (dx @ W2): the (T, Ip) intermediate dg is never written (fused GEMM epilogue)
                call("mca_gemm_nt_geglu_bwd_saved" if saved else "mca_gemm_nt_geglu_bwd", ptr(dxo), D, ptr(w["w2T"]), D,
                     ptr(a["h"]), ptr(dh), 2 * Ip, Ip, T, D, stream_ptr(), flops=2.0 * T * Ip * D, profile_as="mca_gemm_nt_geglu_bwd")
            else:
                self.gemm_nt(dxo, w["w2T"], ws["dg"], T, Ip, D)
                call("mca_geglu_bwd", ptr(ws["dg"]), ptr(a["h"]), ptr(dh), T, Ip, stream_ptr())
            gw1 = G(ly.ff.feedforward[0].weight)
            if not grouped:
                on_side(lambda dh=dh, a=a, gw1=gw1: (tn(dh, a["x1n_b"], gw1, T, I, D), tn(dh[:, Ip:], a["x1n_b"], gw1[I:], T, I, D)))
            rows = self.ln_rows_backward(T)          # d x1n / d xn stay in the GEMM's tile; dx is read (residual) and written in place
            if rows:
                self._gemm_ln_bwd(dh, w["w1T"], 2 * Ip, dx, a["x1"], g, a["m2"], a["r2"], G(g), dx, dx1, ws)
            else:
                self.gemm_nt(dh, w["w1T"], dx_other, T, D, 2 * Ip, residual=dx)            # d x1n = dh @ W1 + dx
                self._ln_bwd(ws, dx_other, D, a["x1"], g, a["m2"], a["r2"], T, D, G(g), dx=dx, dx_bf16=dx1)   # dx = d x1
            # x1 = o @ Wo^T + xn
            if not grouped:
                on_side(lambda dx1=dx1, a=a, ly=ly: tn(dx1, a["o"], G(ly.attn.to_out.weight), T, D, D))
            # dO head-major beside a head-major q | k | v (the one-pass backward reads both in place)
            ws["do_hm"] = a["qkv_hm"] and self.backward_plan(ws, b, self.N).form == "onepass"
            (self.gemm_nt_cb if ws["do_hm"] else self.gemm_nt)(dx1, w["oT"], ws["do"], T, D, D)
            # dq | dk | dv land in dqkv as bf16, each element written once
            self.attn_backward(*self.layer_attention(ws, i), ws)
            # to_q.weight and to_kv.weight are adjacent in the flat gradient buffer: one (3D, D) weight-gradient GEMM
            gq = G(ly.attn.to_q.weight)
            assert G(ly.attn.to_kv.weight).data_ptr() == gq.data_ptr() + D * D * 4
            if grouped:
                gw2, gwo = G(ly.ff.feedforward[2].weight), G(ly.attn.to_out.weight)
                extra = [extra_top] if (bi == 0 and extra_top is not None) else []
                on_side(lambda dqkv=dqkv, dh=dh, dxo=dxo, dx1=dx1, a=a, gq=gq, gw1=gw1, gw2=gw2, gwo=gwo, extra=extra: self._tn_group(
                    ws, [(dqkv, a["xn_b"], gq, 3 * D, D), (dh, a["x1n_b"], gw1, I, D), (dh[:, Ip:], a["x1n_b"], gw1[I:], I, D),
                     (dxo, a["g"], gw2, D, I), (dx1, a["o"], gwo, D, D)] + extra, T))
            else:
                on_side(lambda dqkv=dqkv, a=a, gq=gq: tn(dqkv, a["xn_b"], gq, T, 3 * D, D))
            if rows:
                self._gemm_ln_bwd(dqkv, w["qkvT"], 3 * D, dx, ws["x"][i], g, a["m1"], a["r1"], G(g), dx, below, ws)
            else:
                self.gemm_nt(dqkv, w["qkvT"], dx_other, T, D, 3 * D, residual=dx)          # d xn = dqkv @ Wqkv + d x1
                self._ln_bwd(ws, dx_other, D, ws["x"][i], g, a["m1"], a["r1"], T, D, G(g), dx=dx, dx_bf16=below)  # dx = d x_in
            on_side(lambda bi=bi: bucket_ready(bi + 1))
        # dx = gradient w.r.t. the packed encoder output (b, N, D)
        if self.eao:          # the gradients of a modality's replicas, summed into the segment its encoder wrote
            for src, dst, n in self.st.copies:
                call("mca_rows_copy_add", dx.data_ptr() + dst * D * 4, N * D, dx.data_ptr() + src * D * 4, N * D, n, D, b, 1, stream_ptr())
        if self.F:
            self._reduce_rows(ws, dx.data_ptr() + (N - self.F) * D * 4, D, N * D, self.F, ptr(G(m.fusion_tokens)), D, b * self.F, D)
        for step in self.enc_steps:
            step.backward(ws, dx, on_side)
        on_side(lambda: bucket_ready(len(self.bucket_bounds) - 1))

    # ------------------------------------------------------------------------------------------------
    # model-level forward (autograd node)
    # ------------------------------------------------------------------------------------------------
    def model_forward(self, batch, no_loss=False):
        with hip.cached_stream():
            return self._model_forward(batch, no_loss)

    def can_forward_backward(self) -> bool:
        return all(s.native for s in self.enc_steps)

    def forward_backward(self, batch):
        """forward + loss + backward WITHOUT autograd: the same kernels as ``model(batch)`` followed by ``loss.backward()``, issued
        from the calling thread (autograd runs a CUDA backward on its device thread; a stream capture that is cut into segments
        at the data-parallel collectives must begin and end its captures on one thread: graph.GraphedStep).  Every ``p.grad`` is
        the view of the flat gradient buffer.  Returns the output dict of the forward."""
        m = self.model
        if not self.can_forward_backward():
            raise NotImplementedError("forward_backward needs native encoders (a torch encoder's backward runs under autograd)")
        with hip.cached_stream(), torch.no_grad():
            self._last_direct = None
            out = self._model_forward(batch, no_loss=False)
            ws, res = self._last_direct
            self.backward(ws, res["d_pooled"], res["d_logit"], accumulate=False)
        for p in self.param_order:
            p.grad = self.grad_of(p)
        return out

    def _model_forward(self, batch, no_loss=False):
        m = self.model
        first = batch[m.modality_types[0]]
        b = next(iter(first.values())).shape[0]
        need_grad = torch.is_grad_enabled() and not no_loss
        if self.check_finite:
            if not torch.cuda.is_current_stream_capturing():           # (hipEventQuery would invalidate a stream capture)
                self.poll_finite()                                     # a flagged EARLIER step raises here (no sync)
            self._flag_inputs(batch)
        self.refresh_weights()
        ws = self.workspace(b)
        ws["gen"] += 1          # the saved activations of any earlier forward of this batch size are gone from here on
        # the modality dropout is a training augmentation: eval, no_loss and model.eval() forwards keep today's launches
        sample_mask = self._encode(batch, ws, need_grad, drop=self._mdrop is not None and m.training and not no_loss)
        pooled = self.forward_trunk(ws).view(b, self.R, self.D)
        slots = m.output_slots()
        if self.check_finite:
            self._flag_tensors([pooled], 2)
            call("mca_flag_to_host", ptr(self.finite_flag), self._flag_host.data_ptr(), stream_ptr())          # (a kernel, not a copy node)
            if not torch.cuda.is_current_stream_capturing():          # (a captured step: graph.GraphedStep records it after the replay)
                self._flag_event = torch.cuda.Event()
                self._flag_event.record()
        if no_loss:
            out = {k: pooled[:, s] for k, s in slots.items()}
            out["modality_sample_mask"] = sample_mask
            if self.check_finite and self.check_finite != "deferred":
                self.assert_finite()
            return out
        # in-place clamp of the temperature parameter (utils/contrastive_loss_with_temperature.py:187)
        ls = m.loss.loss_fn
        ls.logit_scale.data.clamp_(ls.logit_scale_min, ls.logit_scale_max)
        present = ws["present_cur"]
        if need_grad:
            pooled_out, terms, loss = _MCAStep.apply(self, ws, pooled, present, *self.param_order)
        else:
            pooled_out, terms, loss, res = _loss_forward(self, pooled, present)
            self._last_direct = (ws, res)          # forward_backward(): the backward chain without an autograd node
        out = {k: pooled_out[:, s] for k, s in slots.items()}
        names = [t.name for t in m.loss_terms]
        out["losses"] = {n: terms[i] for i, n in enumerate(names)}
        if m.fcl and not m.zorro:
            if getattr(self, "_fc_w", None) is None:          # (2, terms) averaging weights, built once: three small kernels per step
                fc = torch.tensor([1.0 if "fcl" in n else 0.0 for n in names], dtype=torch.float32, device=self.device)
                self._fc_w = torch.stack([fc / fc.sum().clamp(min=1), (1 - fc) / (1 - fc).sum().clamp(min=1)])
            both = (torch.nan_to_num(terms)[None, :] * self._fc_w).sum(1)
            out["fcl_loss"], out["no-fcl_loss"] = both[0], both[1]
        out["loss"] = loss.reshape(())
        out["modality_sample_mask"] = sample_mask
        if ws["dropped_cur"] is not None:
            out["modality_dropped"] = ws["dropped_cur"]          # (b, M) bool, this step's draw
        if self.check_finite and self.check_finite != "deferred":
            self.assert_finite()
        return out

    # ---- finite flag ---------------------------------------------------------------------------------
    def _flag_tensors(self, tensors, bit: int):
        fa = hip.FiniteArgs()
        keep = []
        for t in tensors:
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.float().contiguous()
            keep.append(t)
            fa.p[len(keep) - 1], fa.n[len(keep) - 1] = t.data_ptr(), t.numel()
        fa.count = len(keep)
        if keep:
            call("mca_nonfinite_flag", C.byref(fa), ptr(self.finite_flag), bit, stream_ptr())

    def _flag_inputs(self, batch):
        """bit 0: a non-finite value anywhere in an encoder input (encoders.py:197-198 checks the whole `tokens` tensor,
        padded positions included); one launch for every modality.  Integer tensors (the `tokens` of a SequenceEncoder) are
        finite and are not scanned."""
        ts = [v[k] for v in batch.values() if isinstance(v, dict) for k in ("tokens", "values")
              if k in v and torch.is_tensor(v[k]) and v[k].is_floating_point()]
        self._flag_tensors(ts[:hip.MAX_MODALITIES], 1)

    def _raise_flag(self, bits: int):
        self.finite_flag.zero_()
        self._flag_host.zero_()
        self._flag_event = None
        if bits & FLAG_CACHE_MISMATCH:
            raise RuntimeError("gradient-cached step: a chunk's second forward did not reproduce the pooled tokens of its first "
                               "(CachedStep(verify=True)); the step's update is skipped")
        if bits & FLAG_INDEX_RANGE:
            raise IndexError("a token index is outside its encoder's table (the lookup skipped it; the step's update is skipped)")
        if bits & 1:
            raise Exception("Tokens are not finite")                                      # encoders.py:197-198
        raise Exception("Encoder transform / fusion resulted in non-finite values")       # encoders.py:206-213

    def poll_finite(self):
        """Non-blocking: raises if a step whose flag copy has already landed on the host saw non-finite values."""
        ev = self._flag_event
        if ev is not None and ev.query():
            bits = int(self._flag_host[0])
            if bits:
                self._raise_flag(bits)

    def assert_finite(self):
        """Blocking form: waits for the last step's flag copy and raises if it is set."""
        ev = self._flag_event
        if ev is not None:
            ev.synchronize()
            bits = int(self._flag_host[0])
            if bits:
                self._raise_flag(bits)


def _loss_forward(engine, pooled, present):
    """(optional all-gather of pooled embeddings + presence bits) then the fused loss kernels."""
    b = pooled.shape[0]
    if engine.gather_hook is not None:
        pooled_all, present_all, row0 = engine.gather_hook(pooled, present)
    else:
        pooled_all, present_all, row0 = pooled, present, 0
    res = engine.loss_fwd_bwd(pooled_all.contiguous(), present_all.contiguous(), b, row0)
    pooled_out = torch.empty_like(pooled)          # the embeddings handed to the caller: copied by a kernel (no copy node in a captured step)
    flat_in, flat_out = pooled.reshape(-1, pooled.shape[-1]), pooled_out.view(-1, pooled.shape[-1])
    call("mca_rows_copy_add", ptr(flat_in), 0, ptr(flat_out), 0, flat_in.shape[0], flat_in.shape[1], 1, 0, stream_ptr())
    return pooled_out, res["term_loss"], res["loss"], res


class _MCAStep(torch.autograd.Function):
    """One autograd node for the whole step.  forward: (optional all-gather) + loss kernels, which also
    produce d loss/d pooled; backward: the engine's backward chain, gradients written straight into the flat
    gradient buffer (each parameter's ``.grad`` is a view of it)."""

    @staticmethod
    def forward(ctx, engine, ws, pooled, present, *params):
        pooled_out, terms, loss, res = _loss_forward(engine, pooled, present)
        ctx.engine, ctx.ws, ctx.res, ctx.gen = engine, ws, res, ws["gen"]
        ctx.mark_non_differentiable(terms)
        return pooled_out, terms, loss

    @staticmethod
    def backward(ctx, g_pooled, g_terms, g_loss):
        engine, ws, res = ctx.engine, ctx.ws, ctx.res
        if ws["gen"] != ctx.gen:
            raise RuntimeError(
                "MCA.backward: another forward of the same batch size ran after the forward this loss came from; the step keeps "
                "ONE set of saved activations per batch size, so run backward() before the next forward (train or eval)")
        d_pooled = res["d_pooled"] * g_loss.reshape(())
        if g_pooled is not None:
            d_pooled = d_pooled + g_pooled
        params = engine.param_order
        live = params[0].grad is not None and params[0].grad.data_ptr() == engine.grad_of(params[0]).data_ptr()
        with hip.cached_stream():
            engine.backward(ws, d_pooled, res["d_logit"] * g_loss.reshape(()), accumulate=live)
        for p in params:
            p.grad = engine.grad_of(p)
        return (None, None, None, None) + tuple(None for _ in params)
