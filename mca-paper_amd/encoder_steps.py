"""One step object per encoder kind: what FusionEngine needs from a modality's encoder - its bf16 weight copies and their cast records,
its workspace buffers, the shapes of its deterministic launches, its forward and its backward.  The engine builds one per modality
(step_for, the only place that looks at an encoder's type) and loops over them: a new encoder kind is a class here and a line in
step_for.  Reference lines: encoders.py:196-214 (EmbeddedSequenceEncoder), :90-96 (TabularEncoder), :161-166 (SequenceEncoder), :114-120
(SparseTabularEncoder), :260-273 (PatchEncoder; its modes "image" and "video": ImagePatchEncoder, VideoPatchEncoder).
This module binds its own `call` from .hip: a tool that records launches by rebinding `call` patches hip, engine AND this module."""
from __future__ import annotations

import torch

from .encoders import EmbeddedSequenceEncoder, ImagePatchEncoder, PatchEncoder, SequenceEncoder, SparseTabularEncoder, TabularEncoder, VideoPatchEncoder
from .hip import call, ptr, stream_ptr

FLAG_INDEX_RANGE = 4          # the engine's flag word: bit 1 non-finite encoder input, bit 2 non-finite output, this one a token index outside its table


class _Step:
    def __init__(self, engine, name, mi, enc):
        self.eng, self.name, self.mi, self.enc = engine, name, mi, enc
        self.n, self.off = engine.st.token_dims[mi], engine.offsets[mi]          # tokens per sample, first row in the packed (N, D) sample
        self.D, self.N, self.G = engine.D, engine.N, engine.grad_of

    def _bf16(self, *shape):
        return torch.zeros(*shape, dtype=torch.bfloat16, device=self.eng.device)

    def attention_mask(self, bm, ws):
        """the (b, n) key-padding mask of the modality, non-zero = padded, which mca_pack_masks packs: the batch's own"""
        return bm["attention_mask"]


class SequenceStep(_Step):
    """EmbeddedSequenceEncoder: `mca_layernorm_fwd` (pad-masked, bf16 out) -> `mca_gemm_nt` + bias -> `mca_layernorm_fwd` (mask, + positional
    encoding, written into the packed token matrix)"""
    native = True

    def __init__(self, engine, name, mi, enc):
        super().__init__(engine, name, mi, enc)
        self.cin, self.kp = enc.input_size, (enc.input_size + 63) // 64 * 64          # the Linear's input width, padded to 64
        self.w, self.wT = self._bf16(self.D, self.kp), self._bf16(self.kp, self.D)

    def casts(self):
        self.eng._cast(self.enc.token_encoder[1].weight.data, self.w)
        self.eng._cast(self.enc.token_encoder[1].weight.data, self.wT, transpose=True)

    def workspace(self, b, f32, bf, u8):
        rows, D, kp = b * self.n, self.D, self.kp
        return dict(xin_b=bf(rows, kp), m0=f32(rows), r0=f32(rows), y=f32(rows, D), m2=f32(rows), r2=f32(rows),
                    dy=f32(rows, D), dy_b=bf(rows, D), dxin=f32(rows, kp), mask=u8(rows))

    def row_mask(self, ws):
        """the encoder's own row mask, written by mca_pack_masks"""
        return ws["enc"][self.name]["mask"].data_ptr()

    def forward(self, bm, ws, need_grad):
        eng, n, D, cin, b = self.eng, self.n, self.D, self.cin, ws["b"]
        e, te, rows = ws["enc"][self.name], self.enc.token_encoder, b * n
        toks = bm["tokens"]
        if toks.dtype != torch.float32 or not toks.is_contiguous():
            toks = toks.float().contiguous()
        if toks.shape != (b, n, cin):
            raise AssertionError(f"{self.name}: tokens {tuple(toks.shape)} != {(b, n, cin)}")
        e["tokens"] = toks
        eng.ln_fwd(toks.view(rows, cin), te[0].weight, rows, cin, e["m0"], e["r0"], beta=te[0].bias, rowmask=e["mask"],
                   y_bf16=e["xin_b"], cols_pad=self.kp)
        eng.gemm_nt(e["xin_b"], self.w, e["y"], rows, D, self.kp, bias=te[1].bias)
        eng.ln_fwd(e["y"], te[2].weight, rows, D, e["m2"], e["r2"], beta=te[2].bias, rowmask=e["mask"],
                   add=self.enc.positional_encoder.pe, period=n, y=ws["x"][0][self.off:], ldy=D, y_bstride=self.N * D)

    def det_shapes(self, b):
        """the deterministic launches of backward(): one weight gradient, two LayerNorm backwards"""
        rows = b * self.n
        return dict(tn=[(rows, self.D, self.cin)], ln=[(rows, self.D), (rows, self.cin)])

    def backward(self, ws, dx, on_side):
        eng, n, D, G, cin, kp = self.eng, self.n, self.D, self.G, self.cin, self.kp
        e, te, rows = ws["enc"][self.name], self.enc.token_encoder, ws["b"] * n
        # (the Linear's bias gradient = column sums of this norm's dx: same launch)
        eng._ln_bwd(ws, dx[self.off:], D, e["y"], te[2].weight, e["m2"], e["r2"], rows, D, G(te[2].weight), dbeta=G(te[2].bias),
                    rowmask=e["mask"], dx=e["dy"], dx_bf16=e["dy_b"], y_bstride=self.N * D, period=n, dxsum=G(te[1].bias))
        on_side(lambda e=e, te=te, rows=rows: eng._tn(ws, e["dy_b"], e["xin_b"], G(te[1].weight), rows, D, cin))
        eng.gemm_nt(e["dy_b"], self.wT, e["dxin"], rows, kp, D)
        eng._ln_bwd(ws, e["dxin"], kp, e["tokens"].view(rows, cin), te[0].weight, e["m0"], e["r0"], rows, cin, G(te[0].weight),
                    dbeta=G(te[0].bias), rowmask=e["mask"])


class _ValueChain(_Step):
    """The ContinuousValueEncoder part that TabularStep and SparseTabularStep share: `mca_tab_value_fwd` (Linear(1, D) + ReLU on
    min(x, max_value)) -> `mca_gemm_nt` + bias -> `mca_layernorm_fwd`, zero where x == padding_value, written into the packed token
    matrix; and its backward.  The trunk's key-padding mask is the batch's attention_mask."""
    native = True

    def __init__(self, engine, name, mi, enc):
        super().__init__(engine, name, mi, enc)
        self.w2, self.w2T = self._bf16(self.D, self.D), self._bf16(self.D, self.D)

    def casts(self):
        self.eng._cast(self.enc.value_encoder.linear2.weight.data, self.w2)
        self.eng._cast(self.enc.value_encoder.linear2.weight.data, self.w2T, transpose=True)

    def workspace(self, b, f32, bf, u8):
        rows, D = b * self.n, self.D
        return dict(h1_b=bf(rows, D), y=f32(rows, D), m2=f32(rows), r2=f32(rows), dy=f32(rows, D),
                    dy_b=bf(rows, D), dh1=f32(rows, D), mask=u8(rows))

    def row_mask(self, ws):
        return None          # (its mask comes from the values: mca_tab_value_fwd)

    def _value_forward(self, vals, ws, add):
        """vals (b, n) fp32 contiguous; add: (n, D) rows added after the mask, or None"""
        eng, n, D = self.eng, self.n, self.D
        e, ve, rows = ws["enc"][self.name], self.enc.value_encoder, ws["b"] * n
        e["values"] = vals
        call("mca_tab_value_fwd", ptr(vals), ptr(ve.linear1.weight.data), ptr(ve.linear1.bias.data), ptr(e["h1_b"]), ptr(e["mask"]),
             rows, D, float(ve.max_value), float(ve.padding_value), stream_ptr())
        eng.gemm_nt(e["h1_b"], self.w2, e["y"], rows, D, D, bias=ve.linear2.bias)
        eng.ln_fwd(e["y"], ve.norm.weight, rows, D, e["m2"], e["r2"], beta=ve.norm.bias, rowmask=e["mask"], add=add,
                   period=n, y=ws["x"][0][self.off:], ldy=D, y_bstride=self.N * D)

    def _value_det_shapes(self, b):
        """the deterministic launches of _value_backward(): one LayerNorm backward, one weight gradient, Linear1"""
        rows, D = b * self.n, self.D
        return dict(ln=[(rows, D)], tn=[(rows, D, D)], tab=[rows])

    def _value_backward(self, ws, dx, on_side):
        eng, n, off, D, N, G = self.eng, self.n, self.off, self.D, self.N, self.G
        e, ve, rows = ws["enc"][self.name], self.enc.value_encoder, ws["b"] * n
        eng._ln_bwd(ws, dx[off:], D, e["y"], ve.norm.weight, e["m2"], e["r2"], rows, D, G(ve.norm.weight), dbeta=G(ve.norm.bias),
                    rowmask=e["mask"], dx=e["dy"], dx_bf16=e["dy_b"], y_bstride=N * D, period=n, dxsum=G(ve.linear2.bias))
        on_side(lambda e=e, ve=ve, rows=rows: eng._tn(ws, e["dy_b"], e["h1_b"], G(ve.linear2.weight), rows, D, D))
        eng.gemm_nt(e["dy_b"], self.w2T, e["dh1"], rows, D, D)
        eng._sum_launch(ws, "mca_tab_value_bwd", (ptr(e["dh1"]), D, ptr(e["h1_b"]), ptr(e["values"]), ptr(G(ve.linear1.weight)),
                                                  ptr(G(ve.linear1.bias)), rows, D, float(ve.max_value)), lambda: (rows, D))


class TabularStep(_ValueChain):
    """TabularEncoder: E[t] (max_norm-renormalised in place) + LN(Linear2(ReLU(Linear1(min(x, max))))), the value part zeroed where
    x == padding_idx (-1)."""

    def forward(self, bm, ws, need_grad):
        enc, n, D, b = self.enc, self.n, self.D, ws["b"]
        vals = bm["values"]
        if vals.dtype != torch.float32 or not vals.is_contiguous():
            vals = vals.float().contiguous()
        if vals.shape != (b, n):
            raise AssertionError(f"{vals.shape[1]} - {n}")                  # encoders.py:93
        emb = enc.token_encoder.embedding.weight
        call("mca_embedding_renorm", ptr(emb.data), n, D, float(enc.token_encoder.max_norm), stream_ptr())
        self._value_forward(vals, ws, emb.data)

    def det_shapes(self, b):
        """the deterministic launches of backward(): the table's row sum, then the value chain's"""
        return dict(rr=[(b * self.n, self.n)], **self._value_det_shapes(b))

    def backward(self, ws, dx, on_side):
        eng, n, off, D, N, G = self.eng, self.n, self.off, self.D, self.N, self.G
        gemb = G(self.enc.token_encoder.embedding.weight)
        # the table is added after the value path is masked: every row of dx reaches it; padding_idx row stays frozen
        eng._reduce_rows(ws, dx.data_ptr() + off * D * 4, D, N * D, n, ptr(gemb), D, ws["b"] * n, D)
        gemb[n - 1].zero_()
        self._value_backward(ws, dx, on_side)


class _TableLookup:
    """What the two indexed encoders share (mixed into a _Step): the table of `enc.token_encoder`, looked up by a (b, n) integer
    tensor of the batch.  `mca_embedding_lookup` renormalises the rows the batch names and gathers them into the packed token
    matrix; the table gradient is `mca_embedding_scatter_add` over the same indices.  An index outside the table sets
    FLAG_INDEX_RANGE in the engine's flag word and contributes nothing, forward or backward."""

    def _table_init(self):
        te = self.enc.token_encoder
        self.V, pad = te.num_embeddings, te.embedding.padding_idx
        self.pad = self.V if pad is None else int(pad)          # (nn.Embedding has made a negative padding_idx positive)
        self.marker = torch.zeros(self.V, dtype=torch.int32, device=self.eng.device)          # zero between launches (mca_hip.h)

    def _indices(self, t, what, b):
        # a floating-point index tensor is what SequenceCollator emits when a sample of the batch is missing
        if t.dtype not in (torch.int64, torch.int32):
            t = t.to(torch.int64)
        if not t.is_contiguous():
            t = t.contiguous()
        if t.shape != (b, self.n):
            raise AssertionError(f"{self.name}: {what} {tuple(t.shape)} != {(b, self.n)}")
        return t

    def _lookup(self, idx, ws, add, accumulate):
        eng, te, D = self.eng, self.enc.token_encoder, self.D
        ws["enc"][self.name]["idx"] = idx
        call("mca_embedding_lookup", ptr(te.embedding.weight.data), self.V, D, float(te.max_norm), ptr(idx), idx.element_size(),
             ws["b"] * self.n, self.n, ptr(add), ws["x"][0].data_ptr() + self.off * D * 4, D, self.N * D, int(accumulate),
             ptr(self.marker), ptr(eng.finite_flag) if eng.check_finite else None, FLAG_INDEX_RANGE, stream_ptr())

    def _table_backward(self, ws, dx):
        D, rows, idx = self.D, ws["b"] * self.n, ws["enc"][self.name]["idx"]
        self.eng._sum_launch(ws, "mca_embedding_scatter_add",
                             (dx.data_ptr() + self.off * D * 4, D, self.N * D, self.n, ptr(idx), idx.element_size(), rows,
                              ptr(self.G(self.enc.token_encoder.embedding.weight)), self.V, D, self.pad), lambda: (rows,))


class TokenSequenceStep(_Step, _TableLookup):
    """SequenceEncoder: E[tokens] + positional table in one `mca_embedding_lookup`, straight into the packed token matrix; padded
    positions are not zeroed (encoders.py:161-166).  The trunk's key-padding mask is the batch's attention_mask."""
    native = True

    def __init__(self, engine, name, mi, enc):
        super().__init__(engine, name, mi, enc)
        self._table_init()

    def casts(self): pass
    def workspace(self, b, f32, bf, u8): return {}
    def row_mask(self, ws): return None

    def forward(self, bm, ws, need_grad):
        self._lookup(self._indices(bm["tokens"], "tokens", ws["b"]), ws, self.enc.positional_encoder.pe, False)

    def det_shapes(self, b):
        """the deterministic launch of backward(): the table gradient"""
        return dict(emb=[b * self.n])

    def backward(self, ws, dx, on_side):
        self._table_backward(ws, dx)


class SparseTabularStep(_ValueChain, _TableLookup):
    """SparseTabularEncoder: the value chain of `data` written into the packed token matrix (zero where data == padding_idx), then
    E[indices] added onto it, unmasked (encoders.py:114-120)."""

    def __init__(self, engine, name, mi, enc):
        super().__init__(engine, name, mi, enc)
        self._table_init()

    def forward(self, bm, ws, need_grad):
        b = ws["b"]
        idx, vals = self._indices(bm["indices"], "indices", b), bm["data"]
        if vals.dtype != torch.float32 or not vals.is_contiguous():
            vals = vals.float().contiguous()
        if vals.shape != (b, self.n):
            raise AssertionError(f"{self.name}: data {tuple(vals.shape)} != {(b, self.n)}")
        self._value_forward(vals, ws, None)
        self._lookup(idx, ws, None, True)

    def det_shapes(self, b):
        """the deterministic launches of backward(): the table gradient, then the value chain's"""
        return dict(emb=[b * self.n], **self._value_det_shapes(b))

    def backward(self, ws, dx, on_side):
        self._table_backward(ws, dx)
        self._value_backward(ws, dx, on_side)


class PatchStep(_Step):
    """PatchEncoder: `mca_patch_ln_fwd` (patch gather, LayerNorm(P), bf16 out, pad mask: launched by attention_mask(), before the
    masks are packed) -> `mca_gemm_nt` + bias -> `mca_layernorm_fwd` (+ the learned position table, written into the packed token
    matrix).  Padded tokens are not zeroed (encoders.py:268-274): no LayerNorm here takes a row mask."""
    native = True

    def __init__(self, engine, name, mi, enc):
        super().__init__(engine, name, mi, enc)
        self.P = self._patch_elements(enc)
        self.kp = (self.P + 63) // 64 * 64          # the Linear's input width, padded to 64
        self.w, self.wT = self._bf16(self.D, self.kp), self._bf16(self.kp, self.D)

    def _patch_elements(self, enc):
        self.p1, self.p2 = int(enc.patch_size[0]), int(enc.patch_size[1])
        return self.p1 * self.p2

    def casts(self):
        self.eng._cast(self.enc.batch_to_tokens[2].weight.data, self.w)
        self.eng._cast(self.enc.batch_to_tokens[2].weight.data, self.wT, transpose=True)

    def workspace(self, b, f32, bf, u8):
        rows, D, kp = b * self.n, self.D, self.kp
        return dict(xp=f32(rows, self.P), xin_b=bf(rows, kp), m0=f32(rows), r0=f32(rows), y=f32(rows, D), m2=f32(rows), r2=f32(rows),
                    dy=f32(rows, D), dy_b=bf(rows, D), dxin=f32(rows, kp), mask=u8(rows))

    def row_mask(self, ws):
        return None          # (its mask comes from the values: mca_patch_ln_fwd)

    def attention_mask(self, bm, ws):
        """checks `values`, runs the front-end kernel and returns the mask it wrote, (b, n) uint8"""
        from .engine import LN_EPS          # (here: engine imports this module)
        n, b, p1, p2 = self.n, ws["b"], self.p1, self.p2
        e, bt = ws["enc"][self.name], self.enc.batch_to_tokens
        vals = bm["values"]
        if vals.dtype != torch.float32 or not vals.is_contiguous():
            vals = vals.float().contiguous()
        if vals.dim() != 3 or vals.shape[0] != b:
            raise AssertionError(f"{self.name}: values {tuple(vals.shape)} is not (b = {b}, H, W)")
        H, W = vals.shape[1], vals.shape[2]
        if H % p1 or W % p2:
            raise AssertionError(f"{self.name}: values {tuple(vals.shape)} is not a whole number of {(p1, p2)} patches")
        grid = (H // p1) * (W // p2)
        if grid != n:
            raise AssertionError(f"{grid} - {n}")                  # encoders.py:270
        e["values"] = vals
        call("mca_patch_ln_fwd", ptr(vals), H * W, W, b, H, W, p1, p2, ptr(bt[1].weight.data), ptr(bt[1].bias.data),
             float(self.enc.pad_token), LN_EPS, ptr(e["xp"]), ptr(e["xin_b"]), self.kp, self.kp, ptr(e["m0"]), ptr(e["r0"]),
             ptr(e["mask"]), stream_ptr())
        return e["mask"].view(b, n)

    def forward(self, bm, ws, need_grad):
        eng, n, D, rows = self.eng, self.n, self.D, ws["b"] * self.n
        e, bt = ws["enc"][self.name], self.enc.batch_to_tokens
        eng.gemm_nt(e["xin_b"], self.w, e["y"], rows, D, self.kp, bias=bt[2].bias)
        eng.ln_fwd(e["y"], bt[3].weight, rows, D, e["m2"], e["r2"], beta=bt[3].bias, add=self.enc.embedding.weight.data, period=n,
                   y=ws["x"][0][self.off:], ldy=D, y_bstride=self.N * D)

    def det_shapes(self, b):
        """the deterministic launches of backward(): two LayerNorm backwards, one weight gradient, the position table's row sum"""
        rows = b * self.n
        return dict(ln=[(rows, self.D), (rows, self.P)], tn=[(rows, self.D, self.P)], rr=[(rows, self.n)])

    def backward(self, ws, dx, on_side):
        eng, n, off, D, N, G, P, kp = self.eng, self.n, self.off, self.D, self.N, self.G, self.P, self.kp
        e, bt, rows = ws["enc"][self.name], self.enc.batch_to_tokens, ws["b"] * n
        # the table is added to every row, padded or not: every row of dx reaches it (no frozen row: no padding_idx)
        eng._reduce_rows(ws, dx.data_ptr() + off * D * 4, D, N * D, n, ptr(G(self.enc.embedding.weight)), D, rows, D)
        # (the Linear's bias gradient = column sums of this norm's dx: same launch)
        eng._ln_bwd(ws, dx[off:], D, e["y"], bt[3].weight, e["m2"], e["r2"], rows, D, G(bt[3].weight), dbeta=G(bt[3].bias),
                    dx=e["dy"], dx_bf16=e["dy_b"], y_bstride=N * D, period=n, dxsum=G(bt[2].bias))
        on_side(lambda e=e, bt=bt, rows=rows: eng._tn(ws, e["dy_b"], e["xin_b"], G(bt[2].weight), rows, D, P))
        eng.gemm_nt(e["dy_b"], self.wT, e["dxin"], rows, kp, D)
        # parameters only: the matrix needs no gradient
        eng._ln_bwd(ws, e["dxin"], kp, e["xp"], bt[1].weight, e["m0"], e["r0"], rows, P, G(bt[1].weight), dbeta=G(bt[1].bias))


class PatchNDStep(PatchStep):
    """ImagePatchEncoder / VideoPatchEncoder: PatchStep with `mca_patch_nd_ln_fwd` as its front end: values (b, C, H, W) or
    (b, C, T, H, W), P = C * pt * p1 * p2 (an image has pt = T = 1).  Everything behind the gather - workspace, forward, backward,
    deterministic launches - is PatchStep's."""

    def _patch_elements(self, enc):
        self.C, (self.pt, self.p1, self.p2) = enc.num_channels, enc.patch
        return self.C * self.pt * self.p1 * self.p2

    def attention_mask(self, bm, ws):
        """checks `values`, runs the front-end kernel and returns the mask it wrote, (b, n) uint8"""
        from .engine import LN_EPS          # (here: engine imports this module)
        n, b, C, pt, p1, p2 = self.n, ws["b"], self.C, self.pt, self.p1, self.p2
        e, bt, image = ws["enc"][self.name], self.enc.batch_to_tokens, self.enc.ndim == 2
        vals = bm["values"]
        if vals.dtype != torch.float32 or not vals.is_contiguous():
            vals = vals.float().contiguous()
        if vals.dim() != (4 if image else 5) or vals.shape[0] != b or vals.shape[1] != C:
            raise AssertionError(f"{self.name}: values {tuple(vals.shape)} is not (b = {b}, C = {C}, {'H, W' if image else 'T, H, W'})")
        T, H, W = (1, *vals.shape[2:]) if image else vals.shape[2:]
        if T % pt or H % p1 or W % p2:
            raise AssertionError(f"{self.name}: values {tuple(vals.shape)} is not a whole number of {tuple(self.enc.patch_size)} patches")
        grid = (T // pt) * (H // p1) * (W // p2)
        if grid != n:
            raise AssertionError(f"{grid} - {n}")                  # encoders.py:270
        e["values"] = vals
        call("mca_patch_nd_ln_fwd", ptr(vals), C * T * H * W, T * H * W, H * W, W, b, C, T, H, W, pt, p1, p2, ptr(bt[1].weight.data),
             ptr(bt[1].bias.data), float(self.enc.pad_token), LN_EPS, ptr(e["xp"]), ptr(e["xin_b"]), self.kp, self.kp, ptr(e["m0"]),
             ptr(e["r0"]), ptr(e["mask"]), stream_ptr())
        return e["mask"].view(b, n)


class ForeignStep(_Step):
    """A user-registered torch encoder: it runs under autograd and feeds its tokens to the native trunk.  No bf16 copies, no
    workspace buffers, no deterministic launches (torch's own backward is not held to bit-equality)."""
    native = False

    def casts(self): pass
    def workspace(self, b, f32, bf, u8): return {}
    def det_shapes(self, b): return {}

    def forward(self, bm, ws, need_grad):
        n, off, D, N, b = self.n, self.off, self.D, self.N, ws["b"]
        with torch.enable_grad() if need_grad else torch.no_grad():
            toks, amask = self.enc(bm)
        ws["foreign"][self.name] = toks
        ws["x"][0].view(b, N, D)[:, off:off + n].copy_(toks.detach().float())
        ws["padding"].view(b, N)[:, off:off + n].copy_(amask.to(torch.bool))
        ws["present"] |= ((amask == 0).sum(dim=1) != 0).to(torch.int32) << self.mi

    def backward(self, ws, dx, on_side):
        toks = ws["foreign"][self.name]
        if toks.requires_grad:
            # the foreign encoder's parameters live in the flat buffers too: point their .grad at the flat views so
            # that autograd ACCUMULATES in place (FusedAdamW.zero_grad leaves None, and a fresh .grad tensor would be
            # replaced by the zeroed flat view after this backward)
            for p in self.enc.parameters():
                p.grad = self.G(p)
            torch.autograd.backward(toks, dx.view(ws["b"], self.N, self.D)[:, self.off:self.off + self.n].to(toks.dtype))


def step_for(engine, name, mi, enc):
    """The step object of modality `name` (index mi): the one place that looks at an encoder's type."""
    if isinstance(enc, EmbeddedSequenceEncoder):
        return SequenceStep(engine, name, mi, enc)
    if isinstance(enc, TabularEncoder):
        return TabularStep(engine, name, mi, enc)
    if isinstance(enc, SequenceEncoder):
        return TokenSequenceStep(engine, name, mi, enc)
    if isinstance(enc, SparseTabularEncoder):
        return SparseTabularStep(engine, name, mi, enc)
    if isinstance(enc, PatchEncoder):
        return PatchStep(engine, name, mi, enc)
    if isinstance(enc, (ImagePatchEncoder, VideoPatchEncoder)):
        return PatchNDStep(engine, name, mi, enc)
    return ForeignStep(engine, name, mi, enc)
