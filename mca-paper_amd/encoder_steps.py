"""One step object per encoder kind: what FusionEngine needs from a modality's encoder - its bf16 weight copies and their cast records,
its workspace buffers, the shapes of its deterministic launches, its forward and its backward.  The engine builds one per modality
(step_for, the only place that looks at an encoder's type) and loops over them: a new encoder kind is a class here and a line in
step_for.  Reference lines: encoders.py:196-214 (EmbeddedSequenceEncoder), :90-96 (TabularEncoder).
This module binds its own `call` from .hip: a tool that records launches by rebinding `call` patches hip, engine AND this module."""
from __future__ import annotations

import torch

from .encoders import EmbeddedSequenceEncoder, TabularEncoder
from .hip import call, ptr, stream_ptr


class _Step:
    def __init__(self, engine, name, mi, enc):
        self.eng, self.name, self.mi, self.enc = engine, name, mi, enc
        self.n, self.off = engine.st.token_dims[mi], engine.offsets[mi]          # tokens per sample, first row in the packed (N, D) sample
        self.D, self.N, self.G = engine.D, engine.N, engine.grad_of

    def _bf16(self, *shape):
        return torch.zeros(*shape, dtype=torch.bfloat16, device=self.eng.device)


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


class TabularStep(_Step):
    """TabularEncoder: E[t] (max_norm-renormalised in place) + LN(Linear2(ReLU(Linear1(min(x, max))))), the value part zeroed where
    x == padding_idx (-1).  The trunk's key-padding mask is the collator's attention_mask."""
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

    def forward(self, bm, ws, need_grad):
        eng, enc, n, D, b = self.eng, self.enc, self.n, self.D, ws["b"]
        e, ve, rows = ws["enc"][self.name], enc.value_encoder, b * n
        vals = bm["values"]
        if vals.dtype != torch.float32 or not vals.is_contiguous():
            vals = vals.float().contiguous()
        if vals.shape != (b, n):
            raise AssertionError(f"{vals.shape[1]} - {n}")                  # encoders.py:93
        e["values"] = vals
        emb = enc.token_encoder.embedding.weight
        call("mca_embedding_renorm", ptr(emb.data), n, D, float(enc.token_encoder.max_norm), stream_ptr())
        call("mca_tab_value_fwd", ptr(vals), ptr(ve.linear1.weight.data), ptr(ve.linear1.bias.data), ptr(e["h1_b"]), ptr(e["mask"]),
             rows, D, float(ve.max_value), float(ve.padding_value), stream_ptr())
        eng.gemm_nt(e["h1_b"], self.w2, e["y"], rows, D, D, bias=ve.linear2.bias)
        eng.ln_fwd(e["y"], ve.norm.weight, rows, D, e["m2"], e["r2"], beta=ve.norm.bias, rowmask=e["mask"], add=emb.data,
                   period=n, y=ws["x"][0][self.off:], ldy=D, y_bstride=self.N * D)

    def det_shapes(self, b):
        """the deterministic launches of backward(): the table's row sum, one LayerNorm backward, one weight gradient, Linear1"""
        rows, D = b * self.n, self.D
        return dict(rr=[(rows, self.n)], ln=[(rows, D)], tn=[(rows, D, D)], tab=[rows])

    def backward(self, ws, dx, on_side):
        eng, n, off, D, N, G = self.eng, self.n, self.off, self.D, self.N, self.G
        e, ve, rows = ws["enc"][self.name], self.enc.value_encoder, ws["b"] * n
        gemb = G(self.enc.token_encoder.embedding.weight)
        # the table is added after the value path is masked: every row of dx reaches it; padding_idx row stays frozen
        eng._reduce_rows(ws, dx.data_ptr() + off * D * 4, D, N * D, n, ptr(gemb), D, rows, D)
        gemb[n - 1].zero_()
        eng._ln_bwd(ws, dx[off:], D, e["y"], ve.norm.weight, e["m2"], e["r2"], rows, D, G(ve.norm.weight), dbeta=G(ve.norm.bias),
                    rowmask=e["mask"], dx=e["dy"], dx_bf16=e["dy_b"], y_bstride=N * D, period=n, dxsum=G(ve.linear2.bias))
        on_side(lambda e=e, ve=ve, rows=rows: eng._tn(ws, e["dy_b"], e["h1_b"], G(ve.linear2.weight), rows, D, D))
        eng.gemm_nt(e["dy_b"], self.w2T, e["dh1"], rows, D, D)
        eng._sum_launch(ws, "mca_tab_value_bwd", (ptr(e["dh1"]), D, ptr(e["h1_b"]), ptr(e["values"]), ptr(G(ve.linear1.weight)),
                                                  ptr(G(ve.linear1.bias)), rows, D, float(ve.max_value)), lambda: (rows, D))


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
    return ForeignStep(engine, name, mi, enc)
