"""Helpers of the GEMM edge tests (tests/test_gemm_edges_gpu.py; checked themselves by tests/test_gemm_edges_cpu.py).  Plain
functions on any device, no fixtures.

Operands whose products are exact: A and B hold integers in {-2 .. 2} (bf16, optionally scaled by a power of two), bias /
residual / initial C small integers in fp32.  Every partial sum is then an integer (or a multiple of the scale) far below
2^24, fp32 accumulation is exact in ANY order, and a kernel's output must equal the float64 reference bit for bit: as fp32, or
rounded once to nearest-even as bf16.  So every element is compared, and one wrong element fails.

Operands live inside NaN: the columns [cols, ld) of every row and GUARD_ROWS rows in front of and behind the matrix are NaN,
so a read outside the contract poisons the result.  Outputs live inside a sentinel: the same surroundings hold the byte 0xFF
(a NaN in both formats), and assert_guard_intact() finds any store to them; a stray store of a few rows or columns lands in
memory the test owns."""
import math

import torch

GUARD_ROWS = 8
SENTINEL = 0xFF          # every byte of a fresh guarded output: 0xFFFF / 0xFFFFFFFF are NaNs, so an element nobody stored fails too
SHOW = 8                 # bad elements a failure message lists


def _aligned_start(buf, want, align=16):
    """the smallest byte offset >= want into buf (uint8) at which the address is a multiple of align"""
    return want + (-(buf.data_ptr() + want)) % align


def _framed(rows, cols, ld, dtype, device, fill_byte, byte_off):
    """(uint8 allocation, byte offset of element (0, 0), the [rows, cols] view with row stride ld) with GUARD_ROWS rows of ld
    elements in front and behind; element (0, 0) sits byte_off bytes past a 16-byte boundary"""
    assert ld >= cols and rows > 0 and cols > 0
    es = torch.empty((), dtype=dtype).element_size()
    assert byte_off % es == 0
    nbytes = (rows + 2 * GUARD_ROWS) * ld * es + 32 + byte_off
    buf = torch.full((nbytes,), fill_byte, dtype=torch.uint8, device=device)
    start = _aligned_start(buf, GUARD_ROWS * ld * es) + byte_off
    view = buf[start:start + rows * ld * es].view(dtype).view(rows, ld)[:, :cols]
    assert view.data_ptr() == buf.data_ptr() + start and (view.data_ptr() - byte_off) % 16 == 0
    return buf, start, view


def _randint(lo, hi, shape, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen, device=gen.device)


def int_bf16(rows, cols, ld, gen, scale=1.0, poison=True):
    """[rows, cols] bf16 view (row stride ld, 16-byte aligned base) of integers in {-2 .. 2} times `scale` (a power of two).
    poison: columns [cols, ld) and GUARD_ROWS rows before and after are NaN (else zero)."""
    assert math.log2(scale) == int(math.log2(scale))
    buf, _, view = _framed(rows, cols, ld, torch.bfloat16, gen.device, 0xFF if poison else 0, 0)
    view.copy_((_randint(-2, 2, (rows, cols), gen).double() * scale).to(torch.bfloat16))
    return view


def int_f32(rows, cols, ld, gen, amp=8, byte_off=0, poison=True):
    """[rows, cols] fp32 view (row stride ld) of integers in {-amp .. amp}: bias, residual, initial C.  byte_off: the base sits
    that many bytes past a 16-byte boundary.  Padding as int_bf16."""
    _, _, view = _framed(rows, cols, ld, torch.float32, gen.device, 0xFF if poison else 0, byte_off)
    view.copy_(_randint(-amp, amp, (rows, cols), gen).float())
    return view


def framed_copy(src, ld, byte_off=0):
    """any 2-d tensor copied into a NaN frame with row stride ld (an input that is not integer-valued: h, x)"""
    _, _, view = _framed(src.shape[0], src.shape[1], ld, src.dtype, src.device, 0xFF, byte_off)
    view.copy_(src)
    return view


class Guarded:
    """A [rows, cols] output view `t` (row stride ld) inside a sentinel-filled allocation."""

    def __init__(self, rows, cols, ld, dtype, byte_off, device):
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        self.buf, self.start, self.t = _framed(rows, cols, ld, dtype, device, SENTINEL, byte_off)
        self.es = self.t.element_size()

    def data_ptr(self):
        return self.t.data_ptr()

    def _same_view(self, buf):
        return buf[self.start:self.start + self.rows * self.ld * self.es].view(self.dtype).view(self.rows, self.ld)[:, :self.cols]


def guarded_out(rows, cols, ld, dtype, byte_off=0, device="cpu"):
    """A fresh output: every byte of the allocation is SENTINEL, the view included (an element the kernel leaves out stays NaN)."""
    return Guarded(rows, cols, ld, dtype, byte_off, device)


def assert_guard_intact(g, what="output"):
    """Nothing but the view's own elements was stored to: rows -GUARD_ROWS .. -1, rows `rows` .. , and columns [cols, ld) of every
    row still hold the sentinel (compared as bytes)."""
    c = g.buf.clone()
    g._same_view(c).view(torch.uint8 if g.es == 1 else (torch.int16 if g.es == 2 else torch.int32)).fill_(-1)
    bad = (c != SENTINEL).nonzero().flatten()
    if bad.numel():
        rowbytes = g.ld * g.es
        where = sorted({((int(b) - g.start) // rowbytes, ((int(b) - g.start) % rowbytes) // g.es) for b in bad[:64 * g.es].tolist()})[:SHOW]
        raise AssertionError(f"{what}: {int(bad.numel())} guard bytes overwritten around a [{g.rows}, {g.cols}] view with ld {g.ld}; "
                             f"first (row, column): {where}")


def _report(bad, got, ref, extra=None):
    idx = bad.nonzero()[:SHOW].tolist()
    rows = [(i, j, float(got[i, j]), float(ref[i, j])) + ((float(extra[i, j]),) if extra is not None else ()) for i, j in idx]
    return f"{int(bad.sum())} of {bad.numel()} elements wrong; first (row, column, got, want{', bound' if extra is not None else ''}): {rows}"


def assert_exact(got, ref, what="output"):
    """got == ref at every element, as values (-0 == +0, any NaN fails); same shape and dtype"""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    bad = ~(got == ref)
    if bad.any():
        raise AssertionError(f"{what}: " + _report(bad, got, ref))


def assert_close_elementwise(got, ref, tol, what="output"):
    """|got - ref| <= tol at every element (float64; tol a tensor of ref's shape; NaN fails)"""
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    bad = ~((got.double() - ref.double()).abs() <= tol.double())
    if bad.any():
        raise AssertionError(f"{what}: " + _report(bad, got, ref, tol))


# ---- float64 references and the derived element-wise bounds (docs/parity.md, "GEMM edges")
BF16_STEP = 2.0 ** -8          # one bf16 step relative to the value: twice the half-step of round-to-nearest
GELU_ABS = 1e-6                # absolute error allowed on the normal cdf / gelu': 2.5 x (A&S erf 0.75e-7 + fp32 roundings + rcp / exp2)
LN_REL = 2.0 ** -20            # 16 fp32 unit round-offs against the five or so roundings of the LayerNorm epilogue


def matmul64(A, B):
    """A . B^T in float64"""
    return A.double() @ B.double().t()


def gelu64(x):
    x = x.double()
    return x * 0.5 * (1.0 + torch.erf(x * 0.7071067811865476))


def dgelu64(x):
    x = x.double()
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


def geglu_fwd_ref(h, ip):
    """(reference g, bound) from the CHECKED h = [a | gate]"""
    a, gate = h[:, :ip].double(), h[:, ip:2 * ip].double()
    ref = a * gelu64(gate)
    return ref, BF16_STEP * ref.abs() + GELU_ABS * (a * gate).abs()


def geglu_bwd_ref(dg, h, ip):
    """(reference dh = [dh_a | dh_gate], bound) from the exact dg (float64) and h = [a | gate]"""
    a, gate = h[:, :ip].double(), h[:, ip:2 * ip].double()
    ref_a, ref_g = dg * gelu64(gate), dg * a * dgelu64(gate)
    tol_a = BF16_STEP * ref_a.abs() + GELU_ABS * (dg * gate).abs()
    tol_g = BF16_STEP * ref_g.abs() + GELU_ABS * (dg * a).abs()
    return torch.cat([ref_a, ref_g], 1), torch.cat([tol_a, tol_g], 1)


def ln_stats32(x):
    """mean and rstd of every row in float64, rounded to fp32: given to the kernel AND to the reference"""
    xd = x.double()
    return xd.mean(1).float(), (1.0 / torch.sqrt(xd.var(1, unbiased=False) + 1e-5)).float()


def lnres_ref(acc, x, mean32, rstd32, gamma):
    """(reference acc + (x - mean) rstd gamma, bound) in float64"""
    xd, mu, rs, ga = x.double(), mean32.double()[:, None], rstd32.double()[:, None], gamma.double()[None, :]
    ref = acc + (xd - mu) * rs * ga
    return ref, LN_REL * (acc.abs() + (xd.abs() + mu.abs()) * rs * ga.abs())
