"""The checker of the GEMM edge tests, checked (no GPU): a torch emulation of a kernel writes into the guarded buffers of
tests/gemm_edge_util.py; every way a kernel can be wrong in a few places makes the helpers raise, the correct emulation passes,
and the references alone - rounded as the kernels round, computed in fp32 as the kernels compute - satisfy every derived
element-wise bound of the GPU tests with no element left out."""
import pytest
import torch

import gemm_edge_util as U

M, N, K, LDA, LDC = 37, 21, 64, 72, 24


def gen(seed=0):
    return torch.Generator().manual_seed(seed)


def wide(view, ld, rows_before=0, rows_after=0):
    """the same memory with the padding columns (and guard rows) in sight"""
    return torch.as_strided(view, (view.shape[0] + rows_before + rows_after, ld), (ld, 1), view.storage_offset() - rows_before * ld)


def operands(seed=0):
    g = gen(seed)
    return U.int_bf16(M, K, LDA, g), U.int_bf16(N, K, LDA, g), U.int_f32(1, N, N, g), U.int_f32(M, N, LDC, g, byte_off=4)


def emulate(A, B, bias, res, out, k_read=K, skip=None):
    """C = A B^T + bias + res in fp32 (exact for these operands), stored into the guarded view element by element"""
    acc = wide(A, LDA)[:, :k_read].float() @ wide(B, LDA)[:, :k_read].float().t() + bias.float() + res.float()
    val = acc.to(out.dtype)
    if skip is not None:
        val[skip] = out.t[skip]          # that element is not stored
    out.t.copy_(val)


def reference(A, B, bias, res, dtype):
    r = U.matmul64(A, B) + bias.double() + res.double()
    return r.float() if dtype == torch.float32 else r.to(torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("byte_off", [0, 1])
def test_correct_emulation_passes(dtype, byte_off):
    A, B, bias, res = operands()
    out = U.guarded_out(M, N, LDC, dtype, byte_off=byte_off * torch.empty((), dtype=dtype).element_size())
    assert out.t.data_ptr() % 16 == (byte_off * out.es) and out.t.stride(0) == LDC and torch.isnan(out.t).all()
    assert A.data_ptr() % 16 == 0 and A.stride(0) == LDA and res.data_ptr() % 16 == 4
    emulate(A, B, bias, res, out)
    U.assert_exact(out.t, reference(A, B, bias, res, dtype))
    U.assert_guard_intact(out)


def test_operands_are_integers_inside_nan():
    A, _, _, res = operands()
    assert (A.float() == A.float().round()).all() and A.float().abs().max() == 2 and (res == res.round()).all()
    w = wide(A, LDA, U.GUARD_ROWS, U.GUARD_ROWS)
    assert torch.isnan(w[:U.GUARD_ROWS]).all() and torch.isnan(w[-U.GUARD_ROWS:]).all() and torch.isnan(w[U.GUARD_ROWS:-U.GUARD_ROWS, K:]).all()
    assert torch.isnan(wide(res, LDC, U.GUARD_ROWS, U.GUARD_ROWS)).sum() == (M + 2 * U.GUARD_ROWS) * LDC - M * N
    S = U.int_bf16(5, 8, 8, gen(), scale=2.0 ** -4, poison=False)
    assert ((S.float() * 16) == (S.float() * 16).round()).all() and (wide(S, 8, 1, 1)[0] == 0).all()


def test_one_element_off_by_one_bf16_step():
    A, B, bias, res = operands()
    out = U.guarded_out(M, N, LDC, torch.bfloat16)
    emulate(A, B, bias, res, out)
    ref = reference(A, B, bias, res, torch.bfloat16)
    U.assert_exact(out.t, ref)
    assert float(out.t[M - 1, N - 1]) != 0
    out.t.view(torch.int16)[M - 1, N - 1] += 1
    with pytest.raises(AssertionError, match=rf"1 of {M * N} elements wrong.*\({M - 1}, {N - 1},"):
        U.assert_exact(out.t, ref)
    U.assert_guard_intact(out)


def test_one_element_stale():
    A, B, bias, res = operands()
    # a fresh output: the element nobody stored still holds the sentinel
    out = U.guarded_out(M, N, LDC, torch.float32)
    emulate(A, B, bias, res, out, skip=(5, 20))
    with pytest.raises(AssertionError, match=r"1 of .*\(5, 20,"):
        U.assert_exact(out.t, reference(A, B, bias, res, torch.float32))
    # an accumulated output (weight gradient): the element keeps its initial integer
    acc = U.guarded_out(M, N, LDC, torch.float32)
    acc.t.copy_(res)
    prod = U.matmul64(A, B)
    i, j = [int(v) for v in (prod != 0).nonzero()[0]]
    val = (res.double() + prod).float()
    val[i, j] = res[i, j]
    acc.t.copy_(val)
    with pytest.raises(AssertionError, match=rf"1 of .*\({i}, {j},"):
        U.assert_exact(acc.t, (res.double() + prod).float())
    U.assert_guard_intact(acc)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("where", ["column N", "last padding column", "row M", "row -1", "eight rows behind"])
def test_a_store_outside_the_view(dtype, where):
    A, B, bias, res = operands()
    out = U.guarded_out(M, N, LDC, dtype, byte_off=0 if where == "row M" else torch.empty((), dtype=dtype).element_size())
    emulate(A, B, bias, res, out)
    w = wide(out.t, LDC, U.GUARD_ROWS, U.GUARD_ROWS)
    r, c = {"column N": (3, N), "last padding column": (M - 1, LDC - 1), "row M": (M, 0), "row -1": (-1, N - 1),
            "eight rows behind": (M + U.GUARD_ROWS - 1, 2)}[where]
    w[U.GUARD_ROWS + r, c] = 1.0
    U.assert_exact(out.t, reference(A, B, bias, res, dtype))          # the values are all right ...
    with pytest.raises(AssertionError, match=rf"guard bytes overwritten.*\({r}, {c}\)"):
        U.assert_guard_intact(out)                                    # ... the store is found, and where


def test_a_read_of_the_operand_padding():
    A, B, bias, res = operands()
    out = U.guarded_out(M, N, LDC, torch.float32)
    emulate(A, B, bias, res, out, k_read=LDA)          # A[:, :ld] and not A[:, :K]
    with pytest.raises(AssertionError, match=rf"{M * N} of {M * N} elements wrong"):
        U.assert_exact(out.t, reference(A, B, bias, res, torch.float32))
    # one row too many read (a missing clamp at row M) reaches only that tile's last row in a real kernel; here: the row after
    below = wide(A, LDA, 0, 1)[1:, :K]
    out2 = U.guarded_out(M, N, LDC, torch.float32)
    out2.t.copy_(below.float() @ B.float().t())
    assert torch.isnan(out2.t[M - 1]).all() and not torch.isnan(out2.t[:M - 1]).any()


def test_close_elementwise_reports_and_rejects_nan():
    ref = torch.arange(12.0).reshape(3, 4).double()
    tol = torch.full_like(ref, 0.5)
    got = ref.clone().float()
    U.assert_close_elementwise(got, ref, tol)
    got[1, 2] += 0.75
    with pytest.raises(AssertionError, match=r"1 of 12 elements wrong.*\(1, 2,"):
        U.assert_close_elementwise(got, ref, tol)
    got[1, 2] = float("nan")
    with pytest.raises(AssertionError, match=r"\(1, 2,"):
        U.assert_close_elementwise(got, ref, tol)
    with pytest.raises(AssertionError):
        U.assert_exact(got.double(), got.double())          # NaN never equals


# ---- the bounds are satisfiable: the reference alone, computed and rounded as the kernels do, meets them at every element
def test_fp32_accumulation_is_exact_in_any_order():
    g = gen(3)
    for Kk, scale in [(512, 1.0), (320, 2.0 ** -4)]:
        A, B = U.int_bf16(64, Kk, Kk + 8, g), U.int_bf16(48, Kk, Kk, g, scale=scale)
        ref = U.matmul64(A, B)
        assert ref.abs().max() <= 4 * Kk * scale and (ref.float().double() == ref).all()
        perm = torch.randperm(Kk, generator=g)
        acc = torch.zeros(64, 48)
        for k0 in range(0, Kk, 32):          # fp32 adds, 32 columns at a time, in a shuffled order
            idx = perm[k0:k0 + 32]
            acc = acc + A[:, idx].float() @ B[:, idx].float().t()
        assert torch.equal(acc, ref.float())
        # weight gradient: |sum| <= 4 R
        assert torch.equal(A.float().t() @ A.float(), (A.double().t() @ A.double()).float())


def gelu_pair32(x):
    """gelu and gelu' in fp32 with the exact erf: what csrc/common.h computes, up to its erf approximation"""
    cdf = 0.5 * (1.0 + torch.erf(x * 0.70710678118654752))
    return x * cdf, cdf + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


@pytest.mark.parametrize("D", [192, 320])
def test_geglu_forward_bound_is_satisfiable(D):
    g = gen(5)
    rows, ip = 300, 128
    x, w1 = U.int_bf16(rows, D, D, g), U.int_bf16(2 * ip, D, D, g, scale=2.0 ** -4)
    h64 = U.matmul64(x, w1)
    assert (h64.float().double() == h64).all()          # exact in fp32: h is then one rounding away
    h = h64.to(torch.bfloat16)
    assert 1.5 < float(h[:, ip:].float().std()) < 2.4          # the gates are spread out, not at integer points only
    a, gate = h[:, :ip].float(), h[:, ip:].float()
    got = (a * gelu_pair32(gate)[0]).to(torch.bfloat16)
    ref, tol = U.geglu_fwd_ref(h, ip)
    U.assert_close_elementwise(got, ref, tol)


def test_geglu_backward_bound_is_satisfiable():
    g = gen(6)
    rows, ip, D = 300, 72, 320
    h = torch.randn(rows, 2 * ip, generator=g).to(torch.bfloat16)
    dx, w2T = U.int_bf16(rows, D, D, g), U.int_bf16(ip, D, D, g, scale=2.0 ** -4)
    dg = U.matmul64(dx, w2T)
    assert (dg.float().double() == dg).all()
    a, gate = h[:, :ip].float(), h[:, ip:].float()
    ge, dge = gelu_pair32(gate)
    got = torch.cat([(dg.float() * ge).to(torch.bfloat16), (dg.float() * a * dge).to(torch.bfloat16)], 1)
    ref, tol = U.geglu_bwd_ref(dg, h, ip)
    U.assert_close_elementwise(got, ref, tol)


def test_lnres_bound_is_satisfiable():
    g = gen(7)
    Mm, Nn, Kk = 300, 128, 512
    A, B = U.int_bf16(Mm, Kk, Kk, g), U.int_bf16(Nn, Kk, Kk, g)
    x = torch.randn(Mm, Nn, generator=g) * 3 + 0.5
    gamma = torch.randn(Nn, generator=g)
    mean, rstd = U.ln_stats32(x)
    acc = U.matmul64(A, B)
    got = acc.float() + (x - mean[:, None]) * rstd[:, None] * gamma[None, :]          # the epilogue's roundings, in fp32
    ref, tol = U.lnres_ref(acc, x, mean, rstd, gamma)
    U.assert_close_elementwise(got, ref, tol)
    assert float((tol / ref.abs().clamp_min(1e-3)).median()) < 1e-5          # ... and the bound is tight: a few 1e-6 of the value
