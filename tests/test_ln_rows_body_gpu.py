"""The trunk LayerNorm backward's row body (csrc/ln_rows.h) against a float64 evaluation of the same formula, in both kernels that
compile it: ln_bwd_trunk_kernel<NI> (mca_layernorm_bwd at 256, 512 and 1,024 columns) and the epilogue of gemm_nt_rows_kernel
(mca_gemm_nt_res_lnbwd, 512 columns).  tests/test_gemm_rows_gpu.py holds the two kernels to each other bit for bit, which says
nothing about the body they share; this is its independent reference.

The bound is worked out from the body's fp32 roundings, u = 2^-24, with dy, x, gamma and the fp32 mean / rstd taken as exact
inputs (the reference reads the same fp32 values).  Per element, as absolute errors in units of rstd:
  g = dy * gamma                        one rounding:                                         u |g|
  s1 = mean(g)                          the rounding of every g, then a chain of 4 NI lane adds, 6 shuffle adds and the
                                        multiplication by 1 / cols:                           (4 NI + 8) u mean|g|
  xhat = (x - mean) * rstd              two roundings, and xhat enters dx as xhat * s2:       2 u |xhat| |s2|
  s2 = mean(g * xhat)                   three roundings in every product, then the chain of s1 with the first add fused:
                                                                                              (4 NI + 10) u |xhat| mean|g xhat|
  rstd * fma(-xhat, s2, g - s1)         three roundings of the result:                        3 u |g - s1 - xhat s2|
With rms(xhat) <= 1 (so mean|g xhat| and |s2| are at most rms(g)) and |g - s1 - xhat s2| <= |g| in norm (an orthogonal projection
of g), the norm of a row's error is at most (1 + 4 NI + 8 + 2 + 4 NI + 10 + 3) u = (8 NI + 24) u times rstd ||g||: 40 u at 512
columns.  The test computes rstd ||g|| row by row, so nothing is assumed about how much of g the projection removes."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def inputs(M, cols, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x = rn(M, cols) * 1.5 + 0.25
    xd = x.double()
    mean, rstd = xd.mean(1).float(), (1.0 / torch.sqrt(xd.var(1, unbiased=False) + 1e-5)).float()
    return x, rn(cols) * 0.5 + 1.0, mean, rstd


def dx64(dy, x, gamma, mean, rstd):
    """(dx in float64, the norm the bound is relative to: that of rstd * g over all rows)"""
    r = rstd.double()[:, None]
    xh = (x.double() - mean.double()[:, None]) * r
    g = dy.double() * gamma.double()[None, :]
    dx = r * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return dx, float((r * g).norm())


def held(tag, dx, dxb, ref, scale, NI):
    bound = (8 * NI + 24) * U32
    e32 = float((dx.double() - ref).norm()) / scale
    e16 = float((dxb.double() - ref).norm()) / float(ref.norm())
    print(f"ln rows body {tag}: dx error {e32:.2e} of rstd |g| (bound {bound:.2e}), bf16 copy {e16:.2e} of |dx|")
    assert e32 <= bound, (tag, e32, bound)
    assert e16 <= 2.0 ** -9 + bound * scale / float(ref.norm()), (tag, e16)          # one bf16 rounding of every element on top
    assert torch.equal(dxb, dx.to(BF))                                                # the copy is the rounded dx


@pytest.mark.parametrize("cols", [256, 512, 1024])
@pytest.mark.parametrize("M", [5, 165, 257])
def test_layernorm_bwd_trunk_dx_against_float64(H, M, cols):
    x, gamma, mean, rstd = inputs(M, cols, 11)
    dy = torch.randn(M, cols, device="cuda", generator=torch.Generator(device="cuda").manual_seed(12))
    dx, dxb, dgamma = torch.empty(M, cols, device="cuda"), torch.empty(M, cols, dtype=BF, device="cuda"), torch.zeros(cols, device="cuda")
    H.call("mca_layernorm_bwd", dy.data_ptr(), cols, 0, 0, x.data_ptr(), cols, gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None,
           dx.data_ptr(), cols, dxb.data_ptr(), cols, dgamma.data_ptr(), None, None, M, cols, H.stream_ptr())
    torch.cuda.synchronize()
    ref, scale = dx64(dy, x, gamma, mean, rstd)
    held(f"stand-alone M={M} cols={cols}", dx, dxb, ref, scale, cols // 256)


@pytest.mark.parametrize("M,K", [(5, 96), (165, 128), (257, 1408)])
def test_res_lnbwd_dx_against_float64(H, M, K):
    """dy is what mca_gemm_nt stores for the same operands: the fused kernel's accumulator chain and residual add are that
    kernel's (tests/test_gemm_rows_gpu.py), and the bound is about the row body behind them"""
    N = 512
    x, gamma, mean, rstd = inputs(M, N, 21)
    g = torch.Generator(device="cuda").manual_seed(22)
    A, B = torch.randn(M, K, device="cuda", generator=g).to(BF), (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(BF)
    res = torch.randn(M, N, device="cuda", generator=g)
    Kp = (K + 63) // 64 * 64          # mca_gemm_nt takes K % 64 == 0: zero columns add exact zeros to the chain
    Ap, Bp = torch.zeros(M, Kp, dtype=BF, device="cuda"), torch.zeros(N, Kp, dtype=BF, device="cuda")
    Ap[:, :K], Bp[:, :K] = A, B
    dy = torch.empty(M, N, device="cuda")
    H.call("mca_gemm_nt", Ap.data_ptr(), Kp, Bp.data_ptr(), Kp, dy.data_ptr(), N, 0, None, res.data_ptr(), N, 0, M, N, Kp, H.stream_ptr())
    dx, dxb, dgamma = torch.empty(M, N, device="cuda"), torch.empty(M, N, dtype=BF, device="cuda"), torch.zeros(N, device="cuda")
    H.call("mca_gemm_nt_res_lnbwd", A.data_ptr(), K, B.data_ptr(), K, res.data_ptr(), N, x.data_ptr(), N, mean.data_ptr(), rstd.data_ptr(),
           gamma.data_ptr(), dx.data_ptr(), N, dxb.data_ptr(), N, dgamma.data_ptr(), M, N, K, H.stream_ptr())
    torch.cuda.synchronize()
    ref, scale = dx64(dy, x, gamma, mean, rstd)
    held(f"fused M={M} K={K}", dx, dxb, ref, scale, 2)
