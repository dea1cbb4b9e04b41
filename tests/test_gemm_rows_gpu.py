"""mca_gemm_nt_res_lnbwd on the GPU against the two launches it replaces, mca_gemm_nt (fp32 output, residual) followed by
mca_layernorm_bwd (trunk form), on the same inputs: dx and its bf16 copy bit for bit, dgamma - which differs by the order of
its fp32 atomics only - against a float64 column sum with the bound tests/test_kernels_gpu.py uses for mca_layernorm_bwd.

Why equal bits are demanded: the full-row kernel multiplies in the operand order and k16-step order of the plain kernels, so an
accumulator is the same fp32 chain; dy = accumulator + residual is the plain epilogue's one add; the row body is the text of
ln_bwd_trunk_kernel (csrc/ln_rows.h).  Shapes: M = 5 (one partial tile), 128 (one exact tile), 165 (a clamped tail, and an odd
last row in the two-rows-per-wavefront pairing), 257 (three tiles, the last of one row); K = 96 (the three stages of the prologue
and nothing else), 128 (one step of the loop), 1408 (44 steps: every slot reused many times).  mca_gemm_nt takes K % 64 == 0 only,
so at K = 96 the pair runs on copies of A and B with 32 zero columns appended: each adds an exact zero to the chain.  Operands sit
in NaN frames with padded strides, outputs in sentinel frames that must come back untouched."""
import importlib

import pytest
import torch

import gemm_edge_util as U

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
N = 512
DGAMMA_REL = 2e-5          # tests/test_kernels_gpu.py::test_layernorm_fwd_bwd, dgamma against autograd in the same way


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def case(M, K, seed=7):
    g = gen(seed)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    A, B = U.framed_copy(rn(M, K).to(BF), K + 8), U.framed_copy((rn(N, K) * K ** -0.5).to(BF), K + 16)
    x = U.framed_copy(rn(M, N) * 1.5 + 0.25, N + 4)
    res = U.framed_copy(rn(M, N), N + 8)
    gamma = rn(N) * 0.5 + 1.0
    mean, rstd = U.ln_stats32(x)
    return A, B, x, res, gamma, mean.contiguous(), rstd.contiguous()


def pair(H, A, B, x, res, gamma, mean, rstd, M, K):
    """the two launches: dy = A.B^T (+ res) in fp32, then the LayerNorm backward -> (dy, dx, dx_bf16, dgamma)"""
    if K % 64:          # zero columns up to the plain kernel's K % 64 == 0
        Kp = (K + 63) // 64 * 64
        Ap, Bp = torch.zeros(M, Kp, dtype=BF, device="cuda"), torch.zeros(N, Kp, dtype=BF, device="cuda")
        Ap[:, :K], Bp[:, :K] = A, B
        A, B, K = Ap, Bp, Kp
    dy = torch.empty(M, N, device="cuda")
    dx, dxb, dgamma = torch.empty(M, N, device="cuda"), torch.empty(M, N, dtype=BF, device="cuda"), torch.zeros(N, device="cuda")
    H.call("mca_gemm_nt", A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), dy.data_ptr(), N, 0, None, H.ptr(res),
           res.stride(0) if res is not None else 0, 0, M, N, K, H.stream_ptr())
    H.call("mca_layernorm_bwd", dy.data_ptr(), N, 0, 0, x.data_ptr(), x.stride(0), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None,
           dx.data_ptr(), N, dxb.data_ptr(), N, dgamma.data_ptr(), None, None, M, N, H.stream_ptr())
    return dy, dx, dxb, dgamma


def fused(H, A, B, x, res, gamma, mean, rstd, M, K, dx, dxb, dgamma):
    H.call("mca_gemm_nt_res_lnbwd", A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), H.ptr(res), res.stride(0) if res is not None else 0,
           x.data_ptr(), x.stride(0), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), dx.data_ptr(), dx.ld, dxb.data_ptr(), dxb.ld,
           dgamma.data_ptr(), M, N, K, H.stream_ptr())


def dgamma64(dy, x, mean, rstd):
    return (dy.double() * (x.double() - mean.double()[:, None]) * rstd.double()[:, None]).sum(0)


def guarded_dgamma():
    buf = torch.full((N + 64,), 7.0, device="cuda")
    buf[:N] = 0
    return buf


def check(H, M, K, with_res=True, in_place=False):
    A, B, x, res, gamma, mean, rstd = case(M, K)
    if not with_res:
        res = None
    dy, dx_ref, dxb_ref, dg_ref = pair(H, A, B, x, res, gamma, mean, rstd, M, K)
    dx, dxb, dgamma = U.guarded_out(M, N, N + 8, torch.float32, device="cuda"), U.guarded_out(M, N, N + 8, BF, device="cuda"), guarded_dgamma()
    r = res
    if in_place:          # dx is the residual: read and written by the same wavefront, row by row
        dx.t.copy_(res)
        r = dx.t
    fused(H, A, B, x, r, gamma, mean, rstd, M, K, dx, dxb, dgamma)
    torch.cuda.synchronize()
    assert torch.isfinite(dx_ref).all() and torch.isfinite(dg_ref).all()          # no NaN of a frame was read by the pair
    ndx, nb = int((bits(dx.t) != bits(dx_ref)).sum()), int((bits(dxb.t) != bits(dxb_ref)).sum())
    ref64 = dgamma64(dy, x, mean, rstd)
    e_f, e_p = rel(dgamma[:N], ref64), rel(dg_ref, ref64)
    print(f"rows lnbwd M={M} K={K} res={with_res} in_place={in_place}: dx differs at {ndx}, dx_bf16 at {nb} elements; "
          f"dgamma rel to fp64: fused {e_f:.2e}, pair {e_p:.2e}")
    assert ndx == 0, f"dx differs at {ndx} of {M * N} elements"
    assert nb == 0, f"dx_bf16 differs at {nb} of {M * N} elements"
    assert e_f < DGAMMA_REL, e_f
    U.assert_guard_intact(dx, "dx")
    U.assert_guard_intact(dxb, "dx_bf16")
    assert bool((dgamma[N:] == 7.0).all()), "dgamma: stored past column 512"


@pytest.mark.parametrize("K", [96, 128, 1408])
@pytest.mark.parametrize("M", [5, 128, 165, 257])
def test_res_lnbwd_equals_the_pair(H, M, K):
    check(H, M, K)


@pytest.mark.parametrize("M,K", [(165, 128), (257, 1408)])
def test_res_lnbwd_in_place(H, M, K):
    check(H, M, K, in_place=True)


@pytest.mark.parametrize("M,K", [(165, 96), (257, 1024)])
def test_res_lnbwd_without_residual(H, M, K):
    """the final norm's backward behind the pooling kv data gradient"""
    check(H, M, K, with_res=False)
