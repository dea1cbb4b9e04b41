"""mca_gemm_nt_res_lnbwd_tall with its 160-row kernel forced (knob 15 = 2) against the two launches it replaces, mca_gemm_nt (fp32
output, residual) followed by mca_layernorm_bwd, built and compared as tests/test_gemm_rows_gpu.py does for the 128-row kernel
(its helpers are used here): dx and its bf16 copy bit for bit - gemm_nt_rows160_kernel keeps the operand order and the ascending
k16-steps, so every accumulator is the same fp32 chain, and the row body is the same text - dgamma against the float64 column sum,
NaN-framed operands with padded strides, sentinel-framed outputs that must come back untouched.

Shapes: M = 5 (one partial tile; rows 128 .. 159 of the A image all clamped), 160 (one exact tile: the second A piece of waves
0 and 1 and the fifth epilogue pass carry real rows), 161 (a second tile of one row), 197 (a clamped tail of 37 rows, an odd last
row in the two-row pairing), 321 (three tiles, the last of one row); K = 96 (the prologue alone), 128 (one loop step), 1408 (44
steps: every slot reused many times, which is where a wait count that lets waves 0 / 1 read a stage one load early shows)."""
import ctypes as C
import importlib

import pytest
import torch

import gemm_edge_util as U
from test_gemm_rows_gpu import BF, DGAMMA_REL, N, bits, case, dgamma64, guarded_dgamma, pair, rel

pytestmark = pytest.mark.gpu
TALL = "mca_gemm_nt_res_lnbwd_tall"


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def fused(H, entry, A, B, x, res, gamma, mean, rstd, M, K, dx, dxb, dgamma):
    H.call(entry, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), H.ptr(res), res.stride(0) if res is not None else 0,
           x.data_ptr(), x.stride(0), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), dx.data_ptr(), dx.ld, dxb.data_ptr(), dxb.ld,
           dgamma.data_ptr(), M, N, K, H.stream_ptr())


def outputs(M):
    return U.guarded_out(M, N, N + 8, torch.float32, device="cuda"), U.guarded_out(M, N, N + 8, BF, device="cuda"), guarded_dgamma()


def check(H, M, K, with_res=True, in_place=False):
    A, B, x, res, gamma, mean, rstd = case(M, K)
    if not with_res:
        res = None
    dy, dx_ref, dxb_ref, dg_ref = pair(H, A, B, x, res, gamma, mean, rstd, M, K)
    dx, dxb, dgamma = outputs(M)
    r = res
    if in_place:          # dx is the residual: read and written by the same wavefront, row by row
        dx.t.copy_(res)
        r = dx.t
    with H.knobs(**{f"k{H.KNOB_ROWS_HEIGHT}": 2}):          # the 160-row kernel whatever the height rule says; reset on exit
        fused(H, TALL, A, B, x, r, gamma, mean, rstd, M, K, dx, dxb, dgamma)
        torch.cuda.synchronize()
    assert torch.isfinite(dx_ref).all() and torch.isfinite(dg_ref).all()          # no NaN of a frame was read by the pair
    ndx, nb = int((bits(dx.t) != bits(dx_ref)).sum()), int((bits(dxb.t) != bits(dxb_ref)).sum())
    ref64 = dgamma64(dy, x, mean, rstd)
    e_f, e_p = rel(dgamma[:N], ref64), rel(dg_ref, ref64)
    print(f"rows160 lnbwd M={M} K={K} res={with_res} in_place={in_place}: dx differs at {ndx}, dx_bf16 at {nb} elements; "
          f"dgamma rel to fp64: fused {e_f:.2e}, pair {e_p:.2e}")
    assert ndx == 0, f"dx differs at {ndx} of {M * N} elements"
    assert nb == 0, f"dx_bf16 differs at {nb} of {M * N} elements"
    assert e_f < DGAMMA_REL, e_f
    U.assert_guard_intact(dx, "dx")
    U.assert_guard_intact(dxb, "dx_bf16")
    assert bool((dgamma[N:] == 7.0).all()), "dgamma: stored past column 512"


@pytest.mark.parametrize("K", [96, 128, 1408])
@pytest.mark.parametrize("M", [5, 160, 161, 197, 321])
def test_tall_equals_the_pair(H, M, K):
    check(H, M, K)


@pytest.mark.parametrize("M,K", [(197, 128), (321, 1408)])
def test_tall_in_place(H, M, K):
    check(H, M, K, in_place=True)


@pytest.mark.parametrize("M,K", [(197, 96), (321, 1024)])
def test_tall_without_residual(H, M, K):
    check(H, M, K, with_res=False)


def test_unforced_small_m_takes_the_128_row_kernel(H):
    """knob at 0, M = 321: three tiles in either height, one round of them, so the shorter tile costs less and the entry point
    launches gemm_nt_rows_kernel with mca_gemm_nt_res_lnbwd's plan: dx and its copy are equal bits; dgamma is three workgroups'
    atomic adds in either call, so the two agree to twice the bound either is held to against the exact sum"""
    M, K = 321, 1408
    A, B, x, res, gamma, mean, rstd = case(M, K)
    p = H.GemmPlan()
    assert H.lib().mca_dbg_plan_gemm_nt(H.PLAN_RES_LNBWD_TALL, C.byref(H.NtProblem(M=M, N=N, K=K)), 0, C.byref(p)) == 0
    assert p.kernel == H.GK_NT_ROWS_LNBWD and p.nwg == 3
    got = {}
    for entry in ("mca_gemm_nt_res_lnbwd", TALL):
        dx, dxb, dgamma = outputs(M)
        fused(H, entry, A, B, x, res, gamma, mean, rstd, M, K, dx, dxb, dgamma)
        torch.cuda.synchronize()
        U.assert_guard_intact(dx, "dx")
        U.assert_guard_intact(dxb, "dx_bf16")
        got[entry] = (dx.t.clone(), dxb.t.clone(), dgamma.clone())
    a, b = got["mca_gemm_nt_res_lnbwd"], got[TALL]
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
    assert bool((b[2][N:] == 7.0).all()) and rel(b[2][:N], a[2][:N]) < 2 * DGAMMA_REL
