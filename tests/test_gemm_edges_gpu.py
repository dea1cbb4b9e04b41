"""Every GEMM form element by element at its tails, strides and guards (tests/gemm_edge_util.py: operands whose products are
exact inside NaN, outputs inside a sentinel).  fp32 outputs must equal the float64 reference bit for bit, bf16 outputs that
reference rounded once to nearest-even; the GEGLU and LayerNorm fusions keep their GEMM part exact and meet a derived bound at
every element (docs/parity.md, "GEMM edges").  Which kernel and which property each case reaches is asserted without a GPU in
tests/test_gemm_plan_cpu.py.  Only valid calls are made: the guard bands exist so that a stray store lands in memory the test owns."""
import ctypes as C
import importlib

import pytest
import torch

import gemm_edge_util as U
import gemm_shapes as GS

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def check(out, ref, what):
    """values first, then the guards"""
    torch.cuda.synchronize()
    U.assert_exact(out.t, ref, what)
    U.assert_guard_intact(out, what)


# ------------------------------------------------------------------------------------------------ mca_gemm_nt
@pytest.mark.parametrize("case", GS.EDGE_NT, ids=[c["name"] for c in GS.EDGE_NT])
def test_gemm_nt_edges(H, case):
    M, N, K = case["M"], case["N"], case["K"]
    g = gen(1)
    A, B = U.int_bf16(M, K, case["lda"], g), U.int_bf16(N, K, case["ldb"], g)
    bias = U.int_f32(1, N, N, g, byte_off=case["bias_off"])
    res = U.int_f32(M, N, case["ldres"], g, byte_off=case["res_off"])
    res16 = U.int_f32(16, N, case["ldres"], g, byte_off=case["res_off"])
    acc = U.matmul64(A, B)
    assert float(acc.abs().max()) <= 4 * K
    for ob, rs, bi in case["forms"]:
        dtype = BF if ob else F32
        out = U.guarded_out(M, N, case["ldc"], dtype, byte_off=case["c_off"] * (2 if ob else 4), device="cuda")
        r = res if rs == 1 else (res16 if rs == 2 else None)
        H.call("mca_gemm_nt", A.data_ptr(), case["lda"], B.data_ptr(), case["ldb"], out.data_ptr(), case["ldc"], ob, bias.data_ptr() if bi else None,
               H.ptr(r), case["ldres"] if rs else 0, 16 if rs == 2 else 0, M, N, K, H.stream_ptr())
        ref = acc.clone()
        if bi:
            ref += bias.double()
        if rs == 1:
            ref += res.double()
        if rs == 2:
            ref += res16.double().repeat(M // 16, 1)
        check(out, ref.to(dtype), f"{case['name']} (out_bf16, res, bias) = {(ob, rs, bi)}")


# ------------------------------------------------------------------------------------------------ mca_gemm_nt_lnres
@pytest.mark.parametrize("M,N,K,ldc,ldx", GS.EDGE_NT_LNRES)
def test_gemm_nt_lnres_edges(H, M, N, K, ldc, ldx):
    """mean and rstd come from float64, rounded to fp32, and go to the kernel and to the reference alike: this kernel alone is
    under test.  |C - ref| <= 2^-20 (|acc| + (|x| + |mean|) rstd |gamma|) at every element."""
    g = gen(11)
    A, B = U.int_bf16(M, K, K + 8, g), U.int_bf16(N, K, K, g)
    x = U.framed_copy(torch.randn(M, N, device="cuda", generator=g) * 3 + 0.5, ldx)
    gamma = torch.randn(N, device="cuda", generator=g)
    mean, rstd = U.ln_stats32(x)
    out = U.guarded_out(M, N, ldc, F32, device="cuda")
    H.call("mca_gemm_nt_lnres", A.data_ptr(), K + 8, B.data_ptr(), K, out.data_ptr(), ldc, x.data_ptr(), ldx, mean.data_ptr(), rstd.data_ptr(),
           gamma.data_ptr(), M, N, K, H.stream_ptr())
    torch.cuda.synchronize()
    ref, tol = U.lnres_ref(U.matmul64(A, B), x, mean, rstd, gamma)
    U.assert_close_elementwise(out.t, ref, tol, "lnres")
    U.assert_guard_intact(out, "lnres")


# ------------------------------------------------------------------------------------------------ fused GEGLU
@pytest.mark.parametrize("rows,ip,D", GS.EDGE_GEGLU_FWD)
def test_gemm_geglu_fwd_edges(H, rows, ip, D):
    """h bit-exact (W1 = integers / 16: exact in bf16 and in the fp32 sums); g against a * gelu64(gate) of the CHECKED h within
    2^-8 |ref| + 1e-6 |a gate| at every element"""
    plan = H.GemmPlan()
    assert H.lib().mca_dbg_plan_gemm_nt(H.PLAN_GEGLU_FWD, C.byref(H.NtProblem(M=rows, N=ip, K=D)), 0, C.byref(plan)) == 0
    fusedk = plan.kernel != 0          # 0: the plain GEMM over both halves + mca_geglu_fwd
    assert fusedk == (ip != 72)
    ldh, ldg = (2 * ip + 8, ip + 8) if fusedk else (2 * ip, ip)
    gn = gen(43)
    x, w1 = U.int_bf16(rows, D, D + 8, gn), U.int_bf16(2 * ip, D, D + 16, gn, scale=2.0 ** -4)
    h, gout = U.guarded_out(rows, 2 * ip, ldh, BF, device="cuda"), U.guarded_out(rows, ip, ldg, BF, device="cuda")
    args = lambda lh, lg: (x.data_ptr(), D + 8, w1.data_ptr(), D + 16, h.data_ptr(), lh, gout.data_ptr(), lg, ip, rows, D, H.stream_ptr())
    if not fusedk:          # the unfused pair takes packed rows only and says so: nothing launched
        assert H.lib().mca_gemm_nt_geglu_fwd(*args(2 * ip + 8, ip + 8)) == -3
        torch.cuda.synchronize()
        assert torch.isnan(h.t).all() and torch.isnan(gout.t).all()
    H.call("mca_gemm_nt_geglu_fwd", *args(ldh, ldg))
    check(h, U.matmul64(x, w1).to(BF), "h")
    ref, tol = U.geglu_fwd_ref(h.t, ip)
    U.assert_close_elementwise(gout.t, ref, tol, "g")
    U.assert_guard_intact(gout, "g")


@pytest.mark.parametrize("rows,ip,D", GS.EDGE_GEGLU_BWD)
def test_gemm_geglu_bwd_edges(H, rows, ip, D):
    """dg = dx . w2T^T exact (w2T = integers / 16), h any bf16: dh_a within 2^-8 |ref| + 1e-6 |dg gate| of dg gelu64(gate),
    dh_gate within 2^-8 |ref| + 1e-6 |dg a| of dg a gelu64'(gate), at every element"""
    ldh = 2 * ip + 8
    gn = gen(41)
    h = U.framed_copy(torch.randn(rows, 2 * ip, device="cuda", generator=gn).to(BF), ldh)
    dx, w2T = U.int_bf16(rows, D, D, gn), U.int_bf16(ip, D, D + 8, gn, scale=2.0 ** -4)
    dh = U.guarded_out(rows, 2 * ip, ldh, BF, device="cuda")
    H.call("mca_gemm_nt_geglu_bwd", dx.data_ptr(), D, w2T.data_ptr(), D + 8, h.data_ptr(), dh.data_ptr(), ldh, ip, rows, D, H.stream_ptr())
    torch.cuda.synchronize()
    ref, tol = U.geglu_bwd_ref(U.matmul64(dx, w2T), h, ip)
    U.assert_close_elementwise(dh.t, ref, tol, "dh")
    U.assert_guard_intact(dh, "dh")


# ------------------------------------------------------------------------------------------------ weight gradients
def tn_member(R, N, K, lda, ldb, g):
    """operands poisoned from column N (K) on, C = random integers with ldc = K + 4 in its guard, the exact result"""
    A, B = U.int_bf16(R, N, lda, g), U.int_bf16(R, K, ldb, g)
    Cg = U.guarded_out(N, K, K + 4, F32, device="cuda")
    Cg.t.copy_(U.int_f32(N, K, K, g))
    ref = (Cg.t.double() + A.double().t() @ B.double())
    assert float(ref.abs().max()) <= 4 * R + 8
    return A, B, Cg, ref.float()


@pytest.mark.parametrize("R,N,K,lda,ldb", GS.EDGE_TN)
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
def test_gemm_tn_acc_edges(H, R, N, K, lda, ldb, det):
    A, B, Cg, ref = tn_member(R, N, K, lda, ldb, gen(2))
    if det:
        need = H.lib().mca_gemm_tn_acc_det_scratch(R, N, K)
        scratch = U.guarded_out(1, max(need, 4), max(need, 4), F32, device="cuda")
        H.call("mca_gemm_tn_acc_det", A.data_ptr(), lda, B.data_ptr(), ldb, Cg.data_ptr(), K + 4, R, N, K, scratch.data_ptr(), need, H.stream_ptr())
    else:
        H.call("mca_gemm_tn_acc", A.data_ptr(), lda, B.data_ptr(), ldb, Cg.data_ptr(), K + 4, R, N, K, H.stream_ptr())
    check(Cg, ref, "C")
    if det:
        U.assert_guard_intact(scratch, "scratch")


def group_descs(H, R, members, g):
    arr = (H.TnDesc * len(members))()
    keep = []
    for d, (N, K, lda, ldb) in zip(arr, members):
        A, B, Cg, ref = tn_member(R, N, K, lda, ldb, g)
        d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.N, d.K = A.data_ptr(), lda, B.data_ptr(), ldb, Cg.data_ptr(), K + 4, N, K
        keep.append((A, B, Cg, ref))
    return arr, keep


@pytest.mark.parametrize("R,members", GS.EDGE_TN_GROUP)
def test_gemm_tn_acc_group_edges(H, R, members):
    for knob3 in (0, GS.TN_GROUP_UNIFORM_SPLITS):          # the tile-major line of spans, then uniform splits
        arr, keep = group_descs(H, R, members, gen(12))
        H.lib().mca_debug_set(3, knob3)
        try:
            H.call("mca_gemm_tn_acc_group", C.byref(arr), len(members), R, H.stream_ptr())
            torch.cuda.synchronize()
        finally:
            H.lib().mca_debug_set(3, 0)
        for i, (_, _, Cg, ref) in enumerate(keep):
            check(Cg, ref, f"member {i}, knob 3 = {knob3}")


@pytest.mark.parametrize("R,members", GS.EDGE_TN_GROUP)
def test_gemm_tn_acc_group_det_edges(H, R, members):
    n = len(members)
    Ns, Ks = (C.c_int64 * n)(*[m[0] for m in members]), (C.c_int64 * n)(*[m[1] for m in members])
    need = H.lib().mca_gemm_tn_acc_group_det_scratch(Ns, Ks, n, R, 0)
    assert need > 0
    scratch = U.guarded_out(1, need, need, F32, device="cuda")
    arr, keep = group_descs(H, R, members, gen(12))
    H.call("mca_gemm_tn_acc_group_det", C.byref(arr), n, R, scratch.data_ptr(), need, H.stream_ptr())
    for i, (_, _, Cg, ref) in enumerate(keep):
        check(Cg, ref, f"member {i}")
    U.assert_guard_intact(scratch, "scratch")
