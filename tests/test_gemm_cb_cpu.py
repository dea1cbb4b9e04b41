"""The planner of the column-blocked GEMM store (mca_gemm_nt_cb, csrc/gemm_plan.h mca_plan_gemm_nt_cb) as checked facts, without
a GPU: it takes exactly the shapes of the 256 x 256 persistent kernel, with that kernel's grid, block and LDS bytes, refuses
everything else - the knobs that keep mca_gemm_nt off that kernel included - and its kernel value stands outside the counted table."""
import ctypes as C
import importlib

import pytest

BASE = 0x10000000          # a 256-byte aligned stand-in address: the planner reads alignment only
CUS = 256


@pytest.fixture(scope="module")
def H():
    importlib.import_module("mca-paper_amd.build").build()
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def plan_cb(H, M, N, K, c=BASE, cbs=None, cus=CUS):
    p = H.GemmPlan()
    rc = H.lib().mca_dbg_plan_gemm_nt_cb(M, N, K, c, M * 64 if cbs is None else cbs, cus, C.byref(p))
    return rc, p


def plan_plain(H, M, N, K, cus=CUS):
    pr = H.NtProblem(M=M, N=N, K=K, out_bf16=1, C=BASE, ldc=N)
    p = H.GemmPlan()
    assert H.lib().mca_dbg_plan_gemm_nt(H.PLAN_NT, C.byref(pr), cus, C.byref(p)) == 0
    return p


FIELDS = ("grid_x", "grid_y", "block", "lds_bytes", "n", "tiles_n", "nwg", "dbg")


@pytest.mark.parametrize("M,N,K", [(2048, 256, 192), (2085, 512, 512), (2085, 1536, 192), (11520, 1536, 192), (81216, 1536, 512),
                                   (81216, 512, 512), (20304, 512, 224)])
@pytest.mark.parametrize("cus", [256, 64])
def test_cb_plan_is_the_persist256_plan_with_the_blocked_kernel(H, M, N, K, cus):
    rc, p = plan_cb(H, M, N, K, cus=cus)
    assert rc == 0
    q = plan_plain(H, M, N, K, cus)
    assert H.lib().mca_dbg_gemm_kernel_name(q.kernel) == b"gemm_nt_persist256_kernel<false>"
    assert p.kernel == H.GK_NT_PERSIST256_CB == 256
    assert H.lib().mca_dbg_gemm_kernel_name(p.kernel) == b"gemm_nt_persist256_kernel<false,false,true>"
    assert [getattr(p, f) for f in FIELDS] == [getattr(q, f) for f in FIELDS]
    assert p.block == 512 and p.grid_x == min(p.nwg, cus) and p.nwg == (M + 255) // 256 * (N // 256)
    # slabs further apart than their rows (a framed buffer) are taken too
    assert plan_cb(H, M, N, K, cbs=(M + 5) * 64, cus=cus)[0] == 0


@pytest.mark.parametrize("what,M,N,K,kw", [
    ("M < 2048", 2047, 512, 512, {}), ("N % 256", 4096, 384, 512, {}), ("N % 256 (64)", 4096, 576, 512, {}),
    ("K < 192", 4096, 512, 128, {}), ("K % 32", 4096, 512, 208, {}),
    ("C misaligned", 4096, 512, 512, dict(c=BASE + 8)), ("cbs % 8", 4096, 512, 512, dict(cbs=4096 * 64 + 4)),
    ("cbs < M * 64", 4096, 512, 512, dict(cbs=4095 * 64))])
def test_cb_plan_refuses_what_the_kernel_is_not_built_for(H, what, M, N, K, kw):
    assert plan_cb(H, M, N, K, **kw)[0] == -3, what


@pytest.mark.parametrize("knob,value", [(1, 1), (7, 1), (7, 3), (10, 1)])
def test_cb_plan_follows_the_knobs_that_take_the_plain_call_off_the_kernel(H, knob, value):
    assert plan_cb(H, 81216, 1536, 512)[0] == 0
    with H.knobs(**{f"k{knob}": value}):
        assert plan_cb(H, 81216, 1536, 512)[0] == -3
        assert H.lib().mca_dbg_gemm_kernel_name(plan_plain(H, 81216, 1536, 512).kernel) != b"gemm_nt_persist256_kernel<false>"
    assert plan_cb(H, 81216, 1536, 512)[0] == 0


def test_cb_plan_bad_arguments(H):
    assert H.lib().mca_dbg_plan_gemm_nt_cb(4096, 512, 512, BASE, 4096 * 64, CUS, None) == -1
    assert plan_cb(H, 0, 512, 512)[0] == -1 and plan_cb(H, 4096, 0, 512)[0] == -1 and plan_cb(H, 4096, 512, 0)[0] == -1
