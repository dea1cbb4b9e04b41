"""The full-row GEMM form (include/mca_hip.h: mca_gemm_nt_res_lnbwd) without a GPU: its plan (csrc/gemm_plan.h through
mca_dbg_plan_gemm_nt), what the entry point refuses before anything is launched, and that it stands outside the counted kernel
table (tests/test_gemm_plan_cpu.py holds the table itself and every existing plan to tests/golden/gemm_dispatch.json)."""
import ctypes as C
import importlib

import pytest

LDS_BYTES = 3 * (128 + 512) * 32 * 2          # three stages of (A image [128][32], B image [512][32]) bf16
MIN_K = 96                                     # the prologue fills the three stages


@pytest.fixture(scope="module")
def H():
    importlib.import_module("mca-paper_amd.build").build()
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def plan(H, M, N, K, cus=256, knobs=None):
    p = H.GemmPlan()
    with H.knobs(**{f"k{k}": v for k, v in (knobs or {}).items()}):
        rc = H.lib().mca_dbg_plan_gemm_nt(H.PLAN_RES_LNBWD, C.byref(H.NtProblem(M=M, N=N, K=K)), cus, C.byref(p))
    return rc, p


@pytest.mark.parametrize("M,K", [(1, 96), (5, 96), (128, 128), (129, 1408), (165, 2816), (257, 1536), (5076, 1024), (81216, 2816)])
def test_plan_is_one_workgroup_per_128_rows(H, M, K):
    rc, p = plan(H, M, 512, K)
    assert rc == 0
    assert p.kernel == H.GK_NT_ROWS_LNBWD and H.lib().mca_dbg_gemm_kernel_name(p.kernel) == b"gemm_nt_rows_kernel"
    tiles = (M + 127) // 128
    assert (p.grid_x, p.grid_y, p.block, p.lds_bytes) == (tiles, 1, 512, LDS_BYTES)
    assert (p.n, p.tiles_n, p.nwg) == (512, 1, tiles)
    assert LDS_BYTES <= 160 * 1024 and 32 * (512 + 4) * 4 <= LDS_BYTES and 8 * 512 * 4 <= LDS_BYTES          # the epilogue's two uses of the ring fit


def test_plan_reads_neither_knobs_nor_the_cu_count(H):
    base = plan(H, 81216, 512, 2816)[1]
    for cus, knobs in ((64, None), (256, {1: 1}), (256, {7: 1}), (256, {7: 3}), (304, {0: 32, 4: 1, 10: 1})):
        p = plan(H, 81216, 512, 2816, cus, knobs)[1]
        assert all(getattr(p, f) == getattr(base, f) for f, _ in p._fields_)


def test_plan_refusals(H):
    assert plan(H, 4096, 384, 512)[0] == -3 and plan(H, 4096, 640, 512)[0] == -3 and plan(H, 4096, 1024, 512)[0] == -3          # N != 512
    assert plan(H, 4096, 512, 112)[0] == -2 and plan(H, 4096, 512, 1400)[0] == -2                                                 # K % 32
    assert plan(H, 4096, 512, 32)[0] == -3 and plan(H, 4096, 512, MIN_K - 32)[0] == -3 and plan(H, 4096, 512, MIN_K)[0] == 0
    assert plan(H, (1 << 30) + 1, 512, 512)[0] == -3 and plan(H, 0, 512, 512)[0] == -1


def test_entry_point_refusals(H):
    f = H.lib().mca_gemm_nt_res_lnbwd
    b = 1 << 20          # a stand-in aligned address: every call below is refused before anything is launched

    def call(A=b, lda=512, B=b, ldb=512, res=b, ldres=512, x=b, ldx=512, mean=b, rstd=b, gamma=b, dx=b, lddx=512, dxb=b, ldb16=512, dgamma=b,
             M=300, N=512, K=512):
        return f(A, lda, B, ldb, res, ldres, x, ldx, mean, rstd, gamma, dx, lddx, dxb, ldb16, dgamma, M, N, K, None)

    for null in ("A", "B", "x", "mean", "rstd", "gamma", "dx", "dxb", "dgamma"):
        assert call(**{null: None}) == -1, null
    assert call(M=0) == -1 and call(K=0) == -1
    assert call(N=384) == -3 and call(N=1024) == -3
    assert call(K=80) == -2 and call(K=64) == -3 and call(lda=1408, ldb=1408, K=1400) == -2
    for arg in ("A", "B", "res", "x", "gamma", "dx", "dxb"):          # a misaligned base
        assert call(**{arg: b + 8}) == -2, arg
    assert call(lda=516) == -2 and call(ldb=516) == -2 and call(ldb16=516) == -2          # bf16 strides: multiples of 8
    assert call(ldres=514) == -2 and call(ldx=514) == -2 and call(lddx=514) == -2          # fp32 strides: multiples of 4
    assert call(lda=504) == -1 and call(ldb=504) == -1 and call(ldres=508) == -1 and call(ldx=508) == -1 and call(lddx=508) == -1 \
        and call(ldb16=504) == -1
    # (a NULL residual is accepted, and so launches: tests/test_gemm_rows_gpu.py)


def test_the_counted_kernel_table_stands(H):
    name = H.lib().mca_dbg_gemm_kernel_name
    names = [name(k) for k in range(1, 31)]
    assert len(set(names)) == 30 and b"?" not in names and name(31) == b"?"
    assert name(127) == b"?" and name(128) == b"gemm_nt_rows_kernel" and name(129) == b"?"
    assert all(name(k) == b"?" for k in range(96, 128))
