"""The tall form of the full-row GEMM (include/mca_hip.h: mca_gemm_nt_res_lnbwd_tall) without a GPU: the height rule of
csrc/gemm_plan.h (rounds x rows per tile, ties to 128) through plan entry 7 of mca_dbg_plan_gemm_nt, the plan in either height, the
knob that forces a height, and that entry point and plan refuse exactly what mca_gemm_nt_res_lnbwd and entry 6 refuse
(tests/test_gemm_rows_cpu.py), before anything is launched."""
import ctypes as C
import importlib

import pytest

LDS_160 = 3 * (160 + 512) * 32 * 2          # three stages of (A image [160][32], B image [512][32]) bf16
NAME_160 = b"gemm_nt_rows160_kernel"
# (workload, M, height at 256 CUs)
TABLE = [("CMU b=32", 81216, 160), ("CMU b=16", 40608, 160), ("CMU b=8", 20304, 128), ("CMU b=24", 60912, 128), ("CMU b=64", 162432, 128),
         ("LONG b=128", 779264, 128), ("CMU b=2", 5076, 128)]


@pytest.fixture(scope="module")
def H():
    importlib.import_module("mca-paper_amd.build").build()
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def plan(H, M, N=512, K=1536, cus=256, entry=None, height=0):
    p = H.GemmPlan()
    with H.knobs(**{f"k{H.KNOB_ROWS_HEIGHT}": height}):
        rc = H.lib().mca_dbg_plan_gemm_nt(H.PLAN_RES_LNBWD_TALL if entry is None else entry, C.byref(H.NtProblem(M=M, N=N, K=K)), cus, C.byref(p))
    return rc, p


def fields(p):
    return {f: getattr(p, f) for f, _ in p._fields_}


def model_height(M, cus):
    """the stated model: the height h that minimises ceil(ceil(M / h) / cus) * h, ties to 128"""
    cost = lambda h: -(-(-(-M // h)) // cus) * h
    return 160 if cost(160) < cost(128) else 128


def check_plan(H, M, K, cus, height, forced=0):
    rc, p = plan(H, M, K=K, cus=cus, height=forced)
    assert rc == 0
    if height == 128:          # every field is entry 6's
        rc6, p6 = plan(H, M, K=K, cus=cus, entry=H.PLAN_RES_LNBWD)
        assert rc6 == 0 and fields(p) == fields(p6) and p.kernel == H.GK_NT_ROWS_LNBWD, (M, cus, fields(p))
    else:
        tiles = (M + 159) // 160
        assert p.kernel == H.GK_NT_ROWS160_LNBWD == 160 and H.lib().mca_dbg_gemm_kernel_name(p.kernel) == NAME_160
        assert (p.grid_x, p.grid_y, p.block, p.lds_bytes, p.nwg) == (tiles, 1, 512, LDS_160, tiles), (M, cus, fields(p))
        assert (p.n, p.tiles_n) == (512, 1)


@pytest.mark.parametrize("name,M,height", TABLE, ids=[t[0] for t in TABLE])
def test_height_table_at_256_cus(H, name, M, height):
    assert model_height(M, 256) == height
    for K in (1024, 1536, 2816):
        check_plan(H, M, K, 256, height)


def test_the_flagship_runs_two_rounds(H):
    p = plan(H, 81216)[1]
    assert p.nwg == 508 and -(-p.nwg // 256) == 2 and -(-635 // 256) == 3
    p = plan(H, 40608)[1]
    assert p.nwg == 254 and plan(H, 40608, entry=H.PLAN_RES_LNBWD)[1].nwg == 318
    assert LDS_160 == 129024 <= 160 * 1024 and 32 * (512 + 4) * 4 <= LDS_160 and 8 * 512 * 4 <= LDS_160          # the epilogue's two uses of the ring fit


@pytest.mark.parametrize("cus", [64, 304])
def test_other_cu_counts_follow_the_model(H, cus):
    seen = set()
    for M in [1, 5, 127, 128, 129, 160, 161, 5076, 20304, 40608, 60912, 81216, 162432, 779264] + [cus * h * r + d for h in (128, 160) for r in (1, 2, 3, 7)
                                                                                                      for d in (-1, 0, 1)]:
        h = model_height(M, cus)
        seen.add(h)
        check_plan(H, M, 1536, cus, h)
    assert seen == {128, 160}
    # a tie: cus * 640 rows are 5 rounds of 128 and 4 rounds of 160
    assert model_height(cus * 640, cus) == 128 and plan(H, cus * 640, cus=cus)[1].kernel == H.GK_NT_ROWS_LNBWD


def test_the_knob_forces_the_height(H):
    for M in (5, 321, 5076, 20304, 81216):
        for cus in (64, 256):
            check_plan(H, M, 1536, cus, 128, forced=1)
            check_plan(H, M, 1536, cus, 160, forced=2)
    # entry 6 (mca_gemm_nt_res_lnbwd) does not read it
    base = fields(plan(H, 81216, entry=H.PLAN_RES_LNBWD)[1])
    assert fields(plan(H, 81216, entry=H.PLAN_RES_LNBWD, height=2)[1]) == base and base["kernel"] == 128
    assert plan(H, 81216)[1].kernel == 160          # ... and the knob is back at 0 behind every query


def test_plan_refusals_are_entry_6s(H):
    shapes = [(4096, 384, 512), (4096, 640, 512), (4096, 1024, 512), (4096, 512, 112), (4096, 512, 1400), (4096, 512, 32), (4096, 512, 64),
              (4096, 512, 96), ((1 << 30) + 1, 512, 512), (0, 512, 512), (4096, 0, 512), (4096, 512, 0)]
    want = [-3, -3, -3, -2, -2, -3, -3, 0, -3, -1, -1, -1]
    for height in (0, 1, 2):
        got7 = [plan(H, M, N, K, height=height)[0] for M, N, K in shapes]
        got6 = [plan(H, M, N, K, entry=H.PLAN_RES_LNBWD)[0] for M, N, K in shapes]
        assert got7 == got6 == want, (height, got7, got6)


def test_entry_point_refuses_what_the_128_row_one_refuses(H):
    old, new = H.lib().mca_gemm_nt_res_lnbwd, H.lib().mca_gemm_nt_res_lnbwd_tall
    b = 1 << 20          # a stand-in aligned address: every call below is refused before anything is launched

    def call(f, A=b, lda=512, B=b, ldb=512, res=b, ldres=512, x=b, ldx=512, mean=b, rstd=b, gamma=b, dx=b, lddx=512, dxb=b, ldb16=512, dgamma=b,
             M=300, N=512, K=512):
        return f(A, lda, B, ldb, res, ldres, x, ldx, mean, rstd, gamma, dx, lddx, dxb, ldb16, dgamma, M, N, K, None)

    cases = [({null: None}, -1) for null in ("A", "B", "x", "mean", "rstd", "gamma", "dx", "dxb", "dgamma")]
    cases += [(dict(M=0), -1), (dict(K=0), -1), (dict(N=384), -3), (dict(N=1024), -3), (dict(K=80), -2), (dict(K=64), -3),
              (dict(lda=1408, ldb=1408, K=1400), -2), (dict(M=(1 << 30) + 1), -3)]
    cases += [({arg: b + 8}, -2) for arg in ("A", "B", "res", "x", "gamma", "dx", "dxb")]          # a misaligned base
    cases += [({ld: 516}, -2) for ld in ("lda", "ldb", "ldb16")] + [({ld: 514}, -2) for ld in ("ldres", "ldx", "lddx")]
    cases += [({ld: 504}, -1) for ld in ("lda", "ldb", "ldb16")] + [({ld: 508}, -1) for ld in ("ldres", "ldx", "lddx")]
    # the order of the checks: a NULL operand before the shape, the shape before an alignment, an alignment before a short stride
    cases += [(dict(A=None, N=384), -1), (dict(N=384, A=b + 8), -3), (dict(K=80, N=384), -3), (dict(A=b + 8, lda=504), -2)]
    for height in (0, 1, 2):
        with H.knobs(**{f"k{H.KNOB_ROWS_HEIGHT}": height}):
            for kw, want in cases:
                assert call(new, **kw) == call(old, **kw) == want, (height, kw)


def test_kernel_names(H):
    name = H.lib().mca_dbg_gemm_kernel_name
    assert name(160) == NAME_160 and name(159) == b"?" and name(161) == b"?"
    names = [name(k) for k in range(1, 31)]
    assert len(set(names)) == 30 and b"?" not in names and NAME_160 not in names
    assert name(128) == b"gemm_nt_rows_kernel" and name(31) == b"?" and name(129) == b"?"
    assert all(name(k) == b"?" for k in range(96, 128))
