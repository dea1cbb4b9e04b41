"""The saved-factor GEGLU forms without a GPU: their plans are the siblings' plans with the saved kernel (csrc/gemm_plan.h through
mca_dbg_plan_gemm_nt), and the element-wise bounds of tests/test_geglu_saved_gpu.py are satisfiable - by the exact factors
rounded once, and by gelu_pair's own arithmetic restated in fp32 - and reject a value one bf16 step off."""
import ctypes as C
import importlib

import pytest
import torch

import gemm_edge_util as U
import gemm_shapes as GS
import geglu_saved_util as S

FWD, BWD = S.FWD, S.BWD
SAVED_NAME = {"gemm_nt_persist256_kernel<true>": "gemm_nt_persist256_kernel<true,true>",
              "gemm_nt_persist_kernel<4,false>": "gemm_nt_persist_kernel<6,false>",
              "gemm_nt_persist_kernel<3,false>": "gemm_nt_persist_kernel<5,false>",
              "gemm_nt_256_kernel<true,0,0,1>": "gemm_nt_256_kernel<true,0,0,3>",
              "gemm_nt_glds_kernel<true,0,64,1>": "gemm_nt_glds_kernel<true,0,64,3>",
              "none": "none"}


@pytest.fixture(scope="module")
def H():
    importlib.import_module("mca-paper_amd.build").build()
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def plan(H, entry, M, N, K, cus=256, knobs=None):
    p = H.GemmPlan()
    with H.knobs(**{f"k{k}": v for k, v in (knobs or {}).items()}):
        assert H.lib().mca_dbg_plan_gemm_nt(entry, C.byref(H.NtProblem(M=M, N=N, K=K)), cus, C.byref(p)) == 0
    return p


def fields(p, skip=("kernel",)):
    return {f: getattr(p, f) for f, _ in p._fields_ if f not in skip}


def assert_sibling(H, entry, entry_saved, shape, cus=256, knobs=None):
    base, saved = plan(H, entry, *shape, cus, knobs), plan(H, entry_saved, *shape, cus, knobs)
    assert fields(saved) == fields(base), (shape, cus, knobs)          # grid, block, LDS bytes and every integer argument
    name = lambda p: H.lib().mca_dbg_gemm_kernel_name(p.kernel).decode()
    assert name(saved) == SAVED_NAME[name(base)], (shape, name(base), name(saved))
    assert saved.kernel == (base.kernel + H.GK_SAVED if base.kernel else 0)
    return name(base)


def test_saved_plans_are_the_siblings_plans(H):
    got = [assert_sibling(H, H.PLAN_GEGLU_FWD, H.PLAN_GEGLU_FWD_SAVED, s) for s in FWD]
    assert got == ["gemm_nt_persist256_kernel<true>", "gemm_nt_persist256_kernel<true>", "gemm_nt_persist_kernel<4,false>", "none", "none"]
    got = [assert_sibling(H, H.PLAN_GEGLU_BWD, H.PLAN_GEGLU_BWD_SAVED, s) for s in BWD]
    assert got == ["gemm_nt_persist_kernel<3,false>", "gemm_nt_256_kernel<true,0,0,1>", "gemm_nt_glds_kernel<true,0,64,1>",
                   "gemm_nt_glds_kernel<true,0,64,1>"]
    # every form the planners can choose was seen
    assert set(SAVED_NAME) - {"none"} == {H.lib().mca_dbg_gemm_kernel_name(k).decode() for k in (7, 16, 23, 24, 26)}


@pytest.mark.parametrize("cus", [256, 64])
def test_saved_plans_over_the_suite_and_edge_shapes(H, cus):
    step = [(T, GS.IP, GS.D) for T in GS.STEP_ROWS.values()]
    for s in GS.GEGLU_FWD + GS.EDGE_GEGLU_FWD + step:
        assert_sibling(H, H.PLAN_GEGLU_FWD, H.PLAN_GEGLU_FWD_SAVED, s, cus)
    for s in GS.GEGLU_BWD + GS.EDGE_GEGLU_BWD + step:
        assert_sibling(H, H.PLAN_GEGLU_BWD, H.PLAN_GEGLU_BWD_SAVED, s, cus)
    # ... and under the knobs that move these two planners
    for knobs in ({1: 1}, {7: 1}, {10: 1}, {0: 32}):
        for s in GS.GEGLU_FWD:
            assert_sibling(H, H.PLAN_GEGLU_FWD, H.PLAN_GEGLU_FWD_SAVED, s, cus, knobs)
        for s in GS.GEGLU_BWD:
            assert_sibling(H, H.PLAN_GEGLU_BWD, H.PLAN_GEGLU_BWD_SAVED, s, cus, knobs)


def test_base_kernel_table_is_unchanged(H):
    name = H.lib().mca_dbg_gemm_kernel_name
    assert name(31) == b"?" and name(63) == b"?" and name(64) == b"?" and name(64 + 25) == b"?"          # only the five GEGLU forms have a saved sibling
    assert len({name(64 + k) for k in (7, 16, 23, 24, 26)} - {b"?"}) == 5


def test_saved_entry_points_validate_like_their_siblings(H):
    L = H.lib()
    b = 1 << 20          # a stand-in aligned address: every call below is refused before anything is launched
    assert L.mca_gemm_nt_geglu_fwd_saved(b, 64, b, 64, None, 16, b, 8, 8, 4, 64, None) == -1
    assert L.mca_gemm_nt_geglu_fwd_saved(b, 64, b, 64, b, 20, b, 8, 8, 4, 64, None) == -2          # lds % 8
    assert L.mca_gemm_nt_geglu_bwd_saved(b, 64, b, 64, None, b, 16, 8, 4, 64, None) == -1
    assert L.mca_gemm_nt_geglu_bwd_saved(b, 64, b, 64, b, b, 8, 8, 4, 64, None) == -1              # ldh < 2 ip
    assert L.mca_geglu_fwd_saved(b, b, 4, 12, None) == -1 and L.mca_geglu_bwd_saved(b, b, b, 4, 12, None) == -1
    assert L.mca_geglu_fwd_saved(b, b, 0, 8, None) == 0 and L.mca_geglu_bwd_saved(b, b, b, 0, 8, None) == 0


# ---- the bounds
def gen(seed):
    return torch.Generator().manual_seed(seed)


def gelu_pair32(x):
    """csrc/common.h gelu_pair restated in fp32 torch operations (Abramowitz-Stegun 7.1.26)"""
    x = x.float()
    z = x.abs() * 0.70710678118654752
    t = 1.0 / (0.3275911 * z + 1.0)
    e = torch.exp2(x * x * -0.72134752044448170)
    p = t * 1.061405429 - 1.453152027
    p = t * p + 1.421413741
    p = t * p - 0.284496736
    p = t * p + 0.254829592
    erf_abs = 1.0 - p * t * e
    cdf = torch.copysign(erf_abs, x) * 0.5 + 0.5
    return x * cdf, x * 0.3989422804014327 * e + cdf


def checked_h(seed, rows=300, ip=128, D=320):
    """h as the forward tests make it: exact sums of integers / 16, rounded once; gates spread over about +-8"""
    g = gen(seed)
    x, w1 = U.int_bf16(rows, D, D, g), U.int_bf16(2 * ip, D, D, g, scale=2.0 ** -4)
    h = U.matmul64(x, w1).to(torch.bfloat16)
    assert 1.5 < float(h[:, ip:].float().std()) < 2.4 and float(h.float().abs().max()) > 6
    return h, ip


def test_half_step_is_the_bf16_half_step():
    x = torch.tensor([1.0, 1.5, 1.9999, 2.0, 0.75, 3e-5, 100.0, 0.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -24, 2.0 ** -2, 0.0], dtype=torch.float64)
    assert torch.equal(S.half_step_bf16(x), want)
    v = torch.rand(4096, generator=gen(1), dtype=torch.float64) * 16 - 8
    assert ((v.to(torch.bfloat16).double() - v).abs() <= S.half_step_bf16(v)).all()


def test_saved_factor_bound_is_satisfiable_by_the_exact_factors_rounded_once():
    h, ip = checked_h(5)
    ref, tol = S.saved_ref(h, ip)
    U.assert_close_elementwise(ref.to(torch.bfloat16), ref, tol)
    # the rounding alone uses the bound up: the largest |rounded - ref| / bound is close to 1, so nothing else has much room
    ratio = ((ref.to(torch.bfloat16).double() - ref).abs() / tol.clamp_min(1e-300)).max()
    assert 0.98 < float(ratio) <= 1.0, float(ratio)


def test_saved_factor_bound_is_satisfiable_by_fp32_gelu_pair():
    h, ip = checked_h(6)
    a, gate = h[:, :ip].float(), h[:, ip:].float()
    ge, dge = gelu_pair32(gate)
    got = torch.cat([ge.to(torch.bfloat16), (a * dge).to(torch.bfloat16)], 1)
    ref, tol = S.saved_ref(h, ip)
    U.assert_close_elementwise(got, ref, tol)
    # zero halves give zero factors (the padded columns ip > I of the step)
    z = torch.zeros(4, 16, dtype=torch.bfloat16)
    ge0, dge0 = gelu_pair32(z[:, 8:])
    assert (S.factors64(z, 8) == 0).all() and (ge0 == 0).all() and (z[:, :8].float() * dge0 == 0).all()


def test_saved_factor_bound_rejects_one_bf16_step():
    h, ip = checked_h(7)
    ref, tol = S.saved_ref(h, ip)
    got = ref.to(torch.bfloat16)
    i, j = [int(v) for v in (ref.abs() > 0.5).nonzero()[0]]
    got.view(torch.int16)[i, j] += 1
    with pytest.raises(AssertionError, match=rf"1 of {ref.numel()} elements wrong.*\({i}, {j},"):
        U.assert_close_elementwise(got, ref, tol)


def test_saved_backward_is_exact_and_within_the_bound_of_the_unsaved_form():
    """dg exact (w2T = integers / 16) and s bf16: the fp32 product dg * s is exact, so dh = bf16(dg * s) has ONE correct value;
    against the unsaved form's arithmetic on the matching h it stays within 2^-7 |dh| + the unsaved bound's absolute floor"""
    g = gen(8)
    rows, ip, D = 300, 72, 512
    h = torch.randn(rows, 2 * ip, generator=g).to(torch.bfloat16)
    dx, w2T = U.int_bf16(rows, D, D, g), U.int_bf16(ip, D, D, g, scale=2.0 ** -4)
    dg = U.matmul64(dx, w2T)
    s = S.factors64(h, ip).to(torch.bfloat16)
    prod = torch.cat([dg, dg], 1) * s.double()
    assert (prod.float().double() == prod).all()          # 12 + 8 significant bits: exact in fp32
    dh_saved = prod.to(torch.bfloat16)
    a, gate = h[:, :ip].float(), h[:, ip:].float()
    ge, dge = gelu_pair32(gate)
    dh_unsaved = torch.cat([(dg.float() * ge).to(torch.bfloat16), (dg.float() * a * dge).to(torch.bfloat16)], 1)
    U.assert_close_elementwise(dh_saved, dh_unsaved.double(), S.bwd_vs_unsaved_tol(dh_unsaved, dg, h, ip))
