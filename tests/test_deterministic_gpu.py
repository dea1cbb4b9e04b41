"""Deterministic forms of the order-dependent entry points (include/mca_hip.h, "Deterministic mode"), kernel by kernel.  For every
form and shape: (1) three launches from the same inputs and the same initial destination are torch.equal; (2) the destination is
bit-equal to dst_in + (((p_0 + p_1) + p_2) + ...) recomputed on the host in sequential float32 from the partials the launch left
in its scratch, read by the slot layout the header documents - the order is fixed by construction, not by luck; (3) the value is
within the plain form's bound of an fp64 reference; (4) a scratch one float too small is refused and the destination untouched."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import gemm_shapes as GS

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bf(x):
    return x.to(torch.bfloat16)


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


def ordered_sum(dst_in, partials):
    """dst_in + (((p_0 + p_1) + p_2) + ...), every add a float32 add, slots in ascending index"""
    p = partials.astype(np.float32)
    acc = p[0].copy()
    for s in range(1, p.shape[0]):
        acc = acc + p[s]
    assert acc.dtype == np.float32
    return dst_in.astype(np.float32) + acc


def check_form(launch, need, dsts, partials_of, check_order=None):
    """launch(scratch_ptr, scratch_floats) -> rc;  dsts: the destination tensors (any initial value);
    partials_of(scratch as a host float32 array) -> one [S, ...] array per destination, in the header's slot layout"""
    assert need > 0
    init = [d.clone() for d in dsts]
    scratch = torch.empty(need, device="cuda")
    runs = []
    for _ in range(3):
        for d, i in zip(dsts, init):
            d.copy_(i)
        scratch.fill_(NAN)          # a slot element nobody stores would poison the sum
        assert launch(scratch.data_ptr(), need) == 0
        torch.cuda.synchronize()
        runs.append([d.clone() for d in dsts])
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r, runs[0]))
    host = scratch.cpu().numpy()
    for k, (d0, got, p) in enumerate(zip(init, runs[0], partials_of(host))):
        if check_order is not None and not check_order[k]:
            continue
        exp = ordered_sum(d0.cpu().numpy(), p.reshape((p.shape[0],) + tuple(d0.shape)))
        assert np.array_equal(exp.view(np.uint32), bits(got)), f"destination {k}: not the ordered fp32 sum of its {p.shape[0]} slots"
    # one float short: refused, nothing launched
    for d, i in zip(dsts, init):
        d.copy_(i)
    assert launch(scratch.data_ptr(), need - 1) == -1
    assert launch(None, need) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(d, i) for d, i in zip(dsts, init))
    return runs[0]


# ------------------------------------------------------------------------------------------------ weight gradients
def plan_single(H, R, N, K):
    p = H.TnDetPlan()
    assert H.lib().mca_dbg_plan_gemm_tn_det(R, N, K, C.byref(p)) == 0
    return p, H.lib().mca_dbg_gemm_kernel_name(p.launch.kernel).decode()


@pytest.mark.parametrize("R,N,K,lda,ldb,ldc,kernel", [
    (1000, 200, 136, 200, 136, 136, "gemm_tn_kernel"), (4160, 512, 256, 512, 264, 256, "gemm_tn_256_kernel"),
    (4160, 1024, 512, 1536, 512, 520, "gemm_tn_256x256_kernel"), (5000, 1365, 512, 2816, 512, 512, "gemm_tn_256x256_kernel")])
def test_gemm_tn_acc_det(H, R, N, K, lda, ldb, ldc, kernel):
    L = H.lib()
    plan, name = plan_single(H, R, N, K)
    assert name == kernel and plan.slots >= 2 and plan.slots == plan.launch.grid_y          # asserted, not assumed
    need = L.mca_gemm_tn_acc_det_scratch(R, N, K)
    assert need == plan.slots * N * K
    g = torch.Generator(device="cuda").manual_seed(2)
    A = bf(torch.randn(R, lda, device="cuda", generator=g))
    B = bf(torch.randn(R, ldb, device="cuda", generator=g))
    Cbuf = torch.randn(N, ldc, device="cuda", generator=g)
    Cg = Cbuf[:, :K]
    pad0 = Cbuf[:, K:].clone()
    ref = Cg.double() + A[:, :N].double().t() @ B[:, :K].double()
    launch = lambda sp, sf: L.mca_gemm_tn_acc_det(A.data_ptr(), lda, B.data_ptr(), ldb, Cg.data_ptr(), ldc, R, N, K, sp, sf, H.stream_ptr())
    (got,) = check_form(launch, need, [Cg], lambda s: [s[:need].reshape(plan.slots, N, K)])
    assert rel(got, ref) < 2e-5
    assert torch.equal(Cbuf[:, K:], pad0)          # ldc honoured: nothing written between the rows


def group_members(R, members, seed=12):
    g = torch.Generator(device="cuda").manual_seed(seed)
    keep, refs = [], []
    for N, K, lda, ldb in members:
        A = bf(torch.randn(R, lda, device="cuda", generator=g))
        B = bf(torch.randn(R, ldb, device="cuda", generator=g))
        Cg = torch.randn(N, K, device="cuda", generator=g)
        refs.append(Cg.double() + A[:, :N].double().t() @ B[:, :K].double())
        keep.append((A, B, Cg))
    return keep, refs


def group_launch(H, keep, members, R):
    arr = (H.TnDesc * len(members))()
    for d, (A, B, Cg), (N, K, lda, ldb) in zip(arr, keep, members):
        d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.N, d.K = A.data_ptr(), lda, B.data_ptr(), ldb, Cg.data_ptr(), K, N, K
    return arr, lambda sp, sf: H.lib().mca_gemm_tn_acc_group_det(C.byref(arr), len(members), R, sp, sf, H.stream_ptr())


@pytest.mark.parametrize("R,members", [GS.TN_GROUP[3], (4160, [(1024, 512, 1024, 512), (512, 1024, 512, 1024)])])
def test_gemm_tn_acc_group_det(H, R, members):
    L = H.lib()
    n = len(members)
    Ns, Ks = (C.c_int64 * n)(*[m[0] for m in members]), (C.c_int64 * n)(*[m[1] for m in members])
    plan = H.TnGroupDetPlan()
    assert L.mca_dbg_plan_gemm_tn_group_det(Ns, Ks, n, R, 0, C.byref(plan)) == 0
    assert plan.plan.grouped == 1 and L.mca_dbg_gemm_kernel_name(plan.plan.launch.kernel) == b"gemm_tn_256x256_group_kernel"
    S, stride = plan.slots, plan.slot_stride
    assert S >= 2 and S == plan.plan.part.n_full and plan.plan.launch.grid_x == S * plan.plan.part.tiles
    need = L.mca_gemm_tn_acc_group_det_scratch(Ns, Ks, n, R, 0)
    assert need == S * stride == S * sum(m[0] * m[1] for m in members)
    keep, refs = group_members(R, members)
    arr, launch = group_launch(H, keep, members, R)

    def partials(s):
        out, off = [], 0
        for N, K, _, _ in members:          # a slot: member 0's [N][K], then member 1's, ...
            out.append(np.stack([s[k * stride + off:k * stride + off + N * K] for k in range(S)]).reshape(S, N, K))
            off += N * K
        return out
    got = check_form(launch, need, [c for _, _, c in keep], partials)
    for g_, ref in zip(got, refs):
        assert rel(g_, ref) < 2e-5


def test_gemm_tn_acc_group_det_falls_back_to_single_launches(H):
    """a member the grouped kernel does not take: one deterministic launch per member, each with its own layout from scratch + 0
    (so only the LAST member's partials are still there afterwards), need = the largest member's"""
    L = H.lib()
    R, members = GS.TN_GROUP[4]
    n = len(members)
    Ns, Ks = (C.c_int64 * n)(*[m[0] for m in members]), (C.c_int64 * n)(*[m[1] for m in members])
    plan = H.TnGroupDetPlan()
    assert L.mca_dbg_plan_gemm_tn_group_det(Ns, Ks, n, R, 0, C.byref(plan)) == 0 and plan.plan.grouped == 0
    singles = [plan_single(H, R, m[0], m[1])[0] for m in members]
    assert all(p.slots >= 2 for p in singles)
    need = L.mca_gemm_tn_acc_group_det_scratch(Ns, Ks, n, R, 0)
    assert need == max(p.scratch_floats for p in singles)
    keep, refs = group_members(R, members)
    arr, launch = group_launch(H, keep, members, R)
    N, K = members[-1][0], members[-1][1]
    last = singles[-1]
    got = check_form(launch, need, [c for _, _, c in keep], lambda s: [None] * (n - 1) + [s[:last.slots * N * K].reshape(last.slots, N, K)],
                     check_order=[False] * (n - 1) + [True])
    for g_, ref in zip(got, refs):
        assert rel(g_, ref) < 2e-5


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def ln_case(rows, cols, affine, masked, period, seed=3):
    """inputs of one backward and its fp64 reference (the formulas of elementwise.hip)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    nb = rows // period if period else 0
    if period:
        rows = nb * period
    x = torch.randn(rows, cols, device="cuda", generator=g) * 2 + 0.5
    gamma = torch.randn(cols, device="cuda", generator=g)
    mask = (torch.rand(rows, device="cuda", generator=g) < 0.3) if masked else torch.zeros(rows, dtype=torch.bool, device="cuda")
    xd = x.double()
    mean, var = xd.mean(1), xd.var(1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    mean, rstd = mean.masked_fill(mask, 0.0).float(), rstd.masked_fill(mask, 0.0).float()          # a padded row's statistics are (0, 0)
    NTOT = period + 11 if period else 0
    dy_full = torch.randn(nb, NTOT, cols, device="cuda", generator=g) if period else torch.randn(rows, cols, device="cuda", generator=g)
    dy = dy_full[:, 5:5 + period].reshape(rows, cols) if period else dy_full
    dyptr = dy_full.data_ptr() + (5 * cols * 4 if period else 0)
    live = (~mask)[:, None].double()
    xh = (xd - mean.double()[:, None]) * rstd.double()[:, None] * live
    d = dy.double() * live
    gg = d * gamma.double()
    dx = rstd.double()[:, None] * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True)) * live
    ref = dict(dgamma=(d * xh).sum(0), dbeta=d.sum(0), dx=dx, dxsum=dx.sum(0))
    return dict(rows=rows, cols=cols, x=x, gamma=gamma, mean=mean, rstd=rstd, mask=mask.to(torch.uint8) if masked else None,
                dyptr=dyptr, ldy=cols, bstride=NTOT * cols, period=period, keep=dy_full, ref=ref, g=g)


def run_ln_det(H, c, want_dx, dbeta, dxsum):
    """-> the workgroup slabs of the kernel form the call takes are NOT assumed: the slot count is read off the scratch (the
    slots the launch stored are the ones no longer NaN), and the layout [slot][3][cols] is the header's"""
    L = H.lib()
    rows, cols = c["rows"], c["cols"]
    need = L.mca_layernorm_bwd_det_scratch(rows, cols)
    assert need % (3 * cols) == 0
    g = c["g"]
    dgamma = torch.randn(cols, device="cuda", generator=g)
    db = torch.randn(cols, device="cuda", generator=g) if dbeta else None
    ds = torch.randn(cols, device="cuda", generator=g) if dxsum else None
    dx = torch.empty(rows, cols, device="cuda") if want_dx else None
    dxb = torch.empty(rows, cols, device="cuda", dtype=torch.bfloat16) if want_dx else None
    launch = lambda sp, sf: L.mca_layernorm_bwd_det(
        c["dyptr"], c["ldy"], c["bstride"], c["period"], c["x"].data_ptr(), cols, c["gamma"].data_ptr(), c["mean"].data_ptr(), c["rstd"].data_ptr(),
        H.ptr(c["mask"]), H.ptr(dx), cols, H.ptr(dxb), cols, dgamma.data_ptr(), H.ptr(db), H.ptr(ds), rows, cols, sp, sf, H.stream_ptr())
    dsts = [t for t in (dgamma, db, ds) if t is not None]
    which = [k for k, t in enumerate((dgamma, db, ds)) if t is not None]
    init = [t.clone() for t in dsts]
    slots_seen = []

    def partials(s):
        v = s.reshape(-1, 3, cols)
        n = int((~np.isnan(v[:, 0, 0])).sum())          # dgamma is always asked for
        assert n >= 1 and not np.isnan(v[:n][:, which]).any() and np.isnan(v[n:]).all(), "slots 0 .. S-1 written in full, nothing else"
        slots_seen.append(n)
        return [v[:n, k] for k in which]
    got = check_form(launch, need, dsts, partials)
    ref = c["ref"]
    out = dict(zip([("dgamma", "dbeta", "dxsum")[k] for k in which], zip(got, init)))
    assert rel(out["dgamma"][0] - out["dgamma"][1], ref["dgamma"]) < 2e-5
    if dbeta:
        assert rel(out["dbeta"][0] - out["dbeta"][1], ref["dbeta"]) < 2e-5
    if dxsum:
        assert (out["dxsum"][0].double() - out["dxsum"][1].double() - ref["dxsum"]).abs().max() < 2e-4 * ref["dx"].abs().sum(0).max()
    if want_dx:
        assert rel(dx, ref["dx"]) < 2e-5 and rel(dxb.float(), ref["dx"]) < 4e-3
    return slots_seen[0]


@pytest.mark.parametrize("rows,cols,masked,period,slots", [(333, 74, True, 30, 83), (64, 713, True, 30, 15), (1000, 512, False, 0, 250),
                                                           (300, 128, True, 15, 75)])
def test_layernorm_bwd_det_general(H, rows, cols, masked, period, slots):
    """the general kernel (one row per wavefront; scalar and float4 forms), with dbeta and dxsum; the last case: dxsum and a period"""
    assert run_ln_det(H, ln_case(rows, cols, True, masked, period), True, True, True) == slots          # ceil(rows / 4) workgroups


@pytest.mark.parametrize("rows,cols,slots", [(4099, 512, 256), (8192, 256, 256), (1000, 512, 125)])
def test_layernorm_bwd_det_trunk(H, rows, cols, slots):
    """the trunk form: dgamma only, two rows per wavefront, one workgroup per CU at most.  At 1,000 rows the slot count tells the
    forms apart: 125 workgroups of eight rows here, 250 of four rows if the call took the general kernel."""
    assert run_ln_det(H, ln_case(rows, cols, False, False, 0), True, False, False) == slots


@pytest.mark.parametrize("rows,cols,slots", [(4099, 74, 129), (1000, 35, 32)])
def test_layernorm_bwd_det_params_only(H, rows, cols, slots):
    """no dx asked for: the column-parallel kernel, slot = its row slab (blockIdx.y)"""
    assert run_ln_det(H, ln_case(rows, cols, True, True, 0), False, True, False) == slots


# ------------------------------------------------------------------------------------------------ row reductions
@pytest.mark.parametrize("groups,period,cols,slabs", [(20, 15, 512, 17), (12000, 1, 512, 256)])
def test_reduce_rows_det(H, groups, period, cols, slabs):
    L = H.lib()
    rows = groups * period
    g = torch.Generator(device="cuda").manual_seed(5)
    NTOT = period + 5
    src = torch.randn(groups, NTOT, cols, device="cuda", generator=g)
    dst_buf = torch.randn(period, cols + 8, device="cuda", generator=g)
    dst = dst_buf[:, :cols]
    pad0 = dst_buf[:, cols:].clone()
    need = L.mca_reduce_rows_det_scratch(rows, period, cols)
    assert need == slabs * period * cols
    launch = lambda sp, sf: L.mca_reduce_rows_det(src.data_ptr() + 3 * cols * 4, cols, NTOT * cols, period, dst.data_ptr(), cols + 8, rows, cols,
                                                  sp, sf, H.stream_ptr())
    init = dst.clone()
    (got,) = check_form(launch, need, [dst], lambda s: [s.reshape(slabs, period, cols)])
    assert rel(got.double() - init.double(), src[:, 3:3 + period].double().sum(0)) < 1e-6
    assert torch.equal(dst_buf[:, cols:], pad0)


def test_tab_value_bwd_det(H):
    L = H.lib()
    rows, cols, max_value = 1000, 128, 1.5
    g = torch.Generator(device="cuda").manual_seed(6)
    dh1 = torch.randn(rows, cols, device="cuda", generator=g)
    h1 = bf(torch.randn(rows, cols, device="cuda", generator=g))
    x = torch.randn(rows, device="cuda", generator=g) * 2
    dw1, db1 = torch.randn(cols, device="cuda", generator=g), torch.randn(cols, device="cuda", generator=g)
    need = L.mca_tab_value_bwd_det_scratch(rows, cols)
    slabs = need // (2 * cols)
    assert slabs == 500 and need == slabs * 2 * cols
    launch = lambda sp, sf: L.mca_tab_value_bwd_det(dh1.data_ptr(), cols, h1.data_ptr(), x.data_ptr(), dw1.data_ptr(), db1.data_ptr(), rows, cols,
                                                    max_value, sp, sf, H.stream_ptr())
    w0, b0 = dw1.clone(), db1.clone()
    gw, gb = check_form(launch, need, [dw1, db1], lambda s: [s.reshape(slabs, 2, cols)[:, 0], s.reshape(slabs, 2, cols)[:, 1]])
    gr = torch.where(h1.double() > 0, dh1.double(), torch.zeros_like(dh1, dtype=torch.float64))
    # no plain-form test sets a bound for this kernel.  A column is a float32 sum of 1,000 terms (each product rounded once): the
    # rounding errors of n adds accumulate like a random walk, sqrt(n) * 2^-24 = 1.9e-6 relative to the running sum; twice that
    assert rel(gw.double() - w0.double(), (gr * x.double().clamp(max=max_value)[:, None]).sum(0)) < 4e-6
    assert rel(gb.double() - b0.double(), gr.sum(0)) < 4e-6
