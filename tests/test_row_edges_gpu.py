"""The row and streaming kernels (csrc/elementwise.hip, csrc/optim.hip) element by element at their edges: every output inside a
sentinel frame, every input inside NaN (tests/row_edge_util.py), integer data wherever that makes the result exact in any order, a
float64 reference and a derived bound at every element otherwise (docs/parity.md, "Row and streaming kernels: every element, at
the edges").  Which LayerNorm kernel each listed case reaches is asserted without a GPU in tests/test_row_edges_cpu.py, which also
shows every bound satisfiable.  Only valid calls are launched: the frames exist so that a stray access lands in memory the test owns."""
import ctypes as C
import importlib

import pytest
import torch

import row_cases as RC
import row_edge_util as U

pytestmark = pytest.mark.gpu
F32, BF, I32, U8 = torch.float32, torch.bfloat16, torch.int32, torch.uint8
ALIGN = -2


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def knobs_of(H, case):
    return H.knobs(**{f"k{k}": v for k, v in case["knobs"].items()})          # reset on exit, whatever happens inside


def ids(cases):
    return [c["name"] for c in cases]


def ints(shape, g, amp):
    return torch.randint(-amp, amp + 1, shape, generator=g, device="cuda").float()


def filled(rows, cols, ld, dtype, value, byte_off=0):
    """a guarded output whose view starts from `value` (an accumulated or in-place operand)"""
    o = U.guarded_out(rows, cols, ld, dtype, byte_off=byte_off, device="cuda")
    o.t.copy_(value)
    return o


# ================================================================================================ LayerNorm forward
@pytest.mark.parametrize("case", RC.LN_FWD, ids=ids(RC.LN_FWD))
def test_layernorm_fwd_edges(H, case):
    T = U.ln_fwd_setup(case, gen(3))
    with knobs_of(H, case):
        O = U.ln_fwd_outputs(case, T, True, "cuda")
        H.call("mca_layernorm_fwd", *U.ln_fwd_args(case, T, O), H.stream_ptr())
        torch.cuda.synchronize()
        stats = U.ln_fwd_check(case, T, O)
        if not case["stats"]:          # the same call form without statistics: the same kernel, checked against the statistics above
            O = U.ln_fwd_outputs(case, T, False, "cuda")
            H.call("mca_layernorm_fwd", *U.ln_fwd_args(case, T, O), H.stream_ptr())
            torch.cuda.synchronize()
            U.ln_fwd_check(case, T, O, stats, case["name"] + " (no statistics)")


# ================================================================================================ LayerNorm backward
@pytest.mark.parametrize("case", RC.LN_BWD, ids=ids(RC.LN_BWD))
def test_layernorm_bwd_edges(H, case):
    T = U.ln_bwd_setup(case, gen(4))
    with knobs_of(H, case):
        O = U.ln_bwd_outputs(case, T, "cuda")
        H.call("mca_layernorm_bwd", *U.ln_bwd_args(case, T, O), H.stream_ptr())
        torch.cuda.synchronize()
        U.ln_bwd_check(case, T, O)


@pytest.mark.parametrize("case", RC.LN_BWD, ids=ids(RC.LN_BWD))
def test_layernorm_bwd_det_edges(H, case):
    """the deterministic form: a sentinel-framed scratch of exactly the reported size, the planned slots written and nothing else,
    the same bounds, and two runs bitwise equal"""
    T = U.ln_bwd_setup(case, gen(4))
    cols, slots = case["cols"], case["plan"]["slots"]
    runs = []
    with knobs_of(H, case):
        need = H.lib().mca_layernorm_bwd_det_scratch(case["rows"], cols)
        assert need >= slots * 3 * cols
        for _ in range(2):
            O = U.ln_bwd_outputs(case, T, "cuda", scratch_floats=need)
            H.call("mca_layernorm_bwd_det", *U.ln_bwd_args(case, T, O), O["scratch"].data_ptr(), need, H.stream_ptr())
            torch.cuda.synchronize()
            U.ln_bwd_check(case, T, O, case["name"] + " (det)")
            v = (O["scratch"].t[0].view(I32) != -1).reshape(-1, 3, cols)          # [slot][dgamma | dbeta | dxsum][cols]: stored or still the sentinel
            for k, name in enumerate(("dgamma", "dbeta", "dxsum")):
                assert bool(v[:slots, k].all()) == bool(case[name]) and bool(v[:slots, k].any()) == bool(case[name]), f"{name}: slots 0 .. {slots - 1}"
            assert not v[slots:].any(), f"slots from {slots} on are nobody's"
            runs.append(O)
    for k in ("dx", "dxb", "dgamma", "dbeta", "dxsum"):
        if runs[0][k] is not None:
            it = torch.int16 if k == "dxb" else I32
            assert torch.equal(runs[0][k].t.view(it), runs[1][k].t.view(it)), f"{k}: two runs differ"


# ================================================================================================ casts
def _cast_ref(src, rows_pad, cols_pad, transpose, scale):
    ref = torch.zeros(rows_pad, cols_pad, dtype=BF, device="cuda")
    s = (src * scale).to(BF)
    if transpose:
        ref[:src.shape[1], :src.shape[0]] = s.t()
    else:
        ref[:src.shape[0], :src.shape[1]] = s
    return ref


def test_cast_pad_bf16_edges(H):
    """exact against .to(bfloat16): the single form, then all shapes at two scales in ONE multi launch (scale 0 means 1), one
    destination 2 bytes past a 4-byte boundary"""
    g = gen(21)
    srcs = [U.framed_in(torch.randn(r, c, device="cuda", generator=g), lds) for r, c, lds, *_ in RC.CAST_PAD]
    for src, (r, c, lds, rp, cp, ldd, tr) in zip(srcs, RC.CAST_PAD):
        out = U.guarded_out(rp, cp, ldd, BF, device="cuda")
        H.call("mca_cast_pad_bf16", src.data_ptr(), lds, r, c, out.data_ptr(), ldd, rp, cp, tr, H.stream_ptr())
        torch.cuda.synchronize()
        U.assert_exact(out.t, _cast_ref(src, rp, cp, tr, 1.0), f"cast_pad {(r, c, rp, cp, tr)}")
        U.assert_guard_intact(out, f"cast_pad {(r, c, rp, cp, tr)}")
    jobs = [(i, sc) for sc in (0.0, 0.5) for i in range(len(RC.CAST_PAD))]
    descs = (H.CastDesc * len(jobs))()
    outs = []
    for d, (i, sc) in zip(descs, jobs):
        r, c, lds, rp, cp, ldd, tr = RC.CAST_PAD[i]
        out = U.guarded_out(rp, cp, ldd, BF, byte_off=2 if i in (1, 3) else 0, device="cuda")
        outs.append(out)
        d.src, d.dst, d.lds, d.rows, d.cols, d.ldd, d.rows_pad, d.cols_pad, d.transpose, d.scale = srcs[i].data_ptr(), out.data_ptr(), lds, r, c, ldd, rp, cp, tr, sc
    dev = torch.frombuffer(bytearray(bytes(descs)), dtype=U8).cuda()
    H.call("mca_cast_pad_bf16_multi", dev.data_ptr(), len(jobs), H.stream_ptr())
    torch.cuda.synchronize()
    for out, (i, sc) in zip(outs, jobs):
        r, c, lds, rp, cp, ldd, tr = RC.CAST_PAD[i]
        U.assert_exact(out.t, _cast_ref(srcs[i], rp, cp, tr, sc or 1.0), f"cast_pad_multi {RC.CAST_PAD[i]} scale {sc}")
        U.assert_guard_intact(out, f"cast_pad_multi {RC.CAST_PAD[i]} scale {sc}")


@pytest.mark.parametrize("rows,cols,lds,ldd,dst_off,scale", [(3, 4, 8, 8, 0, 0.5), (1, 260, 264, 268, 8, 1.0), (5, 8, 8, 12, 8, 0.5),
                                                              (1025, 4100, 4104, 4108, 8, 0.5)])
def test_f32_to_bf16_edges(H, rows, cols, lds, ldd, dst_off, scale):
    """exact (a product by 0.5 or 1 is); the last shape has more than 4096 x 256 float4 items: a second pass of the grid-stride loop"""
    src = U.framed_in(torch.randn(rows, cols, device="cuda", generator=gen(22)), lds)
    out = U.guarded_out(rows, cols, ldd, BF, byte_off=dst_off, device="cuda")
    assert out.data_ptr() % 16 == dst_off
    H.call("mca_f32_to_bf16", src.data_ptr(), lds, out.data_ptr(), ldd, rows, cols, scale, H.stream_ptr())
    torch.cuda.synchronize()
    U.assert_exact(out.t, (src * scale).to(BF), "f32_to_bf16")
    U.assert_guard_intact(out, "f32_to_bf16")


def test_f32_to_bf16_alignment_refusals(H):
    L = H.lib()
    src = torch.zeros(64, device="cuda")
    out = U.guarded_out(4, 8, 12, BF, device="cuda")
    s, d = src.data_ptr(), out.data_ptr()
    for args in ((s, 8, d, 12, 4, 6, 1.0), (s, 9, d, 12, 4, 8, 1.0), (s, 8, d, 10, 4, 8, 1.0), (s + 4, 8, d, 12, 4, 8, 1.0), (s, 8, d + 4, 12, 4, 8, 1.0)):
        assert L.mca_f32_to_bf16(*args, H.stream_ptr()) == ALIGN, args
    torch.cuda.synchronize()
    U.assert_guard_intact(out, "refused f32_to_bf16")
    assert (out.t.view(torch.int16) == -1).all()


# ================================================================================================ row broadcast / reduction
def _packed(groups, period, extra=5):
    return [g * (period + extra) + 2 + p for g in range(groups) for p in range(period)]


@pytest.mark.parametrize("cols", [255, 256, 257])
@pytest.mark.parametrize("period", [1, 7])
def test_bcast_rows_edges(H, cols, period):
    rows = 3 * period + (period - 1) // 2          # a partial last group when period > 1
    groups = RC.cdiv(rows, period)
    src = U.int_rows(period, cols, cols + 3, gen(23), 100)
    ldd = cols + 2
    out = U.guarded_out(groups * (period + 5), cols, ldd, F32, device="cuda")
    H.call("mca_bcast_rows", src.data_ptr(), cols + 3, out.data_ptr() + 2 * ldd * 4, ldd, (period + 5) * ldd, period, rows, cols, H.stream_ptr())
    torch.cuda.synchronize()
    dest = _packed(groups, period)[:rows]
    U.assert_exact(out.t[dest], src[torch.arange(rows, device="cuda") % period], "bcast_rows")
    U.assert_rows_untouched(out.t, [r for r in range(groups * (period + 5)) if r not in set(dest)], "bcast_rows")
    U.assert_guard_intact(out, "bcast_rows")


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("knob14", [0, 3])
@pytest.mark.parametrize("cols", [255, 256, 257])
@pytest.mark.parametrize("period", [1, 7])
def test_reduce_rows_edges(H, cols, period, knob14, det):
    """integers: exact in any order, atomics or slots.  37 groups and a partial 38th; knob 14 = 3 workgroups: slabs of many groups"""
    g = gen(24)
    rows = 37 * period + (period - 1) // 2
    groups = RC.cdiv(rows, period)
    lds, ldd = cols + 1, cols + 3
    full = U.framed_in(torch.full((groups * (period + 5), cols), float("nan"), device="cuda"), lds)
    at = _packed(groups, period)[:rows]
    vals = ints((rows, cols), g, 4)
    full[at] = vals
    init = ints((period, cols), g, 3)
    want = init.double()
    want.index_add_(0, torch.arange(rows, device="cuda") % period, vals.double())
    with H.knobs(k14=knob14):
        out = filled(period, cols, ldd, F32, init)
        args = (full.data_ptr() + 2 * lds * 4, lds, (period + 5) * lds, period, out.data_ptr(), ldd, rows, cols)
        if det:
            need = H.lib().mca_reduce_rows_det_scratch(rows, period, cols)
            assert need > 0 and need % (period * cols) == 0
            scratch = U.guarded_out(1, need, need + 3, F32, device="cuda")
            H.call("mca_reduce_rows_det", *args, scratch.data_ptr(), need, H.stream_ptr())
        else:
            H.call("mca_reduce_rows", *args, H.stream_ptr())
        torch.cuda.synchronize()
    U.assert_exact(out.t, want.float(), "reduce_rows")
    U.assert_guard_intact(out, "reduce_rows")
    if det:
        U.assert_guard_intact(scratch, "reduce_rows scratch")
        assert (scratch.t.view(I32) != -1).all(), "every slot of a scratch of exactly the reported size is written"


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("rows,cols", [(5, 4), (3, 260)])
def test_rows_copy_add_edges(H, rows, cols, batch):
    g = gen(25)
    per = rows * cols
    src = U.int_rows(batch, per, per + 8, g, 100)
    init = ints((batch, per), g, 100)
    for accumulate in (0, 1):
        out = filled(batch, per, per + 12, F32, init)
        H.call("mca_rows_copy_add", src.data_ptr(), per + 8, out.data_ptr(), per + 12, rows, cols, batch, accumulate, H.stream_ptr())
        torch.cuda.synchronize()
        U.assert_exact(out.t, (init + src) if accumulate else src.clone(), f"rows_copy_add accumulate {accumulate}")
        U.assert_guard_intact(out, f"rows_copy_add accumulate {accumulate}")


# ================================================================================================ segment means
@pytest.mark.parametrize("cols", [4, 252, 256, 260, 1024])
def test_segment_mean_edges(H, cols):
    """segments of 1, 8, 9 and 3 rows, the last with no live row in sample 0; integer x, so the sums and counts are exact and the
    mean is sum * (1 / count): two roundings.  Padded rows of x hold NaN."""
    g = gen(26)
    batch, seg = 2, [0, 1, 9, 18, 21]
    n_tok, n_seg = seg[-1], len(seg) - 1
    pad = torch.rand(batch, n_tok, device="cuda", generator=g) < 0.35
    pad[:, 0], pad[0, 18:21], pad[1, 1:9], pad[0, 9] = False, True, False, False
    x = ints((batch * n_tok, cols), g, 50)
    x[pad.reshape(-1)] = float("nan")
    xf = U.framed_in(x, cols)
    padu = pad.to(U8).contiguous()
    seg_t = torch.tensor(seg, dtype=I32, device="cuda")
    out, cnt = U.guarded_out(batch * n_seg, cols, cols, F32, device="cuda"), U.guarded_out(1, batch * n_seg, batch * n_seg + 3, I32, device="cuda")
    H.call("mca_segment_mean_fwd", xf.data_ptr(), padu.data_ptr(), seg_t.data_ptr(), n_seg, out.data_ptr(), cnt.t.data_ptr(), batch, n_tok, cols, H.stream_ptr())
    torch.cuda.synchronize()
    live = (~pad).double()
    xz = torch.where(pad.reshape(-1, 1), torch.zeros((), device="cuda", dtype=torch.float64), x.double()).reshape(batch, n_tok, cols)
    counts = torch.stack([live[:, seg[s]:seg[s + 1]].sum(1) for s in range(n_seg)], 1)          # [batch, n_seg]
    sums = torch.stack([xz[:, seg[s]:seg[s + 1]].sum(1) for s in range(n_seg)], 1)
    ref = torch.where(counts[..., None] > 0, sums / counts.clamp_min(1)[..., None], torch.zeros((), device="cuda", dtype=torch.float64)).reshape(-1, cols)
    assert counts[0, 3] == 0 and counts[1, 1] == 8 and counts[0, 0] == 1
    U.assert_exact_rows(cnt.t[0], counts.reshape(-1).to(I32), "segment counts")
    U.close(out.t, ref, 2.0 ** -22 * ref.abs(), "segment means", "segment_mean fwd")
    assert (out.t[3] == 0).all()
    U.assert_guard_intact(out, "segment means"), U.assert_guard_intact(cnt, "segment counts")
    # backward: dx = d_out[segment] * (1 / count) on live rows, exactly 0 on padded ones
    d_out = U.framed_in(ints((batch * n_seg, cols), g, 50), cols)
    seg_of_row = torch.cat([torch.full((seg[s + 1] - seg[s],), s) for s in range(n_seg)]).to(U8).cuda()
    dx = U.guarded_out(batch * n_tok, cols, cols, F32, device="cuda")
    H.call("mca_segment_mean_bwd", d_out.data_ptr(), padu.data_ptr(), seg_of_row.data_ptr(), cnt.t.data_ptr(), n_seg, dx.data_ptr(), batch, n_tok, cols, H.stream_ptr())
    torch.cuda.synchronize()
    sor = seg_of_row.long()
    want = d_out.double().reshape(batch, n_seg, cols)[:, sor] / counts[:, sor].clamp_min(1)[..., None] * live[..., None]
    want = want.reshape(-1, cols)
    U.close(dx.t, want, 2.0 ** -22 * want.abs(), "segment mean backward", "segment_mean bwd")
    U.assert_guard_intact(dx, "segment mean backward")


# ================================================================================================ GEGLU
@pytest.mark.parametrize("rows,ip", RC.GEGLU)
def test_geglu_edges(H, rows, ip):
    g = gen(27)
    h = U.framed_in((torch.randn(rows, 2 * ip, device="cuda", generator=g) * 2).to(BF), 2 * ip)
    out = U.guarded_out(rows, ip, ip, BF, device="cuda")
    H.call("mca_geglu_fwd", h.data_ptr(), out.data_ptr(), rows, ip, H.stream_ptr())
    torch.cuda.synchronize()
    U.close(out.t, *U.geglu_fwd_ref(h, ip), "geglu_fwd", "geglu_fwd")
    U.assert_guard_intact(out, "geglu_fwd")
    dg = U.framed_in(ints((rows, ip), g, 4).to(BF), ip)
    dh = U.guarded_out(rows, 2 * ip, 2 * ip, BF, device="cuda")
    H.call("mca_geglu_bwd", dg.data_ptr(), h.data_ptr(), dh.data_ptr(), rows, ip, H.stream_ptr())
    torch.cuda.synchronize()
    U.close(dh.t, *U.geglu_bwd_ref(dg.double(), h, ip), "geglu_bwd", "geglu_bwd")
    U.assert_guard_intact(dh, "geglu_bwd")


# ================================================================================================ tabular value encoder
@pytest.mark.parametrize("cols", [8, 520])
@pytest.mark.parametrize("rows", [1, 513, 1030])
def test_tab_value_edges(H, rows, cols):
    """forward: padmask exact, h1 within a bf16 step + the fp32 roundings of x w1 + b1.  backward: integer dh1 and the ReLU gate of the
    STORED h1, so db1 is exact and dw1 a column sum of rows + 8 roundings; 513 and 1030 rows: slabs of 2 and 3 rows, the last partial"""
    g = gen(28)
    MAXV, PADV = 5.0, -1.0
    x = torch.randn(rows, device="cuda", generator=g) * 4
    x[::7], x[3::11] = PADV, 9.0
    xf = U.vec_framed(x)
    w1, b1 = U.vec_framed(torch.randn(cols, device="cuda", generator=g)), U.vec_framed(torch.randn(cols, device="cuda", generator=g))
    h1, pm = U.guarded_out(rows, cols, cols, BF, device="cuda"), U.guarded_out(1, rows, rows + 5, torch.int8, device="cuda")
    H.call("mca_tab_value_fwd", xf.data_ptr(), w1.data_ptr(), b1.data_ptr(), h1.data_ptr(), pm.data_ptr(), rows, cols, MAXV, PADV, H.stream_ptr())
    torch.cuda.synchronize()
    ref, tol, mask = U.tab_value_fwd_ref(xf, w1, b1, MAXV, PADV)
    U.assert_exact_rows(pm.t[0], mask.to(torch.int8), "padmask")
    U.close(h1.t, ref, tol, "h1", "tab_value h1")
    U.assert_guard_intact(h1, "h1"), U.assert_guard_intact(pm, "padmask")
    ld = cols + 3
    dh1 = U.int_rows(rows, cols, ld, g, 4)
    iw, ib = ints((cols,), g, 3), ints((cols,), g, 3)
    (dw_ref, dw_tol), db_ref = U.tab_value_bwd_ref(dh1, h1.t, xf, MAXV, iw, ib)
    for det in (0, 1):
        dw, db = filled(1, cols, cols + 3, F32, iw), filled(1, cols, cols + 3, F32, ib)
        args = (dh1.data_ptr(), ld, h1.data_ptr(), xf.data_ptr(), dw.data_ptr(), db.data_ptr(), rows, cols, MAXV)
        if det:
            need = H.lib().mca_tab_value_bwd_det_scratch(rows, cols)
            scratch = U.guarded_out(1, need, need + 3, F32, device="cuda")
            H.call("mca_tab_value_bwd_det", *args, scratch.data_ptr(), need, H.stream_ptr())
        else:
            H.call("mca_tab_value_bwd", *args, H.stream_ptr())
        torch.cuda.synchronize()
        U.assert_exact_rows(db.t[0], db_ref.float(), f"db1 (det {det})")
        U.close(dw.t[0], dw_ref, dw_tol, f"dw1 (det {det})", "tab_value dw1")
        U.assert_guard_intact(dw, "dw1"), U.assert_guard_intact(db, "db1")
        if det:
            U.assert_guard_intact(scratch, "tab_value scratch")
            assert (scratch.t.view(I32) != -1).all()


# ================================================================================================ embedding renorm
@pytest.mark.parametrize("rows,cols", [(7, 1), (9, 63), (9, 64), (9, 65), (4 * 2048 + 3, 64)])
def test_embedding_renorm_edges(H, rows, cols):
    """rows of norm below max_norm (row % 3 == 0), exactly max_norm (one non-zero element: the fp32 norm is exact) and above it.
    The first two stay bitwise; a rescaled row is within 2^-20 of w max_norm / (norm + 1e-7): a dozen fp32 roundings."""
    g = gen(29)
    MAXN = 2.0
    w = torch.randn(rows, cols, device="cuda", generator=g).double()
    w = torch.where(w == 0, torch.ones_like(w), w)
    kind = torch.arange(rows, device="cuda") % 3
    target = torch.where(kind == 0, 0.3 + 0.6 * torch.rand(rows, device="cuda", generator=g).double(), 1.1 + 2 * torch.rand(rows, device="cuda", generator=g).double()) * MAXN
    w = (w / w.norm(dim=1, keepdim=True) * target[:, None]).float()
    eq = (kind == 1).nonzero().flatten()
    w[eq] = 0
    w[eq, eq % cols] = torch.where(eq % 2 == 0, MAXN, -MAXN).float()
    buf = filled(rows, cols, cols, F32, w)
    H.call("mca_embedding_renorm", buf.data_ptr(), rows, cols, MAXN, H.stream_ptr())
    torch.cuda.synchronize()
    norm = w.double().norm(dim=1, keepdim=True)
    assert (norm[kind == 0] < MAXN * 0.95).all() and (norm[kind == 1] == MAXN).all() and (norm[kind == 2] > MAXN * 1.05).all()
    keep = (kind != 2)[:, None].expand(-1, cols)
    ref = torch.where(keep, w.double(), w.double() * MAXN / (norm + 1e-7))
    U.close(buf.t, ref, torch.where(keep, torch.zeros_like(ref), 2.0 ** -20 * ref.abs()), "embedding_renorm", "embedding_renorm")
    assert torch.equal(buf.t.view(I32)[kind != 2], w.view(I32)[kind != 2]), "rows at or below max_norm are bitwise untouched"
    U.assert_guard_intact(buf, "embedding_renorm")


# ================================================================================================ finite check
def test_nonfinite_flag_edges(H):
    """one planted non-finite value at the ends of the 16-byte part and of the scalar tail of one of one to four tensors; bases 16 and
    4 bytes aligned (the second has no 16-byte part); the flag gets exactly the requested bit on top of a pre-set other one"""
    L = H.lib()
    OTHER, BIT = 8, 2
    flag = torch.zeros(1, dtype=I32, device="cuda")
    host = torch.zeros(1, dtype=I32).pin_memory()
    FLT_MAX, DENORM = 3.4028234663852886e38, 1e-41

    def run(tensors):
        fa = H.FiniteArgs()
        for i, (t, n) in enumerate(tensors):
            fa.p[i], fa.n[i] = t.data_ptr(), n
        fa.count = len(tensors)
        flag.fill_(OTHER)
        assert L.mca_nonfinite_flag(C.byref(fa), flag.data_ptr(), BIT, H.stream_ptr()) == 0
        assert L.mca_flag_to_host(flag.data_ptr(), host.data_ptr(), H.stream_ptr()) == 0
        torch.cuda.current_stream().synchronize()
        assert int(host[0]) == int(flag.item()), "the pinned host word is the device word"
        return int(host[0])

    def finite(n, off):
        """(tensor, n): all finite, FLT_MAX and a denormal among the values; n == 0: a valid address and no element (what follows it is NaN)"""
        t = U.vec_framed(torch.randn(max(n, 1), device="cuda"), off)
        if n == 0:
            t[0] = float("nan")
        else:
            t[0] = FLT_MAX
            t[n - 1] = -DENORM if n > 1 else -FLT_MAX
        return t, n

    checked = 0
    for off in (0, 4):
        for ni, n in enumerate(RC.FLAG_N):
            count = 1 + ni % 4
            others = [finite(RC.FLAG_N[(ni + 1 + k) % len(RC.FLAG_N)], off) for k in range(count - 1)]
            which = ni % count
            t, _ = finite(n, off)
            assert t.data_ptr() % 16 == off
            tensors = others[:which] + [(t, n)] + others[which:]
            assert run(tensors) == OTHER, f"all finite (FLT_MAX, denormals), n {n}, base + {off}"
            for pos in sorted({0, 4 * (n // 4) - 1, 4 * (n // 4), n - 1}):
                if not 0 <= pos < n:
                    continue
                for bad in (float("inf"), float("-inf"), float("nan")):
                    keep = float(t[pos])
                    t[pos] = bad
                    assert run(tensors) == OTHER | BIT, f"{bad} at element {pos} of {n} (tensor {which} of {count}, base + {off})"
                    t[pos] = keep
                    checked += 1
            assert run(tensors) == OTHER
    assert checked >= 2 * 3 * 10


# ================================================================================================ optimizer
SQ_WORDS = 1026          # MCA_SQNORM_WORDS


def sqnorm_words(H, g_view, n, fill=-7.0):
    sq = filled(1, SQ_WORDS, SQ_WORDS + 3, F32, torch.full((1, SQ_WORDS), fill, device="cuda"))
    H.call("mca_grad_sqnorm", g_view.data_ptr(), n, sq.data_ptr(), H.stream_ptr())
    torch.cuda.synchronize()
    U.assert_guard_intact(sq, "sqnorm words")
    return sq.t[0]


@pytest.mark.parametrize("n", RC.SQNORM_N + [2 * 256 * 1024 * 4 + 7])
def test_grad_sqnorm_edges(H, n):
    """g in {-2 .. 2}: every partial sum is an integer below 2^24, so word 0 is exact.  The listed sizes end at one full pass of 1024
    blocks + a scalar tail of 3 (only block 0 adds it); the added one takes a second pass of the grid-stride loop."""
    g = U.vec_framed(ints((n,), gen(30), 2))
    want = float((g.double() ** 2).sum())
    assert want < 2 ** 24
    blocks = max(1, min(RC.cdiv(n // 4, 256), SQ_WORDS - 2))
    w = sqnorm_words(H, g, n)
    assert float(w[0]) == want, (float(w[0]), want)
    root = torch.tensor(want, dtype=torch.float64).sqrt()
    assert abs(float(w[-1]) - float(root)) <= float(root.float()) * 2.0 ** -23, "the last word: one ulp of sqrt"
    assert (w[1 + blocks:-1] == -7.0).all(), "words between the used slots and the last word keep the caller's fill"
    assert float(w[1:1 + blocks].double().sum()) == want
    assert torch.equal(w.view(I32), sqnorm_words(H, g, n).view(I32)), "two runs are bitwise equal"


def test_grad_sqnorm_alignment_refusal(H):
    g = U.vec_framed(torch.ones(16, device="cuda"), 4)
    sq = torch.zeros(SQ_WORDS, device="cuda")
    assert H.lib().mca_grad_sqnorm(g.data_ptr(), 16, sq.data_ptr(), H.stream_ptr()) == ALIGN
    torch.cuda.synchronize()
    assert (sq == 0).all()


HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01)


@pytest.mark.parametrize("n", RC.ADAMW_N)
@pytest.mark.parametrize("form", ["below", "above", "max_norm0", "no_sqnorm", "hyper", "skip0", "skip1"])
def test_adamw_step_edges(H, n, form):
    """three chained steps from non-zero m and v against a float64 reference per element that starts each step from the kernel's own
    previous state and its own (checked) sum g^2; 4096 x 256 + 3 elements: the three of the second pass"""
    L = H.lib()
    g = gen(31)
    rnd = lambda s=1.0: torch.randn(1, n, device="cuda", generator=g) * s
    p, m, v = filled(1, n, n + 3, F32, rnd()), filled(1, n, n + 3, F32, rnd(0.1)), filled(1, n, n + 3, F32, rnd(0.1).abs() * 0.1)
    hyper = torch.zeros(3, device="cuda")
    flagw = torch.full((1,), 1 if form == "skip1" else 0, dtype=I32, device="cuda")
    for step in (1, 2, 3):
        gr = U.vec_framed(rnd()[0])
        words = sqnorm_words(H, gr, n)
        sq64 = float((gr.double() ** 2).sum())
        assert abs(float(words[0]) - sq64) <= 2.0 ** -18 * sq64, "sum g^2: some 40 fp32 roundings in a tree of depth 40 at the most"
        norm = sq64 ** 0.5
        max_norm = dict(below=2 * norm, above=0.5 * norm, max_norm0=0.0).get(form, 0.5 * norm)
        bc1, bc2 = 1 - 0.9 ** step, 1 - 0.999 ** step
        p0, m0, v0 = p.t[0].clone(), m.t[0].clone(), v.t[0].clone()
        use_norm = form != "no_sqnorm"
        ref = U.adamw_ref(p0, gr, m0, v0, float(words[0]), **HP, bc1=bc1, bc2=bc2, max_norm=max_norm, use_norm=use_norm)
        scal = (HP["lr"], bc1, bc2)
        if form == "hyper":          # the step's values come from device memory; the scalar arguments must be ignored
            assert L.mca_adamw_hyper(hyper.data_ptr(), *scal, H.stream_ptr()) == 0
            scal = (123.0, 0.5, 0.25)
        H.call("mca_adamw_step", p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), n, scal[0], HP["b1"], HP["b2"], HP["eps"], HP["wd"], scal[1], scal[2],
               max_norm, words.data_ptr() if use_norm else None, flagw.data_ptr() if form.startswith("skip") else None,
               hyper.data_ptr() if form == "hyper" else None, H.stream_ptr())
        torch.cuda.synchronize()
        if form == "hyper":
            assert hyper.tolist() == [U.f32(HP["lr"]), U.f32(bc1), U.f32(bc2)]
        if form == "below":
            assert max_norm / (float(words[0]) ** 0.5 + 1e-6) > 1          # the clip is exactly 1
        for name, buf, old in (("p", p, p0), ("m", m, m0), ("v", v, v0)):
            if form == "skip1":
                assert torch.equal(buf.t[0].view(I32), old.view(I32)), f"step {step}: {name} changed under a set skip flag"
            else:
                U.close(buf.t[0], *ref[name], f"step {step}: {name} (row = 0)", f"adamw {name}")
            U.assert_guard_intact(buf, name)


def test_print_worst_ratios():
    """last in the file: the largest error / bound ratio of every bounded output over the cases above (pytest -s shows it)"""
    for k in sorted(U.WORST):
        print(f"worst |got - ref| / bound  {k:24s} {U.WORST[k]:.3f}")
    assert U.WORST
