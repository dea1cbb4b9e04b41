"""The head-major entry points (mca_attn_fwd_hm, mca_attn_vmean_if_needed_hm, mca_attn_bwd_prep_onepass_hm, mca_attn_bwd_onepass_hm)
against the entry points they stand beside, on the same values in the two layouts: q | k | v as the (b n, 3 D) matrix and dO as
(b n, D) through the old calls (the one-pass backward with its packed copies), and as the slabs [block][T][64] that mca_gemm_nt_cb
writes, read in place, through the new ones.  Same kernels, same values in the same order: o, lse, vmean, the row constants,
dvmean, dq, dk and dv must agree BIT FOR BIT.  (What the old entry points compute is checked against float64 in
tests/test_attention_edges_gpu.py.)

Cases from tests/attention_cases.py, their first two samples, 2 heads: tail257 (N = 257, not a multiple of 64; sample 0 without
its first modality, so rows with lse = +inf exist and dvmean is not zero) and aligned256 (sample 0 likewise; dead key blocks).
The slabs lie (T + 64) rows apart: 64 rows of slack behind each, which the pipelined kernel's unclamped tile reads reach; they are
zeros in one run and random finite values in another, and no bit may change.  o, dq and dk | dv are guarded outputs, the row
constants sit between sentinels."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import attention_cases as AC
import attention_edge_util as U
import gemm_edge_util as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDER = 8
B = 2
SLACK = 64              # rows between two slabs
RC_GUARD = 256          # sentinel floats in front of and behind the row constants
RC_SENTINEL = 12345.0


@pytest.fixture(scope="module")
def H():
    importlib.import_module("mca-paper_amd.build").build()
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def blocked(x, T, slack_fill):
    """(T, n * 64) bf16 -> the flat buffer of n slabs [T + SLACK][64]; the slack rows zeros or random finite values"""
    n = x.shape[1] // 64
    buf = torch.zeros(n, T + SLACK, 64, dtype=torch.bfloat16, device=DEV)
    if slack_fill == "randn":
        buf[:, T:] = (torch.randn(n, SLACK, 64, generator=torch.Generator().manual_seed(5)) * 3.0).to(torch.bfloat16).to(DEV)
    buf[:, :T] = x.view(T, n, 64).permute(1, 0, 2)
    return buf.view(-1)


_CTX = {}


def context(H, case):
    if case in _CTX:
        return _CTX[case]
    att = importlib.import_module("mca-paper_amd.attention")
    c = U.make_operands(case, "mca", False, DEV)
    st, N, D, heads = c["st"], c["N"], c["D"], c["heads"]
    T = B * N
    c["T"], c["att"] = T, att
    c["qkv"], c["d_o"], c["pad"] = c["qkv"][:B].reshape(T, 3 * D).contiguous(), c["d_o"][:B].reshape(T, D).contiguous(), c["pad"][:B]
    c["do_f"] = G.framed_copy(c["d_o"], D + WIDER)          # mca_attn_bwd_prep_onepass reads o and d_o with ONE pair of strides: o's
    c["sf"] = att._Sched(st.attn_schedule(128, 64), DEV)
    c["qmask"] = torch.from_numpy(c["qmask_np"].astype(np.uint32).view(np.int32)).to(DEV)
    kgroup = torch.from_numpy(st.kgroup).to(DEV)
    nk_pad = AC.nk_pad_of(N)
    keyinfo, kflags = torch.empty(B, nk_pad, dtype=torch.uint8, device=DEV), torch.empty(B, (N + 63) // 64, dtype=torch.uint8, device=DEV)
    H.call("mca_build_keyinfo", c["pad"].to(torch.uint8).data_ptr(), kgroup.data_ptr(), keyinfo.data_ptr(), kflags.data_ptr(), B, N, nk_pad, H.stream_ptr())
    khot = torch.empty(B, nk_pad, 16, dtype=torch.bfloat16, device=DEV)
    H.call("mca_build_keyhot", keyinfo.data_ptr(), khot.data_ptr(), B, nk_pad, H.stream_ptr())
    qb = (torch.from_numpy(c["qmask_np"].astype(np.int64)).to(DEV)[:, None] >> torch.arange(16, device=DEV)[None, :]) & 1
    qb[:, 15] = 0
    c["qblk"] = torch.where(qb == 1, 0.0, -32768.0).to(torch.bfloat16).contiguous()
    c["keys"] = att.AttnKeys(keyinfo, kflags, khot, N, nk_pad, B, heads, U.SCALE, H.ATTN_Q_PRESCALED)          # khot: the LDS-DMA forward
    # presence bits as mca_pack_masks sets them: a sample with every modality present has no uniform row, both calls skip its mean(V)
    c["present_bits"] = [sum(1 << m for m, ln in enumerate(lens) if ln > 0) for lens in AC.CASES[case]["lengths"][:B]]
    c["present"] = torch.tensor(c["present_bits"], dtype=torch.int32, device=DEV)
    c["sc"] = att._OnePassSched(AC.onepass_tables(st, True), DEV)
    assert c["sc"].fits
    c["cbs"] = (T + SLACK) * 64
    _CTX[case] = c
    return c


def operands(c, layout, o=None, lse=None, slack="zero"):
    """-> (AttnOperands, the buffers that must stay alive) in the row-major or the head-major layout"""
    att, N, D, heads, T, cbs = c["att"], c["N"], c["D"], c["heads"], c["T"], c["cbs"]
    if layout == "rows":
        return att.AttnOperands(c["qkv"].data_ptr(), N * 3 * D, 3 * D, c["qkv"], D, 2 * D, 3 * D, o, lse, N, c["qmask"], c["qblk"], c["sf"], None, None), None
    buf = blocked(c["qkv"], T, slack)
    return att.AttnOperands(buf.data_ptr(), N * 64, 64, buf, heads * cbs, 2 * heads * cbs, 64, o, lse, N, c["qmask"], c["qblk"], c["sf"], None, None, cbs), buf


def forward(H, c, layout, lazy, slack="zero"):
    att, N, D, heads = c["att"], c["N"], c["D"], c["heads"]
    o = G.guarded_out(B * N, D, D + WIDER, torch.bfloat16, device=DEV)
    lse = torch.full((B, heads, N), float("nan"), device=DEV)
    vmean = torch.full((B, D), 7.0, device=DEV)
    ops, keep = operands(c, layout, o.t, lse, slack)
    keys = c["keys"]._replace(flags=H.ATTN_Q_PRESCALED | (H.ATTN_LAZY_REFERENCE if lazy else 0))
    a = att.fwd_args(ops, keys, vmean)
    if layout == "rows":
        H.call("mca_attn_vmean_if_needed", a.v, a.kv_bstride, a.kv_ld, vmean.data_ptr(), B, N, heads, c["present"].data_ptr(), 0b111, H.stream_ptr())
        H.call("mca_attn_fwd", C.byref(a), H.stream_ptr())
    else:
        lay = att.layout_args(ops)
        assert lay.q_hstride == lay.kv_hstride == c["cbs"]
        H.call("mca_attn_vmean_if_needed_hm", a.v, a.kv_bstride, a.kv_ld, lay.kv_hstride, vmean.data_ptr(), B, N, heads, c["present"].data_ptr(), 0b111,
               H.stream_ptr())
        H.call("mca_attn_fwd_hm", C.byref(a), C.byref(lay), H.stream_ptr())
    torch.cuda.synchronize()
    G.assert_guard_intact(o, f"o ({layout})")
    return o, lse, vmean


def framed_rowc(c):
    """the row constants as the caller initialises them (-inf | 0 past a tile's rows and in the null tile, NaN where the prep writes)
    between two runs of sentinel floats -> (whole buffer, the (b, heads, tiles + 1, 2, 64) view)"""
    sc, heads = c["sc"], c["heads"]
    nqt = sc.n_qt
    n = B * heads * (nqt + 1) * 128
    buf = torch.full((RC_GUARD + n + RC_GUARD,), RC_SENTINEL, device=DEV)
    rowc = buf[RC_GUARD:RC_GUARD + n].view(B, heads, nqt + 1, 2, 64)
    rowc.fill_(float("nan"))
    for t, (r0, rn) in enumerate(sc.s.qt_desc.tolist() + [[0, 0]]):
        rowc[:, :, t, 0, rn:] = float("-inf")
        rowc[:, :, t, 1, rn:] = 0.0
    return buf, rowc


def backward(H, c, layout, o, lse, split, slack="zero"):
    """prep + one-pass backward in one layout -> dict(rowc, dvmean, dq, dkv)"""
    att, N, D, heads, T, cbs, sc = c["att"], c["N"], c["D"], c["heads"], c["T"], c["cbs"], c["sc"]
    rc_buf, rowc = framed_rowc(c)
    dvmean = torch.full((B, D), float("nan"), device=DEV)
    dq = G.guarded_out(T, D, D + WIDER, torch.bfloat16, device=DEV)
    dkv = G.guarded_out(T, 3 * D, 3 * D + WIDER, torch.bfloat16, device=DEV)
    acc = torch.full((B * heads * max(1, split) * (sc.n_qt + 1) * 4096,), float("nan"), device=DEV)
    ops, keep = operands(c, layout, o.t, lse, slack)
    grads = att.AttnGrads(c["d_o"], None, dq.data_ptr(), N * (D + WIDER), D + WIDER, False, dkv.t, D, 2 * D, 3 * D + WIDER)
    if layout == "rows":
        packed = [torch.zeros((B * heads * N + 64) * 64, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
        H.call("mca_attn_bwd_prep_onepass", o.data_ptr(), c["do_f"].data_ptr(), N * (D + WIDER), D + WIDER, lse.data_ptr(), sc.row_slot.data_ptr(),
               rowc.data_ptr(), dvmean.data_ptr(), B, heads, N, sc.n_qt, c["qkv"].data_ptr(), N * 3 * D, 3 * D, packed[0].data_ptr(),
               packed[1].data_ptr(), H.stream_ptr())
        a = att.bwd1_args(ops, grads, c["keys"], sc, rowc, acc, dvmean, split, *[att.RowSource(x.data_ptr(), heads * N * 64, N * 64, 64) for x in packed])
        H.call("mca_attn_bwd_onepass", C.byref(a), H.stream_ptr())
    else:
        do_buf = blocked(c["d_o"], T, slack)
        # (o is row-major with its own stride: a guarded output; d_o wherever its rows lie, here inside the frame-less matrix)
        H.call("mca_attn_bwd_prep_onepass_hm", o.data_ptr(), N * (D + WIDER), D + WIDER, do_buf.data_ptr(), N * 64, cbs, 64, lse.data_ptr(),
               sc.row_slot.data_ptr(), rowc.data_ptr(), dvmean.data_ptr(), B, heads, N, sc.n_qt, H.stream_ptr())
        a = att.bwd1_args(ops, grads, c["keys"], sc, rowc, acc, dvmean, split, att.RowSource(ops.q, N * 64, cbs, 64),
                          att.RowSource(do_buf.data_ptr(), N * 64, cbs, 64))
        H.call("mca_attn_bwd_onepass_hm", C.byref(a), C.byref(att.layout_args(ops)), H.stream_ptr())
    torch.cuda.synchronize()
    assert bool((rc_buf[:RC_GUARD] == RC_SENTINEL).all()) and bool((rc_buf[-RC_GUARD:] == RC_SENTINEL).all()), f"a store outside the row constants ({layout})"
    G.assert_guard_intact(dq, f"dq ({layout})")
    G.assert_guard_intact(dkv, f"dk | dv ({layout})")
    return dict(rowc=rowc.clone(), dvmean=dvmean, dq=dq.t.clone(), dkv=dkv.t[:, D:].clone())


@pytest.mark.parametrize("case", ["tail257", "aligned256"])
@pytest.mark.parametrize("lazy", [False, True], ids=["textbook", "lazy"])
def test_forward_head_major_matches_row_major_bit_for_bit(H, case, lazy):
    c = context(H, case)
    o_r, lse_r, vm_r = forward(H, c, "rows", lazy)
    assert torch.isfinite(o_r.t.float()).all() and bool(torch.isinf(lse_r[0]).any()) and bool(torch.isfinite(lse_r).any())          # uniform rows exist
    for s, bits_ in enumerate(c["present_bits"]):          # computed where a modality is missing, left alone elsewhere
        assert bool((vm_r[s] == 7.0).all()) == (bits_ == 0b111) and (bits_ == 0b111 or float(vm_r[s].abs().max()) > 0)
    assert c["present_bits"][0] != 0b111
    for slack in ("zero", "randn"):
        o_h, lse_h, vm_h = forward(H, c, "hm", lazy, slack)
        assert same_bits(o_h.t, o_r.t), f"o differs ({slack} slack)"
        assert same_bits(lse_h, lse_r), f"lse differs ({slack} slack)"
        assert same_bits(vm_h, vm_r), f"vmean differs ({slack} slack)"


@pytest.mark.parametrize("case", ["tail257", "aligned256"])
@pytest.mark.parametrize("split", [1, 2])
def test_onepass_backward_head_major_matches_row_major_bit_for_bit(H, case, split):
    c = context(H, case)
    o, lse, _ = forward(H, c, "rows", False)
    ref = backward(H, c, "rows", o, lse, split)
    assert all(torch.isfinite(ref[k].float()).all() for k in ("dvmean", "dq", "dkv"))
    assert float(ref["dvmean"][0].abs().max()) > 0 and float(ref["dq"].float().abs().max()) > 0          # uniform rows feed dvmean
    assert not torch.isnan(ref["rowc"]).any()
    for slack in ("zero", "randn"):
        got = backward(H, c, "hm", o, lse, split, slack)
        for k in ("rowc", "dvmean", "dq", "dkv"):
            assert same_bits(got[k], ref[k]), f"{k} differs from the row-major run (split {split}, {slack} slack)"


def test_hm_entries_with_a_null_layout_are_the_plain_entries(H):
    """layout NULL: exactly mca_attn_fwd on the row-major operands; a misaligned head stride is refused"""
    c = context(H, "tail257")
    att, N, D, heads = c["att"], c["N"], c["D"], c["heads"]
    o_r, lse_r, _ = forward(H, c, "rows", True)
    o = G.guarded_out(B * N, D, D + WIDER, torch.bfloat16, device=DEV)
    lse = torch.full((B, heads, N), float("nan"), device=DEV)
    vmean = torch.full((B, D), 7.0, device=DEV)
    H.call("mca_attn_vmean_if_needed_hm", c["qkv"].data_ptr() + 4 * D, N * 3 * D, 3 * D, 0, vmean.data_ptr(), B, N, heads, c["present"].data_ptr(), 0b111,
           H.stream_ptr())
    a = att.fwd_args(operands(c, "rows", o.t, lse)[0], c["keys"]._replace(flags=H.ATTN_Q_PRESCALED | H.ATTN_LAZY_REFERENCE), vmean)
    H.call("mca_attn_fwd_hm", C.byref(a), None, H.stream_ptr())
    torch.cuda.synchronize()
    assert same_bits(o.t, o_r.t) and same_bits(lse, lse_r)
    assert H.lib().mca_attn_fwd_hm(C.byref(a), C.byref(H.AttnLayout(68, 64)), H.stream_ptr()) == -2
    assert H.lib().mca_attn_fwd_hm(C.byref(a), C.byref(H.AttnLayout(64, 68)), H.stream_ptr()) == -2
