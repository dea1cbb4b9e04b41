"""The attention kernels element by element at tile and padding edges (docs/parity.md, "Attention edges"), through the C ABI:
mca_attn_fwd in its three forms, mca_attn_bwd_prep / mca_attn_bwd_dq / mca_attn_bwd_dkv in every form, mca_attn_bwd_prep_onepass /
mca_attn_bwd_onepass on both tables, from strided and packed operands, plain, pipelined and split.  The cases (tests/attention_cases.py)
put modality and padding boundaries ON multiples of 64 / 128 / 256 and one element past them; what each reaches is asserted in
tests/test_attention_edges_cpu.py.  Every output is compared with a float64 reference that shares every input with the kernel
(tests/attention_edge_util.py): each element within a derived bound, each 64-column row within half of its bound's norm.

Operands sit inside NaN (row stride 8 elements wider than the matrix, guard rows in front and behind); o, dq and the dk | dv matrix
are sentinel-filled guarded outputs (an element nobody stores stays NaN, a store outside the view is found); lse, delta, the row
constants and the dQ workspace start as NaN."""
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
WIDER = 8          # row stride of every framed / guarded matrix: its columns + 8 elements


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    yield hip
    if U.STATS:
        print("\nlargest |got - ref| / bound per tensor and form (element, row):\n" + U.stats_table())


def nan_f32(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


_CTX = {}


def context(H, case, variant, pool):
    """Operands, tables, the forward's o / lse (register-staged form), mca_attn_bwd_prep's delta / dvmean and the float64 references
    of one case: built once, shared by its tests, never modified."""
    key = (case, variant, pool)
    if key in _CTX:
        return _CTX[key]
    att = importlib.import_module("mca-paper_amd.attention")
    c = U.make_operands(case, variant, pool, DEV)
    st, b, N, D, nq, heads = c["st"], c["b"], c["N"], c["D"], c["nq"], c["heads"]
    c["qkv_f"] = G.framed_copy(c["qkv"].view(b * N, 3 * D), 3 * D + WIDER)
    c["do_f"] = G.framed_copy(c["d_o"].view(b * nq, D), D + WIDER)
    c["kv_ld"], c["kv_bstride"], c["o_ld"], c["o_bstride"] = 3 * D + WIDER, N * (3 * D + WIDER), D + WIDER, nq * (D + WIDER)
    if pool:
        c["qsrc_f"] = G.framed_copy(c["qsrc"], D + WIDER)
        c["q_ptr"], c["q_bstride"], c["q_ld"] = c["qsrc_f"].data_ptr(), 0, D + WIDER
    else:
        c["q_ptr"], c["q_bstride"], c["q_ld"] = c["qkv_f"].data_ptr(), c["kv_bstride"], c["kv_ld"]
    c["v_ptr"] = c["qkv_f"].data_ptr() + 2 * D * 2
    c["sf"] = att._Sched(st.pool_schedule(128, 64) if pool else st.attn_schedule(128, 64), DEV)
    c["sb"] = {bk: att._Sched(st.pool_schedule(64, bk) if pool else st.attn_schedule(64, bk), DEV) for bk in (256, 128)}
    c["qmask"] = torch.from_numpy(c["qmask_np"].astype(np.uint32).view(np.int32)).to(DEV)
    kgroup = torch.from_numpy(st.kgroup).to(DEV)
    nk_pad = c["nk_pad"] = AC.nk_pad_of(N)
    c["keyinfo"] = torch.full((b, nk_pad), 77, dtype=torch.uint8, device=DEV)
    c["kflags"] = torch.full((b, (N + 63) // 64), 77, dtype=torch.uint8, device=DEV)
    H.call("mca_build_keyinfo", c["pad"].to(torch.uint8).data_ptr(), kgroup.data_ptr(), c["keyinfo"].data_ptr(), c["kflags"].data_ptr(), b, N,
           nk_pad, H.stream_ptr())
    c["khot"] = torch.empty(b, nk_pad, 16, dtype=torch.bfloat16, device=DEV)
    H.call("mca_build_keyhot", c["keyinfo"].data_ptr(), c["khot"].data_ptr(), b, nk_pad, H.stream_ptr())
    qb = (torch.from_numpy(c["qmask_np"].astype(np.int64)).to(DEV)[:, None] >> torch.arange(16, device=DEV)[None, :]) & 1
    qb[:, 15] = 0
    c["qblk"] = torch.where(qb == 1, 0.0, -32768.0).to(torch.bfloat16).contiguous()
    c["vmean"] = nan_f32(b, D)
    # the records the builders of attention.py take; the framed operands go in through the stride fields, o / lse per launch
    c["att"] = att
    c["keys"] = att.AttnKeys(c["keyinfo"], c["kflags"], c["khot"], N, nk_pad, b, heads, U.SCALE, H.ATTN_Q_PRESCALED)
    c["ops"] = att.AttnOperands(c["q_ptr"], c["q_bstride"], c["q_ld"], c["qkv_f"], D, 2 * D, c["kv_ld"], None, None, nq, c["qmask"], c["qblk"],
                                c["sf"], None, None)
    H.call("mca_attn_vmean", c["v_ptr"], c["kv_bstride"], c["kv_ld"], c["vmean"].data_ptr(), b, N, heads, H.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(c["kflags"].cpu(), torch.from_numpy(AC.ktile_flags(c["pad"].cpu().numpy())))          # the restated rule IS the kernel's
    want_info = torch.where(c["pad"], torch.full_like(c["pad"], 31, dtype=torch.uint8), kgroup[None].expand(b, -1))
    assert torch.equal(c["keyinfo"][:, :N], want_info) and (c["keyinfo"][:, N:] == 31).all()
    c["q4"], c["k4"], c["v4"], c["do4"] = U.head_operands(c)
    U.check_elements(U.heads4(c["vmean"][:, None], b), c["v4"].mean(2, keepdim=True), (N + 2) * U.ACC * c["v4"].abs().mean(2, keepdim=True), "vmean",
                     names=("sample", "head", "-", "column"))
    c["fwd_ref"] = U.forward_ref(c["q4"], c["k4"], c["v4"], c["blk"])
    # the forward whose o / lse the backward is given: the register-staged form
    c["o"], c["lse"] = run_forward(H, c, khot=False, lazy=False)
    c["ops"] = c["ops"]._replace(o=c["o"].t, lse=c["lse"])
    c["o4"] = U.heads4(c["o"].t, b)
    # mca_attn_bwd_prep on them
    c["delta"], c["dvmean"] = nan_f32(b, heads, nq), nan_f32(b, D)
    H.call("mca_attn_bwd_prep", c["o"].data_ptr(), c["do_f"].data_ptr(), c["o_bstride"], c["o_ld"], c["lse"].data_ptr(), c["delta"].data_ptr(),
           c["dvmean"].data_ptr(), b, heads, nq, N, H.stream_ptr())
    torch.cuda.synchronize()
    c["dvmean4"] = U.heads4(c["dvmean"][:, None], b)
    _CTX[key] = c
    return c


def run_forward(H, c, khot, lazy):
    b, N, D, nq, heads = c["b"], c["N"], c["D"], c["nq"], c["heads"]
    o = G.guarded_out(b * nq, D, D + WIDER, torch.bfloat16, device=DEV)
    lse = nan_f32(b, heads, nq)
    keys = c["keys"]._replace(khot=c["khot"] if khot else None, flags=H.ATTN_Q_PRESCALED | (H.ATTN_LAZY_REFERENCE if lazy else 0))
    a = c["att"].fwd_args(c["ops"]._replace(o=o.t, lse=lse), keys, c["vmean"])
    H.call("mca_attn_fwd", C.byref(a), H.stream_ptr())
    torch.cuda.synchronize()
    return o, lse


def bwd2_args(H, c, dq, dq_f32, dkv, bkeys, hot):
    b, N, D, nq, heads = c["b"], c["N"], c["D"], c["nq"], c["heads"]
    grads = c["att"].AttnGrads(c["do_f"], c["delta"], dq.data_ptr(), nq * (D + WIDER), D + WIDER, dq_f32, dkv.t, D, 2 * D, 3 * D + WIDER)
    return c["att"].bwd2_args(c["ops"], grads, c["keys"] if hot else c["keys"]._replace(khot=None), c["dvmean"], c["sb"][bkeys])


def new_dq(c, f32=False):
    return G.guarded_out(c["b"] * c["nq"], c["D"], c["D"] + WIDER, torch.float32 if f32 else torch.bfloat16, device=DEV)


def new_dkv(c):
    return G.guarded_out(c["b"] * c["N"], 3 * c["D"], 3 * c["D"] + WIDER, torch.bfloat16, device=DEV)


def dkv_heads(c, dkv):
    """(dk, dv) in head form; the q columns of the dk | dv matrix and its guard bands still hold the sentinel"""
    D = c["D"]
    G.assert_guard_intact(dkv, "dk | dv matrix")
    assert (bits(dkv.t[:, :D]) == -1).all(), "a store into the q columns of the dk | dv matrix"
    return U.heads4(dkv.t[:, D:2 * D], c["b"]), U.heads4(dkv.t[:, 2 * D:], c["b"])


def ids(params):
    return ["-".join(str(x) for x in p) for p in params]


FWD_PARAMS = [(c, v, False) for c, v in AC.SELF] + [(c, v, True) for c, v in AC.POOL]


# ------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("case,variant,pool", FWD_PARAMS, ids=ids(FWD_PARAMS))
def test_forward_forms(H, case, variant, pool):
    """register-staged, LDS-DMA (khot) and lazy-reference forms: o per element and row, uniform rows flagged exactly, lse of
    the other rows within its derived bound (below 1e-4 log2 units); the first two bit for bit equal"""
    c = context(H, case, variant, pool)
    ref = c["fwd_ref"]
    assert float(ref["lse_bound"].max()) < 1e-4
    outs = {}
    for form, (khot, lazy) in {"staged": (False, False), "dma": (True, False), "lazy": (True, True)}.items():
        o, lse = (c["o"], c["lse"]) if form == "staged" else run_forward(H, c, khot, lazy)
        G.assert_guard_intact(o, f"o ({form})")
        U.check_forward(U.heads4(o.t, c["b"]), lse, ref, f"{case} {variant} pool={pool} forward ({form})", label=f"fwd {form}")
        outs[form] = (o, lse)
    assert same_bits(outs["staged"][0].t, outs["dma"][0].t) and same_bits(outs["staged"][1], outs["dma"][1])
    o2, lse2 = run_forward(H, c, True, True)
    assert same_bits(o2.t, outs["lazy"][0].t) and same_bits(lse2, outs["lazy"][1])          # a second launch: the same bits


# ------------------------------------------------------------------------------------------- two-pass backward
@pytest.mark.parametrize("case,variant,pool", FWD_PARAMS, ids=ids(FWD_PARAMS))
def test_backward_prep(H, case, variant, pool):
    """delta within DOT sum |dO o| of the float64 row sum at every element; dvmean against the float64 sum over the uniform rows"""
    c = context(H, case, variant, pool)
    ref, bound = U.delta_ref(c["do4"], c["o4"])
    U.check_elements(c["delta"], ref, bound, "delta")
    ref, bound = U.dvmean_ref(c["do4"], c["lse"], c["N"])
    U.check_elements(c["dvmean4"], ref, bound, "dvmean", names=("sample", "head", "-", "column"))
    assert bool(torch.isinf(c["lse"]).any()) == bool(c["fwd_ref"]["uniform"].any())


def bwd_ref(c, dq_f32=False):
    key = ("bwd_ref", dq_f32)
    if key not in c:          # (the kernel's own lse, delta and dvmean: every input shared)
        c[key] = U.backward_ref(c["q4"], c["k4"], c["v4"], c["do4"], c["lse"], c["delta"], c["dvmean4"], c["blk"], dq_f32=dq_f32)
    return c[key]


@pytest.mark.parametrize("case,variant,pool", FWD_PARAMS, ids=ids(FWD_PARAMS))
def test_backward_dq(H, case, variant, pool):
    """mca_attn_bwd_dq: bf16 and fp32 dq, element-wise mask and mask product (the same bits), repeatable; a query tile whose live
    list is empty writes zeros over the sentinel"""
    c = context(H, case, variant, pool)
    for f32 in (False, True):
        got = {}
        for hot in (False, True):
            dq = new_dq(c, f32)
            H.call("mca_attn_bwd_dq", C.byref(bwd2_args(H, c, dq, f32, new_dkv(c), 256, hot)), H.stream_ptr())
            torch.cuda.synchronize()
            G.assert_guard_intact(dq, "dq")
            U.check_backward(U.heads4(dq.t, c["b"]), None, None, bwd_ref(c, f32), f"{case} {variant} pool={pool} dq pass (f32={f32}, mask product={hot})",
                             label=f"dq pass {'fp32' if f32 else 'bf16'}")
            got[hot] = dq
        assert same_bits(got[False].t, got[True].t), "the two mask paths differ"
        again = new_dq(c, f32)
        H.call("mca_attn_bwd_dq", C.byref(bwd2_args(H, c, again, f32, new_dkv(c), 256, True)), H.stream_ptr())
        torch.cuda.synchronize()
        assert same_bits(again.t, got[True].t), "a second launch differs"
    if not pool and case == "aligned256":
        assert (got[True].t[:128] == 0).all()          # sample 0, query tile 0: the empty live list


@pytest.mark.parametrize("case,variant,pool", FWD_PARAMS, ids=ids(FWD_PARAMS))
def test_backward_dkv(H, case, variant, pool):
    """mca_attn_bwd_dkv: 256- and 128-key blocks, both mask paths: each per element and row, all four the same bits, repeatable"""
    c = context(H, case, variant, pool)
    got = {}
    for bkeys in (256, 128):
        for hot in (False, True):
            dkv = new_dkv(c)
            H.call("mca_attn_bwd_dkv", C.byref(bwd2_args(H, c, new_dq(c), False, dkv, bkeys, hot)), H.stream_ptr())
            torch.cuda.synchronize()
            dk4, dv4 = dkv_heads(c, dkv)
            U.check_backward(None, dk4, dv4, bwd_ref(c), f"{case} {variant} pool={pool} dkv pass ({bkeys}-key blocks, mask product={hot})",
                             label=f"dkv pass {bkeys}")
            got[bkeys, hot] = dkv
    first = got[256, False]
    for k_, other in got.items():
        assert same_bits(first.t[:, c["D"]:], other.t[:, c["D"]:]), f"dk | dv of the form {k_} differ from the 256-key element-wise form"
    again = new_dkv(c)
    H.call("mca_attn_bwd_dkv", C.byref(bwd2_args(H, c, new_dq(c), False, again, 256, True)), H.stream_ptr())
    torch.cuda.synchronize()
    assert same_bits(again.t[:, c["D"]:], first.t[:, c["D"]:]), "a second launch differs"
    if case == "aligned256":          # sample 0: the dead 128-key block / the dead wavefronts: dK = 0 exactly, dV = dvmean rounded once
        D = c["D"]
        assert (first.t[:128, D:2 * D] == 0).all()
        assert same_bits(first.t[:128, 2 * D:], c["dvmean"][0].to(torch.bfloat16)[None].expand(128, -1))


# ------------------------------------------------------------------------------------------- one-pass backward
def onepass_prep(H, c, sc, slack):
    """mca_attn_bwd_prep_onepass on the tables sc -> dict(rowc, dvmean, q_hm, do_hm buffers); slack: 'zero' or 'randn' behind the
    packed copies.  Checks the row constants (-lse bit for bit, -delta within its bound, -inf | 0 kept past a tile's rows), dvmean
    (the bits of mca_attn_bwd_prep) and the packed copies (bit for bit)."""
    b, N, D, heads = c["b"], c["N"], c["D"], c["heads"]
    nqt = len(sc.s.qt_desc)
    rowc = nan_f32(b, heads, nqt + 1, 2, 64)
    for t, (r0, rn) in enumerate(sc.s.qt_desc.tolist() + [[0, 0]]):          # written once by the caller: past a tile's rows, the null tile
        rowc[:, :, t, 0, rn:] = float("-inf")
        rowc[:, :, t, 1, rn:] = 0.0
    dvmean = nan_f32(b, D)
    rows = b * heads * N
    bufs = []
    for _ in range(2):
        buf = torch.full(((rows + 64) * 64,), float("nan"), dtype=torch.bfloat16, device=DEV)
        if slack == "zero":
            buf[rows * 64:] = 0
        else:
            buf[rows * 64:] = torch.randn(64 * 64, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).to(DEV)
        bufs.append(buf)
    H.call("mca_attn_bwd_prep_onepass", c["o"].data_ptr(), c["do_f"].data_ptr(), c["o_bstride"], c["o_ld"], c["lse"].data_ptr(),
           sc.row_slot.data_ptr(), rowc.data_ptr(), dvmean.data_ptr(), b, heads, N, nqt, c["q_ptr"], c["q_bstride"], c["q_ld"],
           bufs[0].data_ptr(), bufs[1].data_ptr(), H.stream_ptr())
    torch.cuda.synchronize()
    assert same_bits(dvmean, c["dvmean"])
    q_hm, do_hm = (x[:rows * 64].view(b, heads, N, 64) for x in bufs)
    assert same_bits(q_hm, c["qkv"][:, :, :D].reshape(b, N, heads, 64).permute(0, 2, 1, 3))
    assert same_bits(do_hm, c["d_o"].reshape(b, N, heads, 64).permute(0, 2, 1, 3))
    d_ref, d_bound = U.delta_ref(c["do4"], c["o4"])
    delta = torch.empty_like(c["delta"])
    for t, (r0, rn) in enumerate(sc.s.qt_desc.tolist()):
        assert same_bits(rowc[:, :, t, 0, :rn], -c["lse"][:, :, r0:r0 + rn])
        delta[:, :, r0:r0 + rn] = -rowc[:, :, t, 1, :rn]
        assert torch.isinf(rowc[:, :, t, 0, rn:]).all() and (rowc[:, :, t, 1, rn:] == 0).all()
    assert torch.isinf(rowc[:, :, nqt, 0]).all() and (rowc[:, :, nqt, 1] == 0).all()
    U.check_elements(delta, d_ref, d_bound, "delta of the row constants")
    return dict(rowc=rowc, dvmean=dvmean, bufs=bufs, delta=delta, nqt=nqt)


def run_onepass(H, c, sc, prep, packed, split=0):
    b, N, D, heads = c["b"], c["N"], c["D"], c["heads"]
    nqt = prep["nqt"]
    dq, dkv = new_dq(c), new_dkv(c)
    acc = nan_f32(b * heads * max(1, split) * (nqt + 1) * 4096)
    att = c["att"]
    if packed:
        src = [att.RowSource(x.data_ptr(), heads * N * 64, N * 64, 64) for x in prep["bufs"]]
    else:
        src = [att.RowSource(c["q_ptr"], c["q_bstride"], 0, c["q_ld"]), att.RowSource(c["do_f"].data_ptr(), c["o_bstride"], 0, c["o_ld"])]
    grads = att.AttnGrads(c["do_f"], None, dq.data_ptr(), N * (D + WIDER), D + WIDER, False, dkv.t, D, 2 * D, 3 * D + WIDER)
    a1 = att.bwd1_args(c["ops"], grads, c["keys"], sc, prep["rowc"], acc, prep["dvmean"], split, *src)
    H.call("mca_attn_bwd_onepass", C.byref(a1), H.stream_ptr())          # (a refusal raises: at these sizes the tables always fit)
    torch.cuda.synchronize()
    G.assert_guard_intact(dq, "dq")
    return dq, dkv


ONEPASS_PARAMS = [(c, v, al) for c, v in AC.SELF for al in (True, False)]


@pytest.mark.parametrize("case,variant,aligned", ONEPASS_PARAMS, ids=ids(ONEPASS_PARAMS))
def test_backward_onepass(H, case, variant, aligned):
    """mca_attn_bwd_onepass on the structure-aligned and the plain tables: the plain kernel from the strided operands and (knob 9
    bit 64) from the packed copies, the pipelined kernel from the packed copies, split S = 2, 4, 8 (more workgroups than key
    blocks included).  Each per element and row; strided == packed == pipelined bit for bit; split dK / dV == unsplit bit for bit;
    a second launch reproduces the first; the contents of the slack rows behind the packed copies do not matter."""
    c = context(H, case, variant, False)
    att = importlib.import_module("mca-paper_amd.attention")
    sc = att._OnePassSched(AC.onepass_tables(c["st"], aligned), DEV)
    assert sc.fits
    prep = onepass_prep(H, c, sc, "zero")
    ref = U.backward_ref(c["q4"], c["k4"], c["v4"], c["do4"], c["lse"], prep["delta"], c["dvmean4"], c["blk"])
    what = f"{case} {variant} one-pass ({'aligned' if aligned else 'plain'} tables)"

    def checked(dq, dkv, form, label):
        dk4, dv4 = dkv_heads(c, dkv)
        U.check_backward(U.heads4(dq.t, c["b"]), dk4, dv4, ref, f"{what}, {form}", label=label)
        return dq, dkv

    strided = checked(*run_onepass(H, c, sc, prep, packed=False), "plain kernel, strided operands", "one-pass plain")
    piped = checked(*run_onepass(H, c, sc, prep, packed=True), "pipelined kernel, packed copies", "one-pass pipelined")
    H.lib().mca_debug_set(9, 64)
    try:
        plain_packed = checked(*run_onepass(H, c, sc, prep, packed=True), "plain kernel, packed copies", "one-pass plain")
    finally:
        H.lib().mca_debug_set(9, 0)
    for name, other in (("pipelined / packed", piped), ("plain / packed", plain_packed)):
        assert same_bits(strided[0].t, other[0].t) and same_bits(strided[1].t, other[1].t), f"{name} differs from plain / strided"
    again = run_onepass(H, c, sc, prep, packed=True)
    assert same_bits(again[0].t, piped[0].t) and same_bits(again[1].t, piped[1].t), "a second launch differs"
    # ---- split mode
    for S in AC.SPLITS:
        dq, dkv = checked(*run_onepass(H, c, sc, prep, packed=True, split=S), f"split {S} ({sc.n_kb} key blocks)", "one-pass split")
        assert same_bits(dkv.t[:, c["D"]:], piped[1].t[:, c["D"]:]), f"split {S}: dK / dV differ from the unsplit kernel"
        dq_b, dkv_b = run_onepass(H, c, sc, prep, packed=True, split=S)
        assert same_bits(dq_b.t, dq.t) and same_bits(dkv_b.t, dkv.t), f"split {S}: a second launch differs"
    # ---- the 64 slack rows behind the packed copies: finite values of ordinary magnitude, contents irrelevant
    prep_r = onepass_prep(H, c, sc, "randn")
    assert same_bits(prep_r["rowc"], prep["rowc"])
    slack = run_onepass(H, c, sc, prep_r, packed=True)
    assert same_bits(slack[0].t, piped[0].t) and same_bits(slack[1].t, piped[1].t), "the results depend on the slack rows' contents"
