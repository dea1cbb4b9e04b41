"""The argument structs of the attention launches as attention.py's builders fill them, checked without a GPU on CPU tensors:
every field of AttnFwdArgs, AttnBwd2Args, AttnBwd1Args and AttnReadoutArgs against a value written down here, for a layer
attention (q | k | v in one matrix, mask product) and a pooling attention (one q for every sample, element-wise mask, fp32 dq),
all operands with leading dimensions wider than their data.  A field of a struct is either set to a non-zero value by its
builder in one of these cases or named in that case's LEFT_ZERO list: a field added to hip.py and forgotten in the builder fails."""
import importlib

import pytest
import torch

A = importlib.import_module("mca-paper_amd.attention")
H = importlib.import_module("mca-paper_amd.hip")
S = importlib.import_module("mca-paper_amd.structure")

B, HEADS, D, WIDER = 2, 2, 128, 8
ST = S.FusionStructure([5, 3, 2], 4, (3, 2), fcl=True)
N, R, NK_PAD = 14, len(ST.qmask_pool), 256
FLAGS = H.ATTN_Q_PRESCALED | H.ATTN_LAZY_REFERENCE


def wide(rows, cols, dtype=torch.bfloat16):
    """a (rows, cols) view of a matrix whose rows are WIDER elements longer"""
    return torch.zeros(rows, cols + WIDER, dtype=dtype)[:, :cols]


def i32(*shape):
    return torch.zeros(*shape, dtype=torch.int32)


@pytest.fixture(scope="module")
def case():
    assert ST.n_tokens == N and R > 0
    c = dict(keyinfo=torch.zeros(B, NK_PAD, dtype=torch.uint8), kflags=torch.zeros(B, 1, dtype=torch.uint8),
             khot=torch.zeros(B, NK_PAD, 16, dtype=torch.bfloat16), vmean=torch.zeros(B, D), dvmean=torch.zeros(B, D),
             sf=A._Sched(ST.attn_schedule(128, 64), "cpu"), sb={bk: A._Sched(ST.attn_schedule(64, bk), "cpu") for bk in (128, 256)},
             pf=A._Sched(ST.pool_schedule(128, 64), "cpu"), pb=A._Sched(ST.pool_schedule(64, 256), "cpu"),
             one=A._OnePassSched(ST.attn_onepass_schedule(aligned=True), "cpu"))
    # layer attention: q | k | v and dq | dk | dv are the column blocks of (b * N, 3 D) matrices
    c["qkv"], c["dqkv"], c["o"], c["do"] = wide(B * N, 3 * D), wide(B * N, 3 * D), wide(B * N, D), wide(B * N, D)
    c["lse"], c["delta"], c["qmask"], c["qblk"] = torch.zeros(B, HEADS, N), torch.zeros(B, HEADS, N), i32(N), torch.zeros(N, 16, dtype=torch.bfloat16)
    ld3, ld1 = 3 * D + WIDER, D + WIDER
    c["layer"] = (A.AttnOperands(c["qkv"].data_ptr(), N * ld3, ld3, c["qkv"], D, 2 * D, ld3, c["o"], c["lse"], N, c["qmask"], c["qblk"],
                                 c["sf"], c["sb"][128], 0),
                  A.AttnGrads(c["do"], c["delta"], c["dqkv"].data_ptr(), N * ld3, ld3, False, c["dqkv"], D, 2 * D, ld3))
    # pooling attention: one (R, D) q, k | v packed as (b * N, 2 D), fp32 dq
    c["qp"], c["kvp"], c["dkvp"], c["op"], c["dop"] = wide(R, D), wide(B * N, 2 * D), wide(B * N, 2 * D), wide(B * R, D), wide(B * R, D)
    c["dqp"], c["lse_p"], c["delta_p"] = wide(B * R, D, torch.float32), torch.zeros(B, HEADS, R), torch.zeros(B, HEADS, R)
    c["qmask_p"], c["qblk_p"] = i32(R), torch.zeros(R, 16, dtype=torch.bfloat16)
    ld2 = 2 * D + WIDER
    c["pool"] = (A.AttnOperands(c["qp"].data_ptr(), 0, ld1, c["kvp"], 0, D, ld2, c["op"], c["lse_p"], R, c["qmask_p"], c["qblk_p"], c["pf"],
                                c["pb"], None),
                 A.AttnGrads(c["dop"], c["delta_p"], c["dqp"].data_ptr(), R * ld1, ld1, True, c["dkvp"], 0, D, ld2))
    c["hot"] = A.AttnKeys(c["keyinfo"], c["kflags"], c["khot"], N, NK_PAD, B, HEADS, 0.125, FLAGS)
    c["plain"] = c["hot"]._replace(khot=None)
    return c


def check(a, want, left_zero):
    names = [f for f, _ in a._fields_]
    assert sorted(list(want) + list(left_zero)) == sorted(names), "every field is either expected non-zero or listed as left zero"
    for f in names:
        got = getattr(a, f) or 0          # (a null pointer reads as None)
        if f in left_zero:
            assert got == 0, f"{type(a).__name__}.{f} = {got}, expected untouched"
        else:
            assert want[f] != 0 and got == want[f], f"{type(a).__name__}.{f} = {got}, expected {want[f]}"


def P(t, byte_off=0):
    return t.data_ptr() + byte_off


def test_builders_touch_neither_gpu_nor_library(case, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a builder loaded the library")
    monkeypatch.setattr(H, "lib", refuse)
    ops, grads = case["layer"]
    A.fwd_args(ops, case["hot"], case["vmean"])
    A.bwd2_args(ops, grads, case["hot"], case["dvmean"])
    A.readout_args(ops, case["hot"], torch.zeros(3), torch.zeros(3))


def test_forward_args(case):
    c, ld3, ld2, ld1 = case, 3 * D + WIDER, 2 * D + WIDER, D + WIDER
    sf, pf = c["sf"], c["pf"]
    check(A.fwd_args(c["layer"][0], c["hot"], c["vmean"]),
          dict(q=P(c["qkv"]), q_bstride=N * ld3, q_ld=ld3, k=P(c["qkv"], 2 * D), v=P(c["qkv"], 4 * D), kv_bstride=N * ld3, kv_ld=ld3,
               o=P(c["o"]), o_bstride=N * ld1, o_ld=ld1, lse=P(c["lse"]), qmask=P(c["qmask"]), keyinfo=P(c["keyinfo"]), ktile_flags=P(c["kflags"]),
               q_ptr=P(sf.q_ptr), q_kt=P(sf.q_kt), q_order=P(sf.q_order), vmean=P(c["vmean"]), batch=B, heads=HEADS, nq=N, nk=N, nk_pad=NK_PAD,
               n_qtiles=1, n_ktiles=1, scale=0.125, flags=FLAGS, khot=P(c["khot"])), [])
    check(A.fwd_args(c["pool"][0], c["plain"], c["vmean"]),
          dict(q=P(c["qp"]), q_ld=ld1, k=P(c["kvp"]), v=P(c["kvp"], 2 * D), kv_bstride=N * ld2, kv_ld=ld2,
               o=P(c["op"]), o_bstride=R * ld1, o_ld=ld1, lse=P(c["lse_p"]), qmask=P(c["qmask_p"]), keyinfo=P(c["keyinfo"]), ktile_flags=P(c["kflags"]),
               q_ptr=P(pf.q_ptr), q_kt=P(pf.q_kt), q_order=P(pf.q_order), vmean=P(c["vmean"]), batch=B, heads=HEADS, nq=R, nk=N, nk_pad=NK_PAD,
               n_qtiles=-(-R // 128), n_ktiles=1, scale=0.125, flags=FLAGS), ["q_bstride", "khot"])


def test_twopass_backward_args(case):
    c, ld3, ld2, ld1 = case, 3 * D + WIDER, 2 * D + WIDER, D + WIDER
    sf, pf, pb = c["sf"], c["pf"], c["pb"]
    layer = dict(q=P(c["qkv"]), q_bstride=N * ld3, q_ld=ld3, k=P(c["qkv"], 2 * D), v=P(c["qkv"], 4 * D), kv_bstride=N * ld3, kv_ld=ld3,
                 d_o=P(c["do"]), o_bstride=N * ld1, o_ld=ld1, lse=P(c["lse"]), delta=P(c["delta"]), dvmean=P(c["dvmean"]),
                 dq=P(c["dqkv"]), dq_bstride=N * ld3, dq_ld=ld3, dk=P(c["dqkv"], 2 * D), dv=P(c["dqkv"], 4 * D), dkv_bstride=N * ld3, dkv_ld=ld3,
                 qmask=P(c["qmask"]), keyinfo=P(c["keyinfo"]), ktile_flags=P(c["kflags"]), q_ptr=P(sf.q_ptr), q_kt=P(sf.q_kt), q_order=P(sf.q_order),
                 n_qtiles128=1, n_ktiles64=1, n_qtiles64=1, n_kblocks256=1, batch=B, heads=HEADS, nq=N, nk=N, nk_pad=NK_PAD, scale=0.125,
                 flags=FLAGS, khot=P(c["khot"]), qblk=P(c["qblk"]))
    # the operands' own dkv schedule (128-key blocks), then another one handed in (256-key blocks)
    for sched_b, bk in ((None, 128), (c["sb"][256], 256)):
        sb = c["sb"][bk]
        check(A.bwd2_args(*c["layer"], c["hot"], c["dvmean"], sched_b), dict(layer, k_wg=P(sb.k_wg), k_qt=P(sb.k_qt), kblock_keys=bk), ["dq_f32"])
    check(A.bwd2_args(*c["pool"], c["plain"], c["dvmean"]),
          dict(q=P(c["qp"]), q_ld=ld1, k=P(c["kvp"]), v=P(c["kvp"], 2 * D), kv_bstride=N * ld2, kv_ld=ld2,
               d_o=P(c["dop"]), o_bstride=R * ld1, o_ld=ld1, lse=P(c["lse_p"]), delta=P(c["delta_p"]), dvmean=P(c["dvmean"]),
               dq=P(c["dqp"]), dq_bstride=R * ld1, dq_ld=ld1, dq_f32=1, dk=P(c["dkvp"]), dv=P(c["dkvp"], 2 * D), dkv_bstride=N * ld2, dkv_ld=ld2,
               qmask=P(c["qmask_p"]), keyinfo=P(c["keyinfo"]), ktile_flags=P(c["kflags"]), q_ptr=P(pf.q_ptr), q_kt=P(pf.q_kt), q_order=P(pf.q_order),
               n_qtiles128=-(-R // 128), n_ktiles64=1, k_wg=P(pb.k_wg), k_qt=P(pb.k_qt), n_qtiles64=-(-R // 64), n_kblocks256=1,
               batch=B, heads=HEADS, nq=R, nk=N, nk_pad=NK_PAD, scale=0.125, flags=FLAGS, kblock_keys=256), ["q_bstride", "khot", "qblk"])


def test_onepass_backward_args(case):
    c, ld3, ld1, one = case, 3 * D + WIDER, D + WIDER, case["one"]
    rowc, acc = torch.zeros(B, HEADS, one.n_qt + 1, 2, 64), torch.zeros(B * HEADS * 2 * (one.n_qt + 1) * 4096)
    q_hm, do_hm = torch.zeros(B, HEADS, N, 64, dtype=torch.bfloat16), torch.zeros(B, HEADS, N, 64, dtype=torch.bfloat16)
    s = ST.attn_onepass_schedule(aligned=True)
    want = dict(k=P(c["qkv"], 2 * D), v=P(c["qkv"], 4 * D), kv_bstride=N * ld3, kv_ld=ld3, rowc=P(rowc), dvmean=P(c["dvmean"]),
                dq=P(c["dqkv"]), dq_bstride=N * ld3, dq_ld=ld3, dk=P(c["dqkv"], 2 * D), dv=P(c["dqkv"], 4 * D), dkv_bstride=N * ld3, dkv_ld=ld3,
                dq_acc=P(acc), keyinfo=P(c["keyinfo"]), ktile_flags=P(c["kflags"]), khot=P(c["khot"]), qblk=P(c["qblk"]),
                qt_desc=P(one.qt_desc), kb_desc=P(one.kb_desc), kb_qt=P(one.kb_qt), visit=P(one.visit),
                n_qtiles=len(s.qt_desc), n_kblocks=len(s.kb_desc), max_list=int(s.kb_desc[:, 3].max()), n_entries=len(s.kb_qt),
                batch=B, heads=HEADS, n=N, nk_pad=NK_PAD, n_ktiles64=1, scale=0.125, flags=FLAGS)
    # from the packed head-major copies, key blocks split two ways
    a = A.bwd1_args(*c["layer"], c["hot"], one, rowc, acc, c["dvmean"], 2, A.RowSource(P(q_hm), HEADS * N * 64, N * 64, 64),
                    A.RowSource(P(do_hm), HEADS * N * 64, N * 64, 64))
    check(a, dict(want, q=P(q_hm), q_bstride=HEADS * N * 64, q_hstride=N * 64, q_ld=64, d_o=P(do_hm), o_bstride=HEADS * N * 64, o_hstride=N * 64,
                  o_ld=64, split=2), [])
    # from the row-major matrices, one workgroup per (sample, head)
    a = A.bwd1_args(*c["layer"], c["hot"], one, rowc, acc, c["dvmean"], 0, A.RowSource(P(c["qkv"]), N * ld3, 0, ld3), A.RowSource(P(c["do"]), N * ld1, 0, ld1))
    check(a, dict(want, q=P(c["qkv"]), q_bstride=N * ld3, q_ld=ld3, d_o=P(c["do"]), o_bstride=N * ld1, o_ld=ld1), ["q_hstride", "o_hstride", "split"])


def test_readout_args(case):
    c, ld3, ld2, ld1 = case, 3 * D + WIDER, 2 * D + WIDER, D + WIDER
    sf, pf = c["sf"], c["pf"]
    um, mass, probs, lse2 = torch.zeros(ST.n_groups), torch.zeros(B, HEADS, N, ST.n_groups), torch.zeros(B, HEADS, 3, N), torch.zeros(B, HEADS, N)
    # (the lazy-reference bit is the forward's business: the readout takes the pre-scaled flag alone)
    check(A.readout_args(c["layer"][0]._replace(lse=lse2), c["hot"], um, mass, probs, 1),
          dict(q=P(c["qkv"]), q_bstride=N * ld3, q_ld=ld3, k=P(c["qkv"], 2 * D), kv_bstride=N * ld3, kv_ld=ld3, lse=P(lse2), qmask=P(c["qmask"]),
               keyinfo=P(c["keyinfo"]), ktile_flags=P(c["kflags"]), q_ptr=P(sf.q_ptr), q_kt=P(sf.q_kt), q_order=P(sf.q_order),
               batch=B, heads=HEADS, nq=N, nk=N, nk_pad=NK_PAD, n_qtiles=1, n_ktiles=1, scale=0.125, flags=H.ATTN_Q_PRESCALED,
               n_groups=ST.n_groups, uniform_mass=P(um), mass=P(mass), probs=P(probs), row0=1, n_rows=3), [])
    check(A.readout_args(c["pool"][0], c["plain"], um, mass),
          dict(q=P(c["qp"]), q_ld=ld1, k=P(c["kvp"]), kv_bstride=N * ld2, kv_ld=ld2, lse=P(c["lse_p"]), qmask=P(c["qmask_p"]),
               keyinfo=P(c["keyinfo"]), ktile_flags=P(c["kflags"]), q_ptr=P(pf.q_ptr), q_kt=P(pf.q_kt), q_order=P(pf.q_order),
               batch=B, heads=HEADS, nq=R, nk=N, nk_pad=NK_PAD, n_qtiles=-(-R // 128), n_ktiles=1, scale=0.125, flags=H.ATTN_Q_PRESCALED,
               n_groups=ST.n_groups, uniform_mass=P(um), mass=P(mass)), ["q_bstride", "probs", "row0", "n_rows"])
