"""mca_contrastive_stream_fwd_bwd (csrc/loss_stream.hip), what can be shown without a GPU (tests/loss_stream_util.py,
tests/loss_stream_cases.py):
(a) the tile constants of the case list are the library's, the workspace is the stated layout and at least eight times smaller than
    the dense kernel's at B = 8192, and the argument errors come back with nothing launched;
(b) every listed case reaches the path it is listed for, by the formulas of the launch code;
(c) the checker raises on planted faults of the streaming structure;
(d) every derived bound is satisfiable: an fp32 torch restatement of the three kernels in their summation grouping passes the very
    checker the GPU test runs, at every element of every case and rank."""
import ctypes as C
import importlib

import pytest
import torch

import loss_cases as LC
import loss_edge_util as U
import loss_stream_cases as SC
import loss_stream_util as SU

CASE = {c["name"]: (i, c) for i, c in enumerate(SC.CASES)}
BADARG, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def H():
    importlib.import_module("mca-paper_amd.build").build()
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


# ------------------------------------------------------------------------------------------------ (a) constants, workspace, refusals
def test_tile_constants_are_the_librarys(H):
    lay = H.contrastive_stream_layout(17, 3)
    assert (lay["TI"], lay["TJ"], lay["TK"], lay["DMAX"]) == (SC.TI, SC.TJ, SC.TK, SC.DMAX)
    assert SC.TJ % 32 == 0 and SC.TJ // 32 * 2 == SC.LANES


@pytest.mark.parametrize("B,T", [(1, 1), (17, 3), (100, 50), (8192, 14), (16384, 60)])
def test_workspace_layout(H, B, T):
    lay = H.contrastive_stream_layout(B, T)
    tb = T * B * 4
    assert lay["lse"] == (0, 2 * tb) and lay["erat"] == (2 * tb, 2 * tb) and lay["diag"] == (4 * tb, tb)
    assert lay["red"] == (5 * tb, 3 * tb) and lay["w"] == (8 * tb, tb)
    assert H.lib().mca_contrastive_stream_workspace_bytes(B, T, 15, 512) == 9 * tb + 256
    assert H.lib().mca_dbg_contrastive_stream_layout(B, T, None) == BADARG
    assert H.lib().mca_dbg_contrastive_stream_layout(0, T, (C.c_int64 * 14)()) == BADARG


def test_workspace_is_no_matrix(H):
    """per-row statistics only: an eighth of the dense kernel's workspace, or less, at the size the cached step is for"""
    lib = H.lib()
    assert lib.mca_contrastive_stream_workspace_bytes(8192, 14, 15, 512) * 8 <= lib.mca_contrastive_workspace_bytes(8192, 14)
    assert lib.mca_contrastive_stream_workspace_bytes(16384, 60, 15, 512) < 2 ** 27          # the dense kernel: 64 GB


def _args(H, **over):
    """a valid call's arguments with fake non-null pointers: every refusal below returns before anything is launched or read"""
    B, T, R, D = 6, 3, 3, 7
    a = dict(pooled=64, present=64, terms=64, T=T, s=64, B=B, b_local=2, row0=0, R=R, D=D, term_loss=64, loss=64, d_pooled=64, dls=64, ws=64,
             ws_bytes=None)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = H.lib().mca_contrastive_stream_workspace_bytes(max(a["B"], 1), max(a["T"], 1), max(a["R"], 1), max(a["D"], 1))
    return tuple(a.values()) + (None,)


def test_argument_refusals(H):
    f = H.lib().mca_contrastive_stream_fwd_bwd
    bad = [dict(b_local=4), dict(row0=1), dict(row0=3), dict(row0=6), dict(row0=-2), dict(b_local=0), dict(T=0), dict(B=0), dict(R=0), dict(D=0)]
    bad += [{k: None} for k in ("pooled", "present", "terms", "s", "term_loss", "loss", "d_pooled", "dls", "ws")]
    for over in bad:
        assert f(*_args(H, **over)) == BADARG, over
    need = H.lib().mca_contrastive_stream_workspace_bytes(6, 3, 3, 7)
    assert f(*_args(H, ws_bytes=need - 1)) == BADARG and f(*_args(H, ws_bytes=0)) == BADARG
    assert f(*_args(H, D=SC.DMAX + 1)) == UNSUPPORTED and f(*_args(H, D=1024)) == UNSUPPORTED
    assert f(*_args(H, D=SC.DMAX + 1, ws_bytes=8)) == BADARG          # the workspace is judged first


# ------------------------------------------------------------------------------------------------ (b) the paths of the listed cases
def _T(c):
    return c["T"] if c["T"] is not None else len(U.schedule_terms(c["terms"].split(":")[1])[0])


def test_cases_reach_their_paths():
    TI, TJ, TK = SC.TI, SC.TJ, SC.TK
    P = {c["name"]: SC.paths(c, _T(c)) for c in SC.CASES}
    fam = lambda f: [c for c in SC.CASES if c["family"] == f]
    tiles = fam("tiles")
    assert all(p["accepted"] for p in P.values())
    assert {c["B"] for c in tiles} == {1, TI - 1, TI, TI + 1, 2 * TI + 1, TJ - 1, TJ, TJ + 1, 2 * TJ + 1}
    assert {(c["B"], P[c["name"]]["strips"], P[c["name"]]["strip_tail"]) for c in tiles} >= {(1, 1, 1), (TI - 1, 1, TI - 1), (TI, 1, 0), (TI + 1, 2, 1), (2 * TI + 1, 3, 1)}
    assert {(c["B"], P[c["name"]]["tiles"], P[c["name"]]["tile_tail"]) for c in tiles} >= {(1, 1, 1), (TJ - 1, 1, TJ - 1), (TJ, 1, 0), (TJ + 1, 2, 1), (2 * TJ + 1, 3, 1)}
    assert {(c["D"], P[c["name"]]["k_trips"], P[c["name"]]["k_tail"]) for c in tiles} == {(1, 1, 1), (TK - 1, 1, TK - 1), (TK, 1, 0), (TK + 1, 2, 1), (130, 5, 2)}
    for B in {c["B"] for c in tiles}:
        for D in {c["D"] for c in tiles}:
            kinds = {c["kind"] for c in tiles if (c["B"], c["D"]) == (B, D)}
            assert "exact" in kinds and kinds & {"prod3", "prod4"}
        bl = {c["b_local"] for c in tiles if c["B"] == B}
        assert bl == ({B, B // 3} if B % 3 == 0 else {B})
    # a rank whose first row is no multiple of a strip, with more than one strip of its own
    assert any(not P[c["name"]]["row0_aligned"] and P[c["name"]]["grad_strips"] > 1 and P[c["name"]]["W"] == 3 for c in tiles)
    assert {(c["D"], P[c["name"]]["waves_with_columns"], P[c["name"]]["subtiles"]) for c in fam("width")} == {(128, 1, 4), (512, 4, 16)}
    assert {P[c["name"]]["waves_with_columns"] for c in tiles} == {1, 2}
    sa, sb = {t[0] for t in LC.TERMS_DPOOLED}, {t[1] for t in LC.TERMS_DPOOLED}
    assert 1 in sa and 1 in sb and any(t[0] == t[1] for t in LC.TERMS_DPOOLED) and 3 not in sa | sb and all(c["R"] == 4 for c in fam("slots"))
    assert {P[c["name"]]["tiles"] for c in fam("slots")} == {1, 2} and {c["kind"] for c in fam("slots")} == {"exact", "prod3", "prod4"}
    for c in fam("reduce"):
        assert c["T"] == 60 and c["present"] is LC.P60
    assert {P[c["name"]]["W"] for c in fam("reduce")} == {1, 5} and {P[c["name"]]["W"] for c in fam("ranks")} == {1, 2, 3}
    for c in fam("manyranks"):
        assert P[c["name"]]["dense_lds_bytes"] > LC.LDS_LIMIT and P[c["name"]]["W"] == c["B"]
    assert {c["terms"] for c in fam("schedule")} == {"schedule:mca", "schedule:bimodal", "schedule:zorro"}
    terms, R = SC.cmu_terms()
    assert len(terms) == 14 and R == 16 and {s for t in terms for s in t[:2]} == set(range(15))          # 15 slots named, the global token's not


# ------------------------------------------------------------------------------------------------ (c) planted faults
def _prepared(name):
    i, c = CASE[name]
    d = SU.make_data(c, i)
    return d, SU.reference(d)


def test_checker_sees_a_missing_rescale():
    """two tiles of production-magnitude logits: a lane whose running maximum rises must rescale what it has summed"""
    name = next(c["name"] for c in SC.CASES if c["family"] == "tiles" and c["B"] == 2 * SC.TJ + 1 and c["D"] == SC.TK + 1 and c["kind"] != "exact")
    d, ref = _prepared(name)
    SU.check(d, ref, 0, SU.emulate(d, 0))
    with pytest.raises(AssertionError, match=r"(lse|E / S): \d+ of \d+ elements wrong; first: direction \d, term \d, row \d+"):
        SU.check(d, ref, 0, SU.emulate(d, 0, drop_rescale=True))


def test_checker_sees_a_dropped_direction():
    """slot 1 is slot_b of term 0 and slot_a of term 1: without term 0's column direction it holds term 1's share only"""
    d, ref = _prepared("slots-B5D33R4b5-prod3")
    with pytest.raises(AssertionError, match=r"d_pooled: \d+ of \d+ elements wrong; first: row \d+, slot 1, column \d+"):
        SU.check(d, ref, 0, SU.emulate(d, 0, skip_dir1_of=0))


def test_checker_sees_a_stale_unused_slot_and_a_wrong_nan():
    d, ref = _prepared("slots-B5D33R4b5-prod3")
    o = SU.emulate(d, 0)
    SU.check(d, ref, 0, o)
    o["d_pooled"][:, 3].view(torch.int32).fill_(-1)
    with pytest.raises(AssertionError, match=r"slot 3, which no term names"):
        SU.check(d, ref, 0, o)
    d, ref = _prepared("ranks-B6D7R3b2-exact")
    o = SU.emulate(d, 0)
    SU.check(d, ref, 0, o)
    o["term_loss"].view(torch.int32)[0] = 0x7FC00001
    with pytest.raises(AssertionError, match="quiet NaN"):
        SU.check(d, ref, 0, o)


# ------------------------------------------------------------------------------------------------ (d) every bound is satisfiable
@pytest.mark.parametrize("name", list(CASE))
def test_emulation_within_bounds(name):
    d, ref = _prepared(name)
    common = SU.emulate_common(d)
    for r in range(d["W"]):
        SU.check(d, ref, r, SU.emulate(d, r, common), common=r == 0)


def test_worst_ratios_below_one():
    """after test_emulation_within_bounds (pytest -s shows the ratios)"""
    seen = {k: v for k, v in SU.WORST.items() if k.startswith("stream ")}
    for k in sorted(seen):
        print(f"worst |emulation - ref| / bound  {k:24s} {seen[k]:.3f}")
    assert seen and all(v < 1 for v in seen.values())
