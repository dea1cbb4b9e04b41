"""The token-table edge tests, checked without a GPU (tests/token_edge_util.py, tests/token_cases.py):
(a) the grid and the pass counts every listed case reaches in each of its launches equal the numbers written down, and every
    constant's boundary (wave_grid's 2048 workgroups, RENORM_CHUNK, the 64-lane and 64-float4 loops, the sort's 256 tile, the 64-column
    chunks of the sum) is reached by at least one case on either side;
(b) every derived bound is satisfiable: fp32 restatements of the renormalisation, the gather composition and both sum orders,
    stored where the kernels store, pass the very checks the GPU tests run, at every element of every case;
(c) the near-threshold rows keep their 2^-10 distance and the exactly-at rows have an fp32 norm equal to max_norm;
(d) the helpers raise and name the first (row, column) of each planted fault;
and the refusals, which need no launch."""
import importlib

import pytest
import torch

import token_cases as TC
import token_edge_util as U


def ids(cases):
    return [c["name"] for c in cases]


def by_name(cases, name):
    return next(c for c in cases if c["name"] == name)


def emulate_lookup(fault=None):
    return lambda case, T: U.lookup_emulate_into(case, T, fault)


def emulate_grad(fault=None):
    return lambda case, T, O, det, ib: U.grad_emulate_into(case, T, O, det, fault)


# ------------------------------------------------------------------------------------------------ (a) plans
def test_literal_plans():
    for (vocab, cols, tokens), want in TC.LOOKUP_LITERAL:
        assert TC.lookup_plan(vocab, cols, tokens) == want, (vocab, cols, tokens)
    for (vocab, cols, tokens), want in TC.GRAD_LITERAL:
        assert TC.grad_plan(vocab, cols, tokens) == want, (vocab, cols, tokens)
    shapes = {(c["vocab"], c["cols"], c["tokens"]) for c in TC.LOOKUP}
    assert {(33, 4, 8197), (131089, 4, 10), (33, 4, 524293), (33, 260, 33), (33, 1024, 33)} <= shapes          # the literals are cases
    shapes = {(c["vocab"], c["cols"], c["tokens"]) for c in TC.GRAD}
    assert {(37, 1024, 600), (37, 4, 8197), (37, 65, 257), (1, 129, 513), (37, 1024, 513)} <= shapes
    assert len({c["name"] for c in TC.LOOKUP}) == len(TC.LOOKUP) and len({c["name"] for c in TC.GRAD}) == len(TC.GRAD)


def test_every_boundary_is_reached_on_both_sides():
    L, G = [c["plan"] for c in TC.LOOKUP], [c["plan"] for c in TC.GRAD]
    for launch in ("mark", "renorm", "gather"):          # wave_grid's cap: one pass and a second one
        assert {min(p[launch][1], 2) for p in L} == {1, 2}, launch
        assert any(p[launch][0] == TC.GRID_CAP for p in L) and any(p[launch][0] < TC.GRID_CAP for p in L), launch
    assert {min(p["scatter"][1], 2) for p in G} == {1, 2} and {min(p["sum"][2], 2) for p in G} == {1, 2}
    # the second pass of each loop ends in a partial trip: 5 tokens, 17 table rows
    assert by_name(TC.LOOKUP, "gather-second-pass")["tokens"] % (TC.GRID_CAP * TC.WAVES) == 5
    assert by_name(TC.LOOKUP, "renorm-second-pass")["vocab"] % (TC.GRID_CAP * TC.WAVES * TC.RENORM_CHUNK) == 17
    assert by_name(TC.LOOKUP, "mark-second-pass")["tokens"] % (TC.GRID_CAP * TC.BLOCK) == 5
    # RENORM_CHUNK: a table inside one chunk, exactly one, one more
    assert {15, 16, 17} <= {c["vocab"] for c in TC.LOOKUP}
    # the lane loops: 64 columns (renormalise), 64 float4 (gather)
    assert {p["lane_passes"][0] for p in L} >= {1, 2, 4, 5, 16} and {p["lane_passes"][1] for p in L} >= {1, 2, 4}
    assert {60, 64, 68, 256, 260} <= {c["cols"] for c in TC.LOOKUP}
    # the sort's tile and the sum's chunks, the partial last chunk on both sides of a full one
    assert {1, 255, 256, 257, 513} <= {c["tokens"] for c in TC.GRAD} and {p["sort"][1] for p in G} >= {1, 2, 3, 33}
    assert {(p["chunks"], p["partial_chunk"]) for p in G} >= {(1, 1), (1, 0), (2, 1), (2, 0), (3, 1), (16, 0)}
    # leading dimensions, periods, a partial last group, every padding_idx form, every (add, accumulate) with and without an index out of range
    assert {c["ldd"] - c["cols"] for c in TC.LOOKUP} == {0, 4} and {c["ldy"] - c["cols"] for c in TC.GRAD} == {0, 3}
    for cases in (TC.LOOKUP, TC.GRAD):
        assert any(c["period"] == 1 for c in cases) and any(c["period"] == c["tokens"] > 1 for c in cases)
        assert any(c["period"] == 7 and c["tokens"] > 7 and c["tokens"] % 7 for c in cases)
    assert {(c["add"], c["acc"], c["oob"]) for c in TC.LOOKUP} == {(a, b, o) for a, b in TC.COMBOS for o in (0, 1)}
    assert {c["idx_bytes"] for c in TC.LOOKUP} == {4, 8} and {c["max_norm"] for c in TC.LOOKUP} == set(TC.MAX_NORMS)
    for v in (1, 37):
        assert {c["padding_idx"] for c in TC.GRAD if c["vocab"] == v} >= {0, 5, -1, v}
    assert {c["pattern"] for c in TC.GRAD} >= set(TC.G_PATTERNS) and {c["pattern"] for c in TC.LOOKUP} >= set(TC.L_PATTERNS)
    assert sum(c["pattern"] == "distinct" and c["tokens"] <= c["vocab"] and c["tokens"] > 1 for c in TC.LOOKUP) >= 3


def test_index_patterns_are_what_they_say():
    for c in TC.LOOKUP:
        idx = U.lookup_indices(c)
        bad = (idx < 0) | (idx >= c["vocab"])
        assert bool(bad.any()) == bool(c["oob"]), c["name"]
        if c["pattern"] == "distinct" and c["tokens"] <= c["vocab"]:
            assert len(idx.unique()) == c["tokens"]
    c = by_name(TC.LOOKUP, "mark-second-pass")
    idx = U.lookup_indices(c)
    first_pass = TC.GRID_CAP * TC.BLOCK
    assert ((idx[:first_pass] >= 0) & (idx[:first_pass] < c["vocab"])).all() and (idx[first_pass:] >= c["vocab"]).sum() == 1
    c = by_name(TC.LOOKUP, "renorm-second-pass")
    idx, b = U.lookup_indices(c), TC.GRID_CAP * TC.WAVES * TC.RENORM_CHUNK
    big = U.norm_class(c["vocab"], c["cls0"])[idx] == 0
    assert (idx[big] < b).any() and (idx[big] >= b).any() and {b - 1, b, c["vocab"] - 1, 0} <= set(idx.tolist())
    c = by_name(TC.LOOKUP, "two-lookups")
    a, s = U.lookup_indices(c), U.lookup_indices(c, "second")
    cls = U.norm_class(c["vocab"], c["cls0"])
    assert not torch.equal(a, s) and len(set(a.tolist()) & set(s.tolist())) > 0 and len(set(s.tolist()) - set(a.tolist())) > 0
    assert not any(int(cls[r]) in (0, 2) for r in set(a.tolist()) & set(s.tolist()))
    for c in TC.GRAD:
        idx = U.grad_indices(c)
        if c["pattern"] in ("distinct", "strict-descending"):
            assert len(idx.unique()) == c["tokens"]
        if c["pattern"] in ("descending", "strict-descending"):
            assert (idx[1:] <= idx[:-1]).all() and (c["tokens"] == 1 or c["vocab"] == 1 or idx[0] > idx[-1])
        if c["pattern"] == "alloob":
            assert ((idx < 0) | (idx >= c["vocab"])).all()
    c = by_name(TC.GRAD, "strictly-descending-257")
    assert (U.grad_indices(c).diff() < 0).all()


# ------------------------------------------------------------------------------------------------ (c) the table's norm classes
@pytest.mark.parametrize("max_norm", TC.MAX_NORMS)
@pytest.mark.parametrize("cols", [4, 60, 1024])
def test_norm_classes(max_norm, cols):
    w = U.make_table(33, cols, max_norm, 1, U.gen(5))
    U.assert_table_classes(w, max_norm, 1)
    assert float(torch.tensor(max_norm, dtype=torch.float32) ** 2) == max_norm ** 2          # exact in fp32
    # fp32 and float64 decide alike on every row, the near ones included
    n32, n64 = torch.sqrt((w * w).sum(1)), w.double().norm(dim=1)
    assert torch.equal(n32 > max_norm, n64 > max_norm)


def test_every_case_table_keeps_its_classes():
    for c in TC.LOOKUP:
        if c["vocab"] <= 33:
            U.assert_table_classes(U.make_table(c["vocab"], c["cols"], c["max_norm"], c["cls0"], U.gen(7)), c["max_norm"], c["cls0"])


# ------------------------------------------------------------------------------------------------ (b) the bounds are satisfiable
@pytest.mark.parametrize("case", TC.LOOKUP, ids=ids(TC.LOOKUP))
def test_lookup_bounds_satisfiable(case):
    U.lookup_case(case, "cpu", emulate_lookup())


@pytest.mark.parametrize("case", TC.GRAD, ids=ids(TC.GRAD))
def test_grad_bounds_satisfiable(case):
    U.grad_case(case, "cpu", emulate_grad())


def test_operands_sit_where_the_cases_say():
    case = by_name(TC.LOOKUP, "oob-68x10-a1c1-i32")
    T = U.lookup_setup(case, "cpu")
    assert T["dst"].data_ptr() % 32 == 16 and T["add"].data_ptr() % 32 == 16 and T["idx_dev"].data_ptr() % 8 == 4
    assert case["ldd"] > case["cols"] and T["bstride"] > case["period"] * case["ldd"] and case["tokens"] % case["period"]
    g = by_name(TC.GRAD, "mixed-129x257-pad5")
    T = U.grad_setup(g, "cpu", True)
    dead = (T["key"] == g["vocab"]).nonzero().flatten()
    pad = (T["idx"] == 5).nonzero().flatten()
    assert len(pad) > 0 and len(dead) > len(pad) and torch.isnan(T["dy"][T["src"][dead]]).all()          # padding and out-of-range rows of dy are NaN
    wide = torch.as_strided(T["dy"], (T["dy"].shape[0], g["ldy"]), (g["ldy"], 1), T["dy"].storage_offset())
    assert torch.isnan(wide[:, g["cols"]:]).all()
    gap = torch.ones(T["dy"].shape[0], dtype=torch.bool)
    gap[T["src"]] = False
    assert gap.sum() > 0 and torch.isnan(T["dy"][gap]).all()


# ------------------------------------------------------------------------------------------------ (d) planted faults
FAULT_L = by_name(TC.LOOKUP, "every-class-named")          # 33 tokens, every row once, ldd = cols + 4, add and accumulate
FAULT_P = by_name(TC.LOOKUP, "oob-68x10-a1c0-i64")         # period 7, 10 tokens: a partial last group
FAULT_G = by_name(TC.GRAD, "mixed-129x257-pad5")


def test_fault_one_row_rescaled_twice():
    T = U.lookup_setup(FAULT_L, "cpu")
    named = torch.zeros(33, dtype=torch.bool)
    named[T["idx"]] = True
    r = int((named & (T["w0"].double().norm(dim=1) > 2 * FAULT_L["max_norm"])).nonzero()[0])
    with pytest.raises(AssertionError, match=rf"table: \d+ of \d+ elements wrong; first \(row, column, got, want, bound\): \[\({r}, 0,"):
        U.lookup_case(FAULT_L, "cpu", emulate_lookup("twice"))


def test_fault_one_token_reads_the_next_row():
    T = U.lookup_setup(FAULT_L, "cpu")
    t = FAULT_L["tokens"] - 1
    assert int(T["idx"][t]) == 0
    with pytest.raises(AssertionError, match=rf"destination \(row = the token\): \d+ of \d+ elements differ in their bits; first \(row, column, got, want\): \[\({t}, 0,"):
        U.lookup_case(FAULT_L, "cpu", emulate_lookup("idx+1"))


def test_fault_skipped_last_partial_group():
    with pytest.raises(AssertionError, match=r"destination \(row = the token\): \d+ of \d+ elements differ in their bits; first \(row, column, got, want\): \[\(7, 0, nan"):
        U.lookup_case(FAULT_P, "cpu", emulate_lookup("last-group"))


def test_fault_ldd_taken_for_cols():
    with pytest.raises(AssertionError, match=r"destination \(row = the token\): \d+ of \d+ elements differ in their bits; first \(row, column, got, want\): \[\(1, 0,"):
        U.lookup_case(FAULT_P, "cpu", emulate_lookup("ldd"))


def test_fault_padding_row_summed():
    """the padding tokens' rows of dy are NaN: summed, they poison the padding row of dtable"""
    with pytest.raises(AssertionError, match=r"atomic, int64, integers\): dtable \(integers\): 129 of \d+ elements wrong; first \(row, column, got, want\): \[\(5, 0, nan"):
        U.grad_case(FAULT_G, "cpu", emulate_grad("pad"))


def test_fault_ties_sorted_in_reverse():
    """integer sums do not see the order; the bitwise check of the real sums does, then the scratch would"""
    c = FAULT_G
    T = U.grad_setup(c, "cpu", False)
    O = U.grad_outputs(c, T, "cpu", True)
    U.grad_emulate_into(c, T, O, True, "ties")
    with pytest.raises(AssertionError, match=r"scratch, tokens by \(key, position\).*elements wrong; first \(row, column, got, want\): \[\(0, \d+,"):
        U.grad_check(c, T, O, True)          # integers: exact in any order, the scratch names the first place
    with pytest.raises(AssertionError, match=r"det, int64, randn\): dtable against \(\(\(g_0 \+ g_1\) \+ g_2\) \+ \.\.\.\) in position order: \d+ of \d+ elements differ in their bits; "
                                             r"first \(row, column, got, want\): \[\(\d+, \d+,"):
        U.grad_case(c, "cpu", lambda case, T, O, det, ib: U.grad_emulate_into(case, T, O, det, "ties" if det and T["real"] else None))


def test_fault_store_into_a_guard_and_a_stale_marker():
    T = U.lookup_setup(FAULT_P, "cpu")
    U.lookup_emulate_into(FAULT_P, T)
    U.flat_of(T["dst"], T["dst_rows"] * FAULT_P["ldd"])[2 * FAULT_P["ldd"] + FAULT_P["cols"]] = 1.0          # row 2, first column past cols
    with pytest.raises(AssertionError, match=rf"dst: \d+ guard bytes overwritten.*\(2, {FAULT_P['cols']}\)"):
        U.lookup_check(FAULT_P, T)
    T = U.lookup_setup(FAULT_P, "cpu")
    U.lookup_emulate_into(FAULT_P, T)
    T["marker"].t[0, 3] = 1
    with pytest.raises(AssertionError, match=r"marker .*1 of 17 elements wrong; first \(row, column, got, want\): \[\(0, 3, 1"):
        U.lookup_check(FAULT_P, T)
    T = U.lookup_setup(FAULT_P, "cpu")
    U.lookup_emulate_into(dict(FAULT_P, flag=0), T)          # the flag not raised
    with pytest.raises(AssertionError, match=r"flag word 2, want 6"):
        U.lookup_check(FAULT_P, T)


# ------------------------------------------------------------------------------------------------ refusals (no launch)
@pytest.fixture(scope="module")
def H():
    importlib.import_module("mca-paper_amd.build").build()
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def test_refusals_move_no_byte(H):
    L = H.lib()
    case = by_name(TC.LOOKUP, "oob-68x10-a1c1-i64")
    T = U.lookup_setup(case, "cpu")
    before = U.lookup_snapshot(T)
    for name, rc, want in U.lookup_refusals(L, case, T):
        assert rc == want, f"lookup: {name}: {rc}, want {want}"
    for k, b in before.items():
        assert torch.equal(T[k].buf, b), f"lookup: {k} moved in a refused or empty call"
    g = FAULT_G
    T = U.grad_setup(g, "cpu", False)
    O = U.grad_outputs(g, T, "cpu", True)
    before = {k: O[k].buf.clone() for k in ("dtable", "scratch")}
    assert L.mca_embedding_scatter_add_det_scratch(g["tokens"]) == 2 * g["tokens"] and L.mca_embedding_scatter_add_det_scratch(0) == 0
    for name, rc, want in U.grad_refusals(L, g, T, O):
        assert rc == want, f"{name}: {rc}, want {want}"
    for k, b in before.items():
        assert torch.equal(O[k].buf, b), f"{k} moved in a refused or empty call"


def test_print_worst_ratios():
    """last in the file: how much of each bound the fp32 restatements use over all cases (pytest -s shows it)"""
    for k in sorted(U.WORST):
        print(f"worst |emulation - ref| / bound  {k:24s} {U.WORST[k]:.3f}")
    assert set(U.WORST) >= {"lookup table", "dtable det", "dtable atomic"}
