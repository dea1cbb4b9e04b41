"""Top-k retrieval and the kNN readout, checked without a GPU (tests/topk_edge_util.py, tests/topk_cases.py):
(a) the reference of the semantics against brute force on hand-written matrices with ties, a NaN, +-0 and +-inf;
(b) the case list reaches every boundary it is listed for, and every combination of the optional arguments;
(c) the checker raises and names the element of each planted fault in a torch restatement of the kernel's chunked selection;
(d) knn_predict and hits_at on written-out inputs, the rank <-> top-k identity on exact matrices, cosine_topk's argument errors
    without a HIP device, and the workspace query of the built library."""
import importlib
import math

import pytest
import torch

import topk_cases as TC
import topk_edge_util as U

F64 = torch.float64
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def M():
    return importlib.import_module("mca-paper_amd.metrics")


# ------------------------------------------------------------------------------------------------ (a) the reference
HAND = [
    # ties in every row; row 1 is all equal
    ([[1.0, 3.0, 3.0, 2.0, 3.0], [2.0, 2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 5.0, 5.0, -1.0]], None, None),
    # a NaN score is never returned; +0 and -0 tie (the lower index first); +-inf are ordinary scores
    ([[NAN, 0.0, -0.0, 1.0], [-0.0, 0.0, NAN, -1.0], [-INF, INF, NAN, -INF], [NAN, NAN, NAN, NAN]], None, None),
    # a mask and exclusions (row 0 loses its best, row 1 excludes nothing, row 2 a masked target, row 3 past the end)
    ([[4.0, 3.0, 2.0, 1.0], [4.0, 3.0, 2.0, 1.0], [1.0, 1.0, 1.0, 1.0], [-INF, -INF, 2.0, NAN]], [1, 0, 1, 1], [0, -1, 1, 7]),
]


@pytest.mark.parametrize("k", [1, 2, 4, 6])
@pytest.mark.parametrize("rows,tvalid,exclude", HAND, ids=["ties", "special", "masked"])
def test_reference_against_brute_force(rows, tvalid, exclude, k):
    S = torch.tensor(rows, dtype=F64)
    tv = torch.tensor(tvalid, dtype=torch.uint8) if tvalid is not None else None
    ex = torch.tensor(exclude) if exclude is not None else None
    score, index = U.topk_ref(S, k, tv, ex)
    want = U.brute_force(S, k, tvalid, exclude)
    assert index.tolist() == [[j for _, j in row] for row in want]
    got = score.tolist()
    for r, row in enumerate(want):
        for c, (s, _) in enumerate(row):
            assert got[r][c] == s and math.copysign(1, got[r][c]) == math.copysign(1, s), (r, c, got[r][c], s)


def test_reference_written_out():
    S = torch.tensor(HAND[1][0], dtype=F64)
    score, index = U.topk_ref(S, 3)
    assert index.tolist() == [[3, 1, 2], [0, 1, 3], [1, 0, 3], [-1, -1, -1]]
    assert score[0].tolist() == [1.0, 0.0, -0.0] and score[2].tolist() == [INF, -INF, -INF] and score[3].tolist() == [-INF] * 3
    score, index = U.topk_ref(torch.zeros(2, 0, dtype=F64), 2)          # no target: all padding
    assert index.tolist() == [[-1, -1]] * 2 and score.tolist() == [[-INF, -INF]] * 2


# ------------------------------------------------------------------------------------------------ (b) the list's coverage
def test_cases_reach_their_boundaries():
    C = TC.TOPK
    assert len({c["name"] for c in C}) == len(C)
    assert {(c["nq"], TC.cdiv(c["nq"], TC.TILE), c["nq"] % TC.TILE) for c in C} == {(1, 1, 1), (63, 1, 63), (64, 1, 0), (65, 2, 1)}
    assert {(c["d"], TC.cdiv(c["d"], TC.KC), c["d"] % TC.KC) for c in C} == {(1, 1, 1), (16, 1, 0), (17, 2, 1), (96, 6, 0)}
    assert {c["k"] for c in C} == {1, 2, 10, 63, 64} and TC.TOPK_MAX == 64
    tiles = {c["nt"]: (TC.cdiv(c["nt"], TC.TILE), TC.chunks(c["nt"])) for c in C}
    assert tiles == {1: (1, 1), 63: (1, 1), 64: (1, 1), 65: (2, 1), 1023: (16, 1), 1024: (16, 1), 1025: (17, 2), 2049: (33, 3)}
    assert max(c["nt"] for c in C) <= 2100
    assert {(c["qidx"], c["tvalid"], c["exclude"]) for c in C} == {(a, b, e) for a in (0, 1) for b in (0, 1) for e in (0, 1)}
    assert any(c["k"] > c["nt"] for c in C) and any(c["k"] == 64 and TC.chunks(c["nt"]) > 1 for c in C)
    for mine in ([c for c in C if TC.chunks(c["nt"]) == 1], [c for c in C if TC.chunks(c["nt"]) > 1]):          # with and without a merge of chunks
        assert len({(c["qidx"], c["tvalid"], c["exclude"]) for c in mine}) == 8
    # the gather is out of order and repeats; the patterns remove something and keep something
    assert U.gather_index(5, 10).tolist() == [9, 8, 7, 6, 9]
    v = U.valid_pattern(65, "cpu")
    assert not v[64] and not v[1] and v[0] and v[63] and U.valid_pattern(1, "cpu").tolist() == [True]
    assert U.exclude_pattern(6, 4, "cpu").tolist() == [0, 1, 2, 3, -1, 1]


def test_exclusions_and_masks_change_the_listed_results():
    """an option that never changed a result would be an option never tested"""
    changed = {"tvalid": 0, "exclude": 0}
    for c in TC.TOPK:
        T, _ = U.topk_setup(c, "cpu")
        S = U.scores64(c, T)
        full = U.topk_ref(S, c["k"])[1]
        if c["tvalid"]:
            changed["tvalid"] += int(not torch.equal(full, U.topk_ref(S, c["k"], T["tvalid"])[1]))
        if c["exclude"]:
            changed["exclude"] += int(not torch.equal(full, U.topk_ref(S, c["k"], None, T["exclude"].long())[1]))
    assert changed["tvalid"] >= 8 and changed["exclude"] >= 8, changed


# ------------------------------------------------------------------------------------------------ (c) planted faults
def by(**attrs):
    return next(c for c in TC.TOPK if all(c[k] == v for k, v in attrs.items()))


def run(c, fault=None):
    T, O = U.topk_setup(c, "cpu")
    U.topk_emulate(c, T, O, fault)
    return T, O


@pytest.mark.parametrize("case", TC.TOPK, ids=[c["name"] for c in TC.TOPK])
def test_restatement_passes_the_check(case):
    T, O = run(case)
    U.topk_check(case, T, O)


WHERE = r"\d+ of \d+ elements wrong; first \(row, column, got, want\): \[\(\d+, \d+,"
PLANTED = [
    ("tie_high", dict(nt=65, nq=64), r"index \(row = the query, column = the place\): " + WHERE),
    ("merge_drop", dict(nt=1025, k=10), r"index .*" + WHERE),
    ("tail", dict(nt=63, k=64), r"index .*" + WHERE),
    ("exclude_ignored", dict(nt=65, nq=64), r"index .*" + WHERE),
    ("pad_sentinel", dict(nt=1, k=10), r"score \(row = the query, column = the place\): " + WHERE),
]


@pytest.mark.parametrize("fault,attrs,message", PLANTED, ids=[p[0] for p in PLANTED])
def test_checker_names_the_element_of_a_planted_fault(fault, attrs, message):
    c = by(**attrs)
    T, O = run(c, fault)
    with pytest.raises(AssertionError, match=message):
        U.topk_check(c, T, O)


def test_checker_names_one_element():
    c = by(nt=2049, k=63)
    T, O = run(c)
    U.topk_check(c, T, O)
    O["index"].t[c["nq"] - 1, 62] += 1
    with pytest.raises(AssertionError, match=rf"index .*1 of {c['nq'] * 63} elements wrong; first \(row, column, got, want\): \[\({c['nq'] - 1}, 62,"):
        U.topk_check(c, T, O)
    T, O = run(c)
    O["ws"].buf[O["ws"].start - 1] = 0
    with pytest.raises(AssertionError, match="ws: 1 guard bytes overwritten"):
        U.topk_check(c, T, O)


# ------------------------------------------------------------------------------------------------ (d) the python surface
def test_knn_predict_written_out(M):
    labels = torch.tensor([1.0, 0.0, 4.0, 2.0])
    idx = torch.tensor([[0, 2, 3], [1, -1, -1], [-1, -1, -1], [2, 3, -1]])
    sc = torch.tensor([[0.5, 0.25, 0.25], [-0.5, -INF, -INF], [-INF, -INF, -INF], [0.0, -1.0, -INF]])
    got = M.knn_predict(sc, idx, labels)
    assert got.shape == (4,) and got[:2].tolist() == [torch.tensor(7.0).div(3.0).item(), 0.0] and math.isnan(got[2]) and got[3].item() == 3.0
    w = M.knn_predict(sc, idx, labels, weighted=True)
    assert w[0].item() == (0.5 * 1 + 0.25 * 4 + 0.25 * 2) / 1.0          # weights 0.5, 0.25, 0.25
    assert math.isnan(w[1]) and math.isnan(w[2]) and math.isnan(w[3])    # every weight clamps to 0
    two = torch.stack([labels, 2 * labels], 1)
    got2 = M.knn_predict(sc, idx, two)
    assert got2.shape == (4, 2) and torch.equal(got2[[0, 1, 3]], torch.stack([got, 2 * got], 1)[[0, 1, 3]]) and torch.isnan(got2[2]).all()
    poisoned = labels.clone()
    poisoned[0] = NAN                        # padding picks row 0 and must drop it
    assert M.knn_predict(sc, idx, poisoned)[1].item() == 0.0 and M.knn_predict(sc, idx, poisoned)[3].item() == 3.0


def test_hits_at_written_out(M):
    idx = torch.tensor([[4, 2, 9], [1, 0, -1], [-1, -1, -1], [5, 6, 7]])
    pos = torch.tensor([9, 1, 0, 6])
    assert M.hits_at(idx, pos, 1).tolist() == [False, True, False, False]
    assert M.hits_at(idx, pos, 2).tolist() == [False, True, False, True]
    assert M.hits_at(idx, pos, 3).tolist() == [True, True, False, True]
    assert M.hits_at(idx, torch.tensor([9, 1, -1, 6]), 3).tolist() == [True, True, False, True]          # padding is no hit
    assert "ties" in M.hits_at.__doc__ and "rank < m" in M.hits_at.__doc__


def test_rank_topk_identity_on_exact_matrices():
    """rank[r] < m  <=>  s_true[r] >= score[r][m - 1] for every m <= min(k, nt): fewer than m scores lie strictly above the true one
    exactly when the m-th best does not"""
    g = torch.Generator().manual_seed(5)
    ties = 0
    for nq, nt, k in ((7, 9, 4), (9, 9, 9), (5, 70, 64), (3, 3, 10)):
        S = torch.randint(-3, 4, (nq, nt), generator=g).double()
        st = S[torch.arange(nq), torch.arange(nq)]
        rank = (S > st[:, None]).sum(1)
        score, index = U.topk_ref(S, k)
        for m in range(1, min(k, nt) + 1):
            assert torch.equal(rank < m, st >= score[:, m - 1]), (nq, nt, k, m)
        for m in range(1, min(k, nt) + 1):          # presence is the stricter statement, and differs only on ties
            hit = (index[:, :m] == torch.arange(nq)[:, None]).any(1)
            assert bool((hit <= (rank < m)).all())
            ties += int((hit != (rank < m)).sum())
    assert ties > 0


def test_cosine_topk_argument_errors_need_no_device(M):
    q, t = torch.zeros(5, 8), torch.zeros(7, 8)
    for k in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError, match="k must be"):
            M.cosine_topk(q, t, k)
    with pytest.raises(ValueError, match="features"):
        M.cosine_topk(q, torch.zeros(7, 9), 3)
    with pytest.raises(ValueError, match="target_mask has 6 entries for 7 targets"):
        M.cosine_topk(q, t, 3, target_mask=torch.ones(6, dtype=torch.bool))
    with pytest.raises(ValueError, match="exclude has 5 entries for 2 queries"):
        M.cosine_topk(q, t, 3, query_index=torch.tensor([0, 4]), exclude=torch.zeros(5, dtype=torch.long))
    with pytest.raises(ValueError, match="exclude has 4 entries for 5 queries"):
        M.cosine_topk(q, t, 3, exclude=torch.zeros(4, dtype=torch.long))
    for bad in ([5], [-1], [0, 7]):
        with pytest.raises(IndexError, match="outside the 5 query rows"):
            M.cosine_topk(q, t, 3, query_index=torch.tensor(bad))
    with pytest.raises(ValueError, match="HIP device, not on cpu"):
        M.cosine_topk(q, t, 3, device="cpu")
    import utils.metrics as um
    assert um.cosine_topk is M.cosine_topk and um.knn_predict is M.knn_predict and um.hits_at is M.hits_at


def test_workspace_query_of_the_built_library():
    importlib.import_module("mca-paper_amd.build").build(verbose=False)
    hip = importlib.import_module("mca-paper_amd.hip")
    ws = hip.lib().mca_cosine_topk_workspace
    for c in TC.TOPK:
        assert ws(c["nq"], c["nt"], c["k"]) == TC.workspace_bytes(c["nq"], c["nt"], c["k"])
    sizes = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 70000)
    for a, b in zip(sizes, sizes[1:]):          # monotone in every argument
        assert 0 <= ws(a, 1025, 10) <= ws(b, 1025, 10) and 0 <= ws(65, a, 10) <= ws(65, b, 10)
    assert ws(65, 1024, 10) < ws(65, 1025, 10) and ws(64, 1025, 10) < ws(65, 1025, 10)
    for k in range(1, 64):
        assert ws(65, 1025, k) < ws(65, 1025, k + 1)
    assert ws(0, 5, 3) == 0 and ws(5, 0, 3) == 0
    for bad in ((-1, 5, 3), (5, -1, 3), (5, 5, 0), (5, 5, 65), (5, 5, -2)):
        assert ws(*bad) < 0, bad
