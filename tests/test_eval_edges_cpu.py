"""The evaluation-kernel edge tests, checked without a GPU (tests/eval_edge_util.py, tests/eval_cases.py):
(a) every listed case reaches the tile, chunk and lane edges it is listed for, by the formulas of csrc/evaluate.hip's launch code;
(b) the checkers raise and name the element of each planted fault;
(c) every derived bound is satisfiable: fp32 torch restatements of the kernels, stored where the kernels store, pass the very checks
    the GPU tests run, at every element of every case, with the worst ratio to each bound under a recorded cap."""
import pytest
import torch

import eval_cases as EC
import eval_edge_util as E

FAMILIES = {"normalize": EC.NORMALIZE, "rank": EC.RANK, "pair": EC.PAIR, "nt": EC.PROBE_NT, "head": EC.PROBE_HEAD, "tn": EC.PROBE_TN}
ALL = [(f, c) for f, cases in FAMILIES.items() for c in cases]


def run(family, case, **kw):
    T, O = getattr(E, family + "_setup")(case, "cpu")
    getattr(E, family + "_emulate")(case, T, O, **kw)
    return T, O


def by_name(cases, name):
    return next(c for c in cases if c["name"] == name)


def pick(cases, **attrs):
    return next(c for c in cases if all(c[k] == v for k, v in attrs.items()))


# ------------------------------------------------------------------------------------------------ (a) paths
def test_cases_reach_their_edges():
    t, k = EC.TILE, EC.KC
    assert {(c["nq"], EC.cdiv(c["nq"], t), c["nq"] % t) for c in EC.RANK} == {(1, 1, 1), (63, 1, 63), (64, 1, 0), (65, 2, 1)}
    chunks = {c["nt"]: (EC.cdiv(c["nt"], t), EC.cdiv(EC.cdiv(c["nt"], t), EC.RANK_TILES_PER_CHUNK)) for c in EC.RANK}
    assert chunks == {1: (1, 1), 63: (1, 1), 65: (2, 1), 1024: (16, 1), 1025: (17, 2)}          # 1024: one full chunk; 1025: a second chunk of one tile
    assert {(c["d"], EC.cdiv(c["d"], k), c["d"] % k) for c in EC.RANK} == {(1, 1, 1), (15, 1, 15), (16, 1, 0), (17, 2, 1), (96, 6, 0)}
    assert any(c["gather"] for c in EC.RANK) and any(not c["gather"] for c in EC.RANK) and all(c["gather"] for c in EC.RANK if c["nq"] > c["nt"])
    assert {(c["n"], E.pair_tiles(c["n"])) for c in EC.PAIR} == {(0, 1), (1, 1), (2, 1), (63, 1), (64, 1), (65, 2), (129, 3)}
    forms = {(c["act"], c["p"]) for c in EC.PROBE_NT}
    assert forms == {(0, 0.0), (1, 0.0), (2, 0.0), (2, 0.5), (2, 1.0), (2, 0.25)}
    for N in (1, 63, 64, 65, 130):          # every width sees every form, bias given and not, gathered and not
        mine = [c for c in EC.PROBE_NT if c["N"] == N]
        assert {(c["act"], c["p"]) for c in mine} == forms and {c["bias"] for c in mine} == {0, 1} and {c["gather"] for c in mine} == {0, 1}
    assert {EC.cdiv(c["K"], 64) for c in EC.PROBE_HEAD} == {1, 2, 16} and max(c["K"] for c in EC.PROBE_HEAD) == 1024          # av[16] up to j = 15
    for K in (1, 63, 64, 65, 1023, 1024):
        mine = [c for c in EC.PROBE_HEAD if c["K"] == K]
        assert {c["loss"] for c in mine} == {EC.L1, EC.MSE, EC.BCE} and {c["L"] for c in mine} == {1, 2, 63, 64}
        for flag in ("dz", "da", "aidx", "yidx"):
            assert {c[flag] for c in mine} == {0, 1}
    assert {(c["B"], EC.cdiv(c["B"], 4), c["B"] % 4) for c in EC.PROBE_HEAD} == {(1, 1, 1), (3, 1, 3), (4, 1, 0), (5, 2, 1)}          # B = 5: a block with three idle waves
    assert {(c["R"], EC.cdiv(c["R"], EC.PROBE_ROWS_PER_CHUNK)) for c in EC.PROBE_TN} == {(1, 1), (127, 1), (128, 1), (129, 2), (300, 3)}
    assert {(c["K"], EC.cdiv(c["K"] + 1, t)) for c in EC.PROBE_TN} == {(1, 1), (62, 1), (63, 1), (64, 2), (127, 2)}          # the ones column: last of a tile, first of the next
    assert {c["gather"] for c in EC.PROBE_TN} == {0, 1}


# ------------------------------------------------------------------------------------------------ (b) planted faults
def test_rank_checker_names_the_query():
    c = pick(EC.RANK, nq=65, nt=1025, d=17)
    T, O = run("rank", c)
    E.rank_check(c, T, O)
    O["rank"].t[0, 64] += 1
    with pytest.raises(AssertionError, match=r"rank .*1 of 65 elements wrong; first \(row, column, got, want\): \[\(0, 64,"):
        E.rank_check(c, T, O)


def test_rank_ties_are_planted_and_not_counted():
    c = pick(EC.RANK, nq=64, nt=65, gather=False)
    T, _ = run("rank", c)
    st, rk = E.rank_ref(c, T)
    S = T["q"].double() @ T["t"].double().t()
    assert float(S[0, 0]) == float(S[0, 64]) and torch.equal(T["q"][1], T["t"][1])          # a duplicate target, a query equal to its target
    assert int(((S == st[:, None].double()).sum(1) > 1).sum()) > 32 and int((S >= st[:, None].double()).sum(1)[0]) > int(rk[0])


def test_pair_checker_sees_a_partial_below_the_diagonal():
    c = by_name(EC.PAIR, "pair-n129d17")
    T, O = run("pair", c)
    E.pair_check(c, T, O)
    O["partials"].t[0, 3] = 1e-30          # tile (1, 0)
    with pytest.raises(AssertionError, match="below the diagonal"):
        E.pair_check(c, T, O)
    T, O = run("pair", c)
    O["partials"].t[0, 4] += 64.0          # tile (1, 1) with its own diagonal counted: exp(0) per row
    with pytest.raises(AssertionError, match=r"partials.*first \(row, column, got, want, bound\): \[\(1, 1,"):
        E.pair_check(c, T, O)


def test_nt_checker_sees_a_wrong_mask_unit():
    c = by_name(EC.PROBE_NT, next(x["name"] for x in EC.PROBE_NT if x["act"] == 2 and x["p"] == 0.5 and x["M"] == 65 and x["N"] == 65))
    T, O = run("nt", c)
    E.nt_check(c, T, O)
    keep = E._mask_ref(E.SEED, E.STEP, 65, 65, 0.5)
    assert 0.4 < float(keep.float().mean()) < 0.6
    assert bool(keep[64, 64]) == bool(O["y"].t[64, 64] > 0)
    O["y"].t[64, 64] = 0.0 if keep[64, 64] else 1.0
    with pytest.raises(AssertionError, match=r"kept units.*\[\(64, 64,"):
        E.nt_check(c, T, O)


def test_head_checker_sees_a_gate_that_lets_zero_through():
    c = by_name(EC.PROBE_HEAD, next(x["name"] for x in EC.PROBE_HEAD if x["da"] and x["loss"] == EC.MSE and x["K"] == 65 and x["B"] == 5))
    T, O = run("head", c)
    E.head_check(c, T, O)
    T, O = run("head", c, gate=lambda a: a >= 0)
    with pytest.raises(AssertionError, match=r": da: \d+ of \d+ elements wrong"):
        E.head_check(c, T, O)


def test_head_planted_values():
    c = by_name(EC.PROBE_HEAD, next(x["name"] for x in EC.PROBE_HEAD if x["loss"] == EC.BCE and x["L"] == 63 and x["dz"]))
    T, O = run("head", c)
    z = O["pred"].t
    assert set(E.PLANT_Z) <= set(z[0].tolist()) and torch.isfinite(O["dz"].t).all() and torch.isfinite(O["loss_part"].t).all()
    c = by_name(EC.PROBE_HEAD, next(x["name"] for x in EC.PROBE_HEAD if x["loss"] == EC.L1 and x["dz"] and x["B"] == 5))
    T, O = run("head", c)
    assert (O["dz"].t[4] == 0).all() and (O["dz"].t[:4] != 0).any()          # e == 0 under L1: gradient 0


def test_tn_checker_sees_a_bias_column_that_is_not_ones():
    c = pick(EC.PROBE_TN, R=129, N=65, K=63)
    T, O = run("tn", c)
    E.tn_check(c, T, O)
    T, O = run("tn", c, ones=3.0)
    with pytest.raises(AssertionError, match=r"gb \(row = 0, column = the output unit\)"):
        E.tn_check(c, T, O)


# ------------------------------------------------------------------------------------------------ (c) every bound is satisfiable
@pytest.mark.parametrize("family,case", ALL, ids=[c["name"] for _, c in ALL])
def test_emulation_within_bounds(family, case):
    T, O = run(family, case)
    getattr(E, family + "_check")(case, T, O)


# the worst |emulation - reference| / bound over every case above, rounded up to the next 0.05 (docs/parity.md)
CAPS = {"eval normalize": 0.35, "eval pair partials": 0.10, "eval pair sum": 0.10, "eval pair value": 0.40, "eval probe_nt p=0.25": 0.70,
        "eval head dz (BCE)": 0.65, "eval head da": 0.25, "eval head loss_part (BCE)": 0.20}


def test_worst_ratios_under_their_caps():
    assert all(c < 1 for c in CAPS.values())
    seen = {k: v for k, v in E.WORST.items() if k in CAPS}
    for k in sorted(seen):
        print(f"worst |emulation - ref| / bound  {k:28s} {seen[k]:.3f}  (cap {CAPS[k]:.2f})")
    assert seen, "run after test_emulation_within_bounds"
    for k, v in seen.items():
        assert v <= CAPS[k], (k, v, CAPS[k])
