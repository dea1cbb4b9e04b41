"""The contrastive-loss edge tests, checked without a GPU (tests/loss_edge_util.py, tests/loss_cases.py):
(a) the float64 restatement of csrc/loss.hip's formulas agrees with oracle.mca_oracle.pretraining_loss + autograd on the three
    small-config schedules at one and two ranks;
(b) the checker raises and names the element of each planted fault;
(c) every listed case reaches the path it is listed for, by the formulas of the launch code;
(d) every derived bound is satisfiable: an fp32 torch restatement of the five kernels in their summation grouping passes the very
    checker the GPU test runs, at every element of every case and rank, with its worst ratio to each bound under a recorded cap;
and the workspace layout, which needs no launch."""
import importlib

import pytest
import torch

import loss_cases as LC
import loss_edge_util as U

CASE = {c["name"]: (i, c) for i, c in enumerate(LC.CASES)}
_cache = {}


def prepared(name):
    """(data, reference) of a listed case, computed once"""
    if name not in _cache:
        i, c = CASE[name]
        d = U.make_data(c, i)
        _cache[name] = (d, U.reference(d))
    return _cache[name]


@pytest.fixture(scope="module")
def H():
    importlib.import_module("mca-paper_amd.build").build()
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


# ------------------------------------------------------------------------------------------------ the workspace layout
@pytest.mark.parametrize("B,T", [(1, 1), (17, 3), (100, 50), (513, 1), (4096, 60)])
def test_workspace_layout(H, B, T):
    lay = H.contrastive_layout(B, T)
    (g0, gn), (s0, sn), (w0, wn) = lay["G"], lay["stats"], lay["w"]
    assert g0 == 0 and gn == T * B * B * 4 and s0 == g0 + gn and sn == T * B * 4 * 4 and w0 == s0 + sn and wn == T * B * 4
    assert g0 % 4 == 0 and s0 % 4 == 0 and w0 % 4 == 0
    assert H.lib().mca_contrastive_workspace_bytes(B, T) == w0 + wn + 256
    assert H.lib().mca_dbg_contrastive_layout(B, T, None) == -1


# ------------------------------------------------------------------------------------------------ (a) the reference against the oracle
@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("variant", ["mca", "bimodal", "zorro"])
def test_reference_agrees_with_oracle(variant, world):
    from oracle import mca_oracle as O
    from util_small import small_config
    cfg = small_config(variant)
    OS = O.Structure(cfg)
    terms, R, names = U.schedule_terms(variant)
    assert names == [t[0] for t in O.loss_schedule(OS)]
    mods = list(cfg["encoder_configs"].keys())
    b, D = 3, 16
    B = b * world
    d = U.make_data(dict(name=f"oracle-{variant}-{world}", terms=f"schedule:{variant}", R=None, B=B, D=D, b_local=b, kind="prod3",
                         present={0: 0b101, 1: 0b101, 2: 0b001}), 7)          # rank 0 never sees modality 1: NaN terms there
    d["pooled"] = (torch.randn(B, R, D, generator=torch.Generator().manual_seed(21)) * 0.3).float()
    ref = U.reference(d)
    pa = d["pooled"].double().requires_grad_(True)
    total, outs = torch.zeros(B, R, D, dtype=torch.float64), []
    for r in range(world):
        lg = d["s"].double().clone().requires_grad_(True)
        sm = {n: ((d["present"][r * b:(r + 1) * b] >> i) & 1).bool() for i, n in enumerate(mods)}
        out = O.pretraining_loss(OS, pa[r * b:(r + 1) * b], sm, lg, pooled_all=pa, rank=r)
        gp, gl = torch.autograd.grad(out["loss"], [pa, lg])
        total += gp
        outs.append((out, gl))
    rel = lambda a, b_: float((a - b_).abs().max()) <= 1e-12 * max(float(b_.abs().max()), 1e-300)
    saw_nan = False
    for r in range(world):
        out, gl = outs[r]
        R_ = ref["ranks"][r]
        want = torch.stack([out["losses"][n].detach() for n in names])
        assert torch.equal(torch.isnan(want), ~R_["live"])
        saw_nan |= bool(torch.isnan(want).any())
        assert rel(R_["term_loss"][R_["live"]], want[R_["live"]])
        assert rel(R_["loss"], out["loss"].detach()) and rel(R_["dls"], gl)
        assert rel(R_["d_pooled"], total[r * b:(r + 1) * b])
    assert saw_nan or variant != "mca"


# ------------------------------------------------------------------------------------------------ (b) planted faults
def emulated(name, r=0, **faults):
    d, ref = prepared(name)
    return d, ref, U.emulate(d, r, **faults)


def test_checker_names_a_wrong_dG_element_in_a_tail_tile():
    d, ref, o = emulated("gram-B17D16R3b17-exact")
    U.check(d, ref, 0, o)
    o["dG"][2, 16, 16] += 4 * float(ref["dG_tol"][2, 16, 16]) + 1e-6
    with pytest.raises(AssertionError, match=r"dG: 1 of 867 elements wrong; first: term 2, row 16, column 16"):
        U.check(d, ref, 0, o)


def test_checker_sees_a_dropped_fourth_slice():
    name = "dpooled-B5D129R4b5-exact"
    d, ref, o = emulated(name, slices=3)
    with pytest.raises(AssertionError, match=r"d_pooled: \d+ of \d+ elements wrong; first: row \d+, slot \d+, column \d+"):
        U.check(d, ref, 0, o)
    iso, tol = U.dpooled64(d, o["dG"].double(), None, 0)          # the check that isolates dpooled_kernel sees it on its own
    with pytest.raises(AssertionError, match=r"row \d+, slot \d+, column \d+"):
        U.close(o["d_pooled"], iso, tol, "d_pooled | dG", None, ("row", "slot", "column"))
    good = U.emulate(d, 0)
    U.close(good["d_pooled"], *U.dpooled64(d, good["dG"].double(), None, 0), "d_pooled | dG", None, ("row", "slot", "column"))


def test_checker_sees_rank_0_counts_used_for_every_rank():
    d, ref, o = emulated("ranks-B6D7R3b2-exact", n_from_rank0=True)
    assert ref["n"][0].tolist() == [0, 2, 2]          # the and-only term: no valid row on rank 0 only
    with pytest.raises(AssertionError, match=r"w: \d+ of 9 elements wrong; first: term 0, rank 1"):
        U.check(d, ref, 0, o)


def test_checker_sees_ignored_or_bits():
    d, ref, o = emulated("ranks-B6D7R3b6-exact", ignore_or=True)
    assert int(d["present"][5]) == 1 and int(ref["n"][1, 0]) == 5          # row 5 has neither modality of the or-only term
    with pytest.raises(AssertionError, match=r"w: 1 of 3 elements wrong; first: term 1, rank 0"):
        U.check(d, ref, 0, o)


def test_checker_sees_a_stale_sentinel_in_an_unused_slot():
    d, ref, o = emulated("dpooled-B3D127R4b3-prod3")
    U.check(d, ref, 0, o)
    o["d_pooled"][:, 3].view(torch.int32).fill_(-1)
    with pytest.raises(AssertionError, match=r"slot 3, which no term names: 381 of 381 elements wrong; first: row 0, column 0"):
        U.check(d, ref, 0, o)


def test_checker_sees_a_wrong_nan_and_a_missing_nan():
    d, ref, o = emulated("ranks-B6D7R3b2-exact")
    U.check(d, ref, 0, o)
    o["term_loss"].view(torch.int32)[0] = 0x7FC00001
    with pytest.raises(AssertionError, match="quiet NaN"):
        U.check(d, ref, 0, o)
    o["term_loss"][0] = 0.0
    with pytest.raises(AssertionError, match=r"term_loss is NaN: 1 of 3 elements wrong; first: term 0"):
        U.check(d, ref, 0, o)


def test_production_magnitude_needs_the_max_subtraction():
    """the fp32 restatement without the max subtraction overflows on the production-magnitude data and passes on nothing else"""
    d, ref = prepared("gram-B17D17R3b17-prod4")
    with pytest.raises(AssertionError, match=r"stats: \d+ of \d+ elements wrong; first: term \d+, row \d+, column \d+"):
        U.check(d, ref, 0, U.emulate(d, 0, max_subtract=False))


# ------------------------------------------------------------------------------------------------ (c) the paths of the listed cases
def _paths(c):
    T = c["T"] if c["T"] is not None else len(U.schedule_terms(c["terms"].split(":")[1])[0])
    return LC.paths(c, T)


def test_cases_reach_their_paths():
    fam = lambda f: [c for c in LC.CASES if c["family"] == f]
    gram = fam("gram")
    assert {(c["B"], _paths(c)["gram_tiles"], _paths(c)["gram_tail"]) for c in gram} == {(1, 1, 1), (15, 1, 15), (16, 1, 0), (17, 2, 1), (33, 3, 1)}
    assert {(c["D"], _paths(c)["d_trips"], _paths(c)["d_tail"]) for c in gram} == {(1, 1, 1), (15, 1, 15), (16, 1, 0), (17, 2, 1), (130, 9, 2)}
    assert {(c["B"], _paths(c)["W"]) for c in gram} == {(1, 1), (15, 1), (15, 3), (16, 1), (17, 1), (33, 1), (33, 3)}
    for B in (1, 15, 16, 17, 33):
        for D in (1, 15, 16, 17, 130):
            kinds = {c["kind"] for c in gram if (c["B"], c["D"]) == (B, D)}
            assert "exact" in kinds and kinds & {"prod3", "prod4"}
    assert {(c["B"], _paths(c)["rowstats_trips"]) for c in fam("rowstats")} == {(255, 1), (256, 1), (257, 2)}
    for c in LC.CASES:
        p = _paths(c)
        assert p["dgram_passes"] == (2 if c["family"] == "dgram" else 1), c["name"]
        assert p["lds_bytes"] <= LC.LDS_LIMIT
        if c["family"] not in ("reduce", "ldslimit"):
            assert p["reduce_trips"] == 1
        if c["family"] not in ("rowstats", "dgram"):
            assert p["rowstats_trips"] == 1
    for c in fam("dgram"):
        p = _paths(c)
        assert p["dgram_grid"] == LC.DGRAM_MAX_GRID and c["B"] ** 2 - LC.DGRAM_MAX_GRID * LC.DGRAM_BLOCK == 1025
    assert {(c["D"], _paths(c)["dpooled_trips"]) for c in fam("dpooled")} == {(127, 1), (128, 1), (129, 2), (257, 3)}
    assert {(c["B"], tuple(_paths(c)["dpooled_slices"])) for c in fam("dpooled")} == {(1, (1, 0, 0, 0)), (2, (1, 1, 0, 0)), (3, (1, 1, 1, 0)), (4, (1, 1, 1, 1)),
                                                                                     (5, (2, 1, 1, 1))}
    sa, sb = {t[0] for t in LC.TERMS_DPOOLED}, {t[1] for t in LC.TERMS_DPOOLED}
    assert 1 in sa and 1 in sb and any(t[0] == t[1] for t in LC.TERMS_DPOOLED) and 3 not in sa | sb and fam("dpooled")[0]["R"] == 4
    for c in fam("reduce"):
        p = _paths(c)
        assert c["T"] == 60 and p["W"] == 5 and p["reduce_trips"] == 2
        kinds = {(bool(t[2]), bool(t[3])) for t in c["terms"]}
        assert kinds == {(True, False), (False, True), (True, True)}
        d, ref = prepared(c["name"])
        dead = (ref["n"] == 0)
        assert dead[:, 3].all() and dead[:, 1].any() and not dead[:, 1].all() and not dead[:, 2].any() and int(d["present"][9]) == 0
        assert float(ref["ranks"][3]["loss"]) == 0.0 and float(ref["ranks"][3]["loss_tol"]) == 0.0
    assert {_paths(c)["W"] for c in fam("ranks")} == {1, 2, 3}
    for c in fam("ldslimit"):
        assert _paths(c)["lds_bytes"] == LC.LDS_LIMIT == 60000 and c["T"] * _paths(c)["W"] == 5000
    r = LC.LDS_REFUSED
    assert 3 * r["T"] * (r["B"] // r["b_local"]) * 4 == 60480 > LC.LDS_LIMIT and r["T"] * r["B"] // r["b_local"] == 5040
    assert {c["terms"] for c in fam("schedule")} == {"schedule:mca", "schedule:bimodal", "schedule:zorro"} and all(c["B"] == 17 for c in fam("schedule"))


def test_data_is_what_the_cases_say():
    """exact: integer logits and a tied maximum in row 0 and column 0; production: the stated magnitude, which overflows expf unshifted,
    near one-hot softmax rows, and a finite float64 reference (asserted inside reference() for every case)"""
    for name in ("gram-B17D130R3b17-exact", "dpooled-B5D257R4b5-exact", "rowstats-B257D8R3b257-exact"):
        d, ref = prepared(name)
        l = ref["l"]
        assert torch.equal(l, l.round()) and float(d["s"]) == 0.0
        assert (l[:, 0] == l[:, 0].max(1, keepdim=True).values).sum(1).min() >= 2 and (l[:, :, 0] == l[:, :, 0].max(1, keepdim=True).values).sum(1).min() >= 2
    for name, target in (("gram-B33D130R3b11-prod3", 1e3), ("gram-B33D17R3b33-prod4", 1e4), ("rowstats-B257D8R3b257-prod4", 1e4)):
        d, ref = prepared(name)
        l = ref["l"]
        assert abs(float(l.abs().max()) / target - 1) < 1e-3 and float(l.max()) > 89          # expf(89) is inf in fp32
        top = torch.exp(l - torch.logsumexp(l, 2, keepdim=True)).max(2).values
        assert float(top.median()) > 0.99


# ------------------------------------------------------------------------------------------------ (d) every bound is satisfiable
@pytest.mark.parametrize("name", list(CASE))
def test_emulation_within_bounds(name):
    d, ref = prepared(name)
    common = U.emulate_common(d)
    for r in range(d["W"]):
        U.check(d, ref, r, U.emulate(d, r, common), common=r == 0)
    _cache.pop(name, None)


# the worst |emulation - reference| / bound over every case above, rounded up to the next 0.05 (docs/parity.md)
CAPS = {"loss lse_row": 0.65, "loss lse_col": 0.75, "loss ce": 0.55, "loss dsum": 0.20, "loss dG": 0.70, "loss term_loss": 0.50, "loss loss": 0.50,
        "loss d_logit_scale": 0.10, "loss d_pooled": 0.50, "loss d_pooled | dG": 0.60}


def test_worst_ratios_under_their_caps():
    """after test_emulation_within_bounds: a bound the restatement only just meets would not be one the kernels can be held to"""
    assert all(c < 1 for c in CAPS.values())
    seen = {k: v for k, v in U.WORST.items() if k in CAPS}
    for k in sorted(seen):
        print(f"worst |emulation - ref| / bound  {k:24s} {seen[k]:.3f}  (cap {CAPS[k]:.2f})")
    assert seen, "run after test_emulation_within_bounds"
    for k, v in seen.items():
        assert v <= CAPS[k], (k, v, CAPS[k])
