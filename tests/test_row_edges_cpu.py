"""The row-kernel edge tests, checked without a GPU (tests/row_edge_util.py, tests/row_cases.py):
(a) every listed LayerNorm case reaches the form, vector width, grid and slot count it is listed for (csrc/ln_plan.h through the
    mca_dbg_plan_layernorm_* hooks), and every form is reached with and without a second pass of its row loop;
(b) the helpers raise and name the (row, column) of each planted fault;
(c) every derived bound is satisfiable: an fp32 torch restatement of each kernel's formula, stored where the kernel stores, passes
    the very checks the GPU tests run, at every element of every case;
and the argument checks that need no launch."""
import ctypes as C
import importlib

import pytest
import torch

import row_cases as RC
import row_edge_util as U

BASE = 0x10000000          # a 256-byte aligned stand-in address: the planners read null-ness and alignment only
F32, BF = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def H():
    importlib.import_module("mca-paper_amd.build").build()
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def gen(seed=0):
    return torch.Generator().manual_seed(seed)


def ids(cases):
    return [c["name"] for c in cases]


# ------------------------------------------------------------------------------------------------ (a) plans
def fwd_plan(H, c):
    at = lambda on, off=0: BASE + off if on else 0
    pr = H.LnFwdProblem(rows=c["rows"], cols=c["cols"], cols_pad=c["cols_pad"], ldx=c["ldx"], ldy=c["ldy"] if c["y"] else 0,
                        y_bstride=(c["period"] + RC.PACK_EXTRA) * c["ldy"] if c["period"] else 0, ld_bf16=c["ld_bf16"] if c["ybf"] else 0, period=c["period"],
                        x=at(1, c["x_off"]), gamma=at(1, c["gamma_off"]), beta=at(c["beta"]), rowmask=at(c["mask"]), add=at(c["add"], c["add_off"]),
                        y=at(c["y"]), y_bf16=at(c["ybf"], c["ybf_off"]))
    p = H.LnFwdPlan()
    with H.knobs(**{f"k{k}": v for k, v in c["knobs"].items()}):
        assert H.lib().mca_dbg_plan_layernorm_fwd(C.byref(pr), C.byref(p)) == 0
    return dict(form=p.form, width=p.width, grid_x=p.grid_x, passes=p.passes)


def bwd_plan(H, c):
    at = lambda on, off=0: BASE + off if on else 0
    pr = H.LnBwdProblem(rows=c["rows"], cols=c["cols"], ldy=c["ldy"], y_bstride=(c["period"] + RC.PACK_EXTRA) * c["ldy"] if c["period"] else 0, period=c["period"],
                        ldx=c["ldx"], lddx=c["lddx"] if c["dx"] else 0, ld_bf16=c["ld_bf16"] if c["dxb"] else 0, dy=at(1), x=at(1, c["x_off"]),
                        gamma=at(1, c["gamma_off"]), rowmask=at(c["mask"]), dx=at(c["dx"]), dx_bf16=at(c["dxb"], c["dxb_off"]), dgamma=at(c["dgamma"]),
                        dbeta=at(c["dbeta"]), dxsum=at(c["dxsum"]))
    p = H.LnBwdPlan()
    with H.knobs(**{f"k{k}": v for k, v in c["knobs"].items()}):
        assert H.lib().mca_dbg_plan_layernorm_bwd(C.byref(pr), C.byref(p)) == 0
        scratch = H.lib().mca_layernorm_bwd_det_scratch(c["rows"], c["cols"])
    return dict(form=p.form, width=p.width, grid_x=p.grid_x, grid_y=p.grid_y, rows_per_block=p.rows_per_block, slots=p.slots, passes=p.passes), scratch


def test_plan_constants(H):
    assert (RC.NONE, RC.NARROW, RC.TRUNK, RC.GENERAL, RC.PARAMS) == (H.LN_NONE, H.LN_NARROW, H.LN_TRUNK, H.LN_GENERAL, H.LN_PARAMS)


@pytest.mark.parametrize("case", RC.LN_FWD, ids=ids(RC.LN_FWD))
def test_layernorm_fwd_case_reaches_its_plan(H, case):
    assert fwd_plan(H, case) == case["plan"]


@pytest.mark.parametrize("case", RC.LN_BWD, ids=ids(RC.LN_BWD))
def test_layernorm_bwd_case_reaches_its_plan(H, case):
    plan, scratch = bwd_plan(H, case)
    assert plan == case["plan"]
    assert scratch >= plan["slots"] * 3 * case["cols"] and scratch % (3 * case["cols"]) == 0          # the _det form's slots fit its scratch


def _literal(d, bwd):
    """a literal plan's call: 16-byte aligned pointers; vec_ld: leading dimensions of cols + 4 (else odd ones)"""
    cols, v = d["cols"], d.get("vec_ld", 0)
    if bwd:
        c = RC._bwd("literal", d["rows"], cols, RC.GENERAL, 1, **{k: d.get(k, 0) for k in ("dgamma", "dbeta", "dxsum", "dx", "dxb", "mask", "period")})
        c.update(ldx=cols + 4, ldy=cols + 4, lddx=cols + 4, ld_bf16=cols + 4) if v else None
    else:
        c = RC._fwd("literal", d["rows"], cols, RC.GENERAL, 1, **{k: d.get(k, 0) for k in ("ybf", "y", "beta", "mask")}, cols_pad=d.get("cols_pad", cols))
        c.update(ldx=cols + 4, ldy=cols + 4, ld_bf16=cols + 4) if v else None
    return c


def test_literal_plans(H):
    """the grid rules the case lists restate, pinned to numbers written down (the slot counts of tests/test_deterministic_gpu.py
    among them)"""
    for d, want in RC.LN_FWD_LITERAL:
        assert fwd_plan(H, _literal(d, False)) == want, d
    for d, want in RC.LN_BWD_LITERAL:
        assert bwd_plan(H, _literal(d, True))[0] == want, d


def test_every_form_with_and_without_a_second_pass():
    fwd = {(c["plan"]["form"], c["plan"]["width"], c["plan"]["passes"] > 1) for c in RC.LN_FWD}
    # (the trunk forward has no row loop: a workgroup per eight rows; its 256-column instantiation is shadowed by the narrow form)
    assert fwd == {(RC.NARROW, 0, False), (RC.NARROW, 0, True), (RC.TRUNK, 2, False), (RC.TRUNK, 4, False),
                   (RC.GENERAL, 1, False), (RC.GENERAL, 1, True), (RC.GENERAL, 4, False), (RC.GENERAL, 4, True)}
    bwd = {(c["plan"]["form"], c["plan"]["width"], c["plan"]["passes"] > 1) for c in RC.LN_BWD}
    assert bwd == {(f, w, s) for f, ws in ((RC.PARAMS, (64, 128, 256)), (RC.TRUNK, (1, 2, 4)), (RC.GENERAL, (1, 4))) for w in ws for s in (False, True)}
    # a partial last slab of the parameter form, and an odd last row in the trunk form's second pass
    assert any(c["plan"]["form"] == RC.PARAMS and c["rows"] % c["plan"]["rows_per_block"] for c in RC.LN_BWD)
    assert any(c["plan"]["form"] == RC.TRUNK and c["plan"]["passes"] == 2 and c["rows"] % 2 for c in RC.LN_BWD)


def test_alignment_rule_of_the_vector_forms(H):
    """the one deliberate change of the dispatch: an 8-byte store needs an 8-byte aligned y_bf16 / dx_bf16; add is read as scalars"""
    base = next(c for c in RC.LN_FWD if c["name"] == "vec-shapes-ybf+2-scalar")
    for off, width in ((0, 4), (2, 1), (4, 1), (6, 1), (8, 4)):
        assert fwd_plan(H, dict(base, ybf_off=off))["width"] == width
    assert fwd_plan(H, dict(base, ybf_off=2, ybf=0, ld_bf16=0))["width"] == 4          # no y_bf16: nothing to align
    for off in (0, 4, 8, 12):
        assert fwd_plan(H, dict(base, ybf_off=0, add=1, add_off=off))["width"] == 4
    b = next(c for c in RC.LN_BWD if c["name"] == "vec-shapes-dxb+2-scalar")
    for off, width in ((0, 4), (2, 1), (4, 1), (8, 4)):
        assert bwd_plan(H, dict(b, dxb_off=off))[0]["width"] == width


# ------------------------------------------------------------------------------------------------ (c) the bounds are satisfiable
@pytest.mark.parametrize("case", RC.LN_FWD, ids=ids(RC.LN_FWD))
def test_layernorm_fwd_bounds_satisfiable(case):
    g = gen(3)
    T = U.ln_fwd_setup(case, g)
    O = U.ln_fwd_outputs(case, T, True, "cpu")
    U.ln_fwd_emulate_into(case, T, O)
    stats = U.ln_fwd_check(case, T, O)
    if not case["stats"]:
        O = U.ln_fwd_outputs(case, T, False, "cpu")
        U.ln_fwd_emulate_into(case, T, O)
        U.ln_fwd_check(case, T, O, stats)


@pytest.mark.parametrize("case", RC.LN_BWD, ids=ids(RC.LN_BWD))
def test_layernorm_bwd_bounds_satisfiable(case):
    T = U.ln_bwd_setup(case, gen(4))
    O = U.ln_bwd_outputs(case, T, "cpu")
    U.ln_bwd_emulate_into(case, T, O)
    U.ln_bwd_check(case, T, O)


@pytest.mark.parametrize("n", [1, 255, 257, 70001])
@pytest.mark.parametrize("max_norm", [0.0, 1.0, 1e6])
def test_adamw_bounds_satisfiable(n, max_norm):
    g = gen(5)
    p, gr, m = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    v = torch.rand(n, generator=g) * 0.01
    hp = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, max_norm=max_norm)
    for step in (1, 2, 3):
        sq = float((gr.double() ** 2).sum().float())
        bc = dict(bc1=1 - 0.9 ** step, bc2=1 - 0.999 ** step)
        ref = U.adamw_ref(p, gr, m, v, sq, **hp, **bc)
        p, m, v = U.adamw_emulate32(p, gr, m, v, sq, **hp, **bc)
        for k, t in (("m", m), ("v", v), ("p", p)):
            U.assert_close_rows(t, *ref[k], f"step {step}: {k}")
        gr = torch.randn(n, generator=g)


def test_tab_value_bounds_satisfiable():
    g = gen(6)
    rows, cols = 1030, 520
    x = torch.randn(rows, generator=g) * 3
    x[::7], x[3::11] = -1.0, 9.0
    w1, b1 = torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    ref, tol, pm = U.tab_value_fwd_ref(x, w1, b1, 5.0, -1.0)
    h1 = torch.clamp_min(torch.minimum(x, torch.tensor(5.0))[:, None] * w1[None, :] + b1[None, :], 0).to(BF)
    U.assert_close_elementwise(h1, ref, tol, "h1")
    assert pm.sum() == (x == -1.0).sum() > 0
    dh1 = torch.randint(-4, 5, (rows, cols), generator=g).float()
    iw, ib = torch.randint(-3, 4, (cols,), generator=g).float(), torch.randint(-3, 4, (cols,), generator=g).float()
    (dw, tolw), db = U.tab_value_bwd_ref(dh1, h1, x, 5.0, iw, ib)
    gsel = torch.where(h1.float() > 0, dh1, torch.zeros(()))
    U.assert_close_rows(iw + (gsel * torch.minimum(x, torch.tensor(5.0))[:, None]).sum(0), dw, tolw, "dw1")
    U.assert_exact_rows(ib + gsel.sum(0), db.float(), "db1")


# ------------------------------------------------------------------------------------------------ (b) planted faults
FAULT_FWD = next(c for c in RC.LN_FWD if c["name"] == "vec-260x5-packed")


def fwd_emulated(case=FAULT_FWD):
    T = U.ln_fwd_setup(case, gen(7))
    O = U.ln_fwd_outputs(case, T, True, "cpu")
    U.ln_fwd_emulate_into(case, T, O)
    return T, O


def test_fault_free_emulation_passes_and_frames_hold():
    T, O = fwd_emulated()
    U.ln_fwd_check(FAULT_FWD, T, O)
    assert FAULT_FWD["ldx"] > FAULT_FWD["cols"] and T["mask"].sum() > 0 and torch.isnan(T["x"][T["mask"].bool()]).all()
    w = torch.as_strided(T["x"], (FAULT_FWD["rows"], FAULT_FWD["ldx"]), (FAULT_FWD["ldx"], 1), T["x"].storage_offset())
    assert torch.isnan(w[:, FAULT_FWD["cols"]:]).all()


def test_fault_one_element_a_bf16_step_off():
    T, O = fwd_emulated()
    r = int((T["mask"] == 0).nonzero()[-1])
    col = int(O["ybf"].t[r, :FAULT_FWD["cols"]].float().abs().argmax())          # a large element: the fp32 part of its bound is far below a step
    O["ybf"].t.view(torch.int16)[r, col] += 2
    with pytest.raises(AssertionError, match=rf"y_bf16: 1 of \d+ elements wrong.*\({r}, {col},"):
        U.ln_fwd_check(FAULT_FWD, T, O)


def test_fault_one_stale_element():
    T, O = fwd_emulated()
    O["y"].t.view(torch.int32)[T["dest"][3], 259] = -1          # never stored: still the sentinel
    with pytest.raises(AssertionError, match=r"y: 1 of \d+ elements wrong.*\(3, 259,"):
        U.ln_fwd_check(FAULT_FWD, T, O)


def test_fault_store_into_a_guard():
    T, O = fwd_emulated()
    O["ybf"].buf[O["ybf"].start + (2 * FAULT_FWD["ld_bf16"] + FAULT_FWD["cols_pad"]) * 2] = 0          # row 2, first column past cols_pad
    with pytest.raises(AssertionError, match=rf"ybf: \d+ guard bytes overwritten.*\(2, {FAULT_FWD['cols_pad']}\)"):
        U.ln_fwd_check(FAULT_FWD, T, O)
    T, O = fwd_emulated()
    gap = next(r for r in range(T["y_rows"]) if r not in set(T["dest"]))
    O["y"].t[gap, 5] = 1.0          # a row of the packed placement that belongs to another modality
    with pytest.raises(AssertionError, match=rf"rows no kernel row maps to; first \(row, column\): \({gap}, 5\)"):
        U.ln_fwd_check(FAULT_FWD, T, O)
    T, O = fwd_emulated()
    O["ybf"].t[1, FAULT_FWD["cols"] + 3] = 1.0          # columns [cols, cols_pad) are exactly 0
    with pytest.raises(AssertionError, match=r"columns \[cols, cols_pad\): 1 of \d+ elements wrong.*\(1, 3,"):
        U.ln_fwd_check(FAULT_FWD, T, O)


def test_fault_read_of_a_nan_pad():
    """a kernel that walks one column too far reads the NaN frame: its statistics are NaN and the first check names the row"""
    case = next(c for c in RC.LN_FWD if c["name"] == "narrow-74x17-b0m0-pad74" or c["name"].startswith("narrow-74x17"))
    T = U.ln_fwd_setup(case, gen(8))
    O = U.ln_fwd_outputs(case, T, True, "cpu")
    wide = torch.as_strided(T["x"], (case["rows"], case["cols"] + 1), (case["ldx"], 1), T["x"].storage_offset())
    T2 = dict(T, x=wide)
    mean, rstd, _, yb = U.ln_fwd_emulate32(wide, torch.cat([T["gamma"], T["gamma"][:1]]), None, None, T["mask"])
    O["mean"].t[0].copy_(mean), O["rstd"].t[0].copy_(rstd), O["ybf"].t[:, :case["cols"]].copy_(yb[:, :case["cols"]])
    O["ybf"].t[:, case["cols"]:] = 0
    assert T2 is not T
    with pytest.raises(AssertionError, match=r"mean .*elements wrong.*\(0, 0,"):
        U.ln_fwd_check(case, T, O)


def test_fault_leaked_nan_from_a_masked_row():
    """a backward that loads a masked row: its dgamma column sums turn NaN, and so does the row's dx"""
    case = next(c for c in RC.LN_BWD if c["cols"] == 260 and c["rows"] > 1 and c["mask"] and c["dx"] and c["dgamma"] and c["dbeta"])
    T = U.ln_bwd_setup(case, gen(9))
    O = U.ln_bwd_outputs(case, T, "cpu")
    U.ln_bwd_emulate_into(case, T, O)
    U.ln_bwd_check(case, T, O)
    r = int(T["mask"].nonzero()[0])
    O["dx"].t[r, 17] = float("nan")
    with pytest.raises(AssertionError, match=rf"dx: 1 of \d+ elements wrong.*\({r}, 17,"):
        U.ln_bwd_check(case, T, O)
    U.ln_bwd_emulate_into(case, T, O)
    O["dgamma"].t[0, 259] = float("nan")
    with pytest.raises(AssertionError, match=r"dgamma .*1 of 260 elements wrong.*\(0, 259,"):
        U.ln_bwd_check(case, T, O)
    U.ln_bwd_emulate_into(case, T, O)
    O["dbeta"].t[0, 0] += 1          # one row's dy counted twice: integers, so any difference is an error
    with pytest.raises(AssertionError, match=r"dbeta .*1 of 260 elements wrong.*\(0, 0,"):
        U.ln_bwd_check(case, T, O)


def test_fault_masked_row_must_be_exactly_zero():
    T, O = fwd_emulated()
    r = int(T["mask"].nonzero()[0])
    O["ybf"].t.view(torch.int16)[r, 0] = 1          # the smallest bf16 denormal
    with pytest.raises(AssertionError, match=rf"y_bf16: 1 of \d+ elements wrong.*\({r}, 0,"):
        U.ln_fwd_check(FAULT_FWD, T, O)
    T, O = fwd_emulated()
    O["mean"].t[0, r] = 1e-30
    with pytest.raises(AssertionError, match=rf"mean .*\(0, {r},"):
        U.ln_fwd_check(FAULT_FWD, T, O)


# ------------------------------------------------------------------------------------------------ argument checks (no launch)
def test_argument_checks(H):
    L = H.lib()
    out = U.guarded_out(4, 8, 12, F32)
    bf = U.guarded_out(4, 8, 12, BF)
    src = torch.zeros(64)
    p, q, b = src.data_ptr(), out.data_ptr(), bf.data_ptr()
    BAD = -1
    ln_f = lambda rows, cols: L.mca_layernorm_fwd(p, 8, p, None, None, None, 0, q, 12, 0, b, 12, 8, None, None, rows, cols, 1e-5, None)
    ln_b = lambda rows, cols: L.mca_layernorm_bwd(p, 8, 0, 0, p, 8, p, p, p, None, q, 12, b, 12, p, None, None, rows, cols, None)
    for f in (ln_f, ln_b):
        assert f(4, 0) == BAD and f(4, 1025) == BAD and f(-1, 8) == BAD
        assert f(0, 8) == 0
    need = L.mca_layernorm_bwd_det_scratch(4, 8)
    assert need == 3 * 8
    det = lambda rows, sf: L.mca_layernorm_bwd_det(p, 8, 0, 0, p, 8, p, p, p, None, q, 12, b, 12, p, None, None, rows, 8, p, sf, None)
    assert det(4, need - 1) == BAD and det(0, 0) == 0
    assert L.mca_geglu_fwd(b, b, 4, 12, None) == BAD and L.mca_geglu_bwd(b, b, b, 4, 12, None) == BAD and L.mca_geglu_fwd(b, b, 0, 8, None) == 0
    assert L.mca_tab_value_fwd(p, p, p, b, b, 4, 12, 1.0, -1.0, None) == BAD
    fa = H.FiniteArgs()
    fa.p[0], fa.n[0], fa.count = p, 4, 1
    assert L.mca_nonfinite_flag(C.byref(fa), q, 0, None) == BAD
    assert L.mca_reduce_rows_det_scratch(10, 3, 8) == 4 * 3 * 8
    assert L.mca_reduce_rows_det(p, 8, 24, 3, q, 12, 10, 8, p, 4 * 3 * 8 - 1, None) == BAD
    assert L.mca_tab_value_bwd_det_scratch(4, 8) == 4 * 2 * 8
    assert L.mca_tab_value_bwd_det(p, 8, b, p, q, q, 4, 8, 1.0, p, 4 * 2 * 8 - 1, None) == BAD
    assert L.mca_f32_to_bf16(p, 8, b, 12, 0, 8, 1.0, None) == 0 and L.mca_bcast_rows(p, 8, q, 12, 0, 1, 0, 8, None) == 0
    assert L.mca_reduce_rows(p, 8, 0, 1, q, 12, 0, 8, None) == 0 and L.mca_rows_copy_add(p, 0, q, 0, 0, 8, 1, 0, None) == 0
    U.assert_guard_intact(out, "fp32 output of refused and empty calls")
    U.assert_guard_intact(bf, "bf16 output of refused and empty calls")
    assert (out.t.view(torch.int32) == -1).all() and (bf.t.view(torch.int16) == -1).all()          # and the views themselves


def test_fault_frame_nan_carried_into_a_guard():
    """a kernel that reads one row too many and stores one row too many carries the input frame's NaN, bits intact, into the output's
    guard: seen only because the two frames hold different NaNs (U.framed_in)"""
    case = FAULT_FWD
    T, O = fwd_emulated()
    x_guard = torch.as_strided(T["x"], (1, case["cols"]), (case["ldx"], 1), T["x"].storage_offset() + case["rows"] * case["ldx"])
    assert torch.isnan(x_guard).all()
    y_guard = torch.as_strided(O["y"].t, (1, case["cols"]), (case["ldy"], 1), O["y"].t.storage_offset() + T["y_rows"] * case["ldy"])
    y_guard.copy_(x_guard + x_guard)          # arithmetic keeps a NaN's bits
    with pytest.raises(AssertionError, match=rf"y: \d+ guard bytes overwritten.*\({T['y_rows']}, 0\)"):
        U.ln_fwd_check(case, T, O)
    T, O = fwd_emulated()
    b_guard = torch.as_strided(O["ybf"].t, (1, case["cols"]), (case["ld_bf16"], 1), O["ybf"].t.storage_offset() + case["rows"] * case["ld_bf16"])
    b_guard.view(torch.int16).copy_(x_guard.view(torch.int32) >> 16)          # the truncating side of a bf16 rounding
    with pytest.raises(AssertionError, match=rf"ybf: \d+ guard bytes overwritten.*\({case['rows']}, 0\)"):
        U.ln_fwd_check(case, T, O)


def test_print_worst_ratios():
    """last in the file: how much of each bound the fp32 restatements use over all cases (pytest -s shows it)"""
    for k in sorted(U.WORST):
        print(f"worst |emulation - ref| / bound  {k:24s} {U.WORST[k]:.3f}")
    assert U.WORST
