"""Which GEMM kernel runs, as checked facts (no GPU): the library's planners (csrc/gemm_plan.h through the mca_dbg_plan_gemm_*
hooks) against the dispatch recorded from the code before them, the grouped weight gradient's row partition, and what the GEMM
shape lists of the GPU tests reach."""
import ctypes as C
import importlib
import json
import os
import shutil
import subprocess

import pytest

import gemm_shapes as GS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 0x10000000          # a 256-byte aligned stand-in address: the planners read null-ness and alignment only


@pytest.fixture(scope="module")
def H():
    importlib.import_module("mca-paper_amd.build").build()
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def kernel_name(H, plan):
    return H.lib().mca_dbg_gemm_kernel_name(plan.kernel).decode()


def plan_call(H, call, cus=256, knobs=None):
    """The plan of one call dict (gemm_shapes): (return code, GemmPlan | TnGroupPlan)."""
    L = H.lib()
    with H.knobs(**{f"k{k}": v for k, v in (knobs or {}).items()}):
        e = call["entry"]
        if e == "tn":
            p = H.GemmPlan()
            return L.mca_dbg_plan_gemm_tn(call["R"], call["N"], call["K"], C.byref(p)), p
        if e == "tn_group":
            n = len(call["members"])
            N, K = (C.c_int64 * n)(*[m[0] for m in call["members"]]), (C.c_int64 * n)(*[m[1] for m in call["members"]])
            p = H.TnGroupPlan()
            return L.mca_dbg_plan_gemm_tn_group(N, K, n, call["R"], cus, C.byref(p)), p
        pr = H.NtProblem(M=call["M"], N=call["N"], K=call["K"])
        if e == "nt":
            pr.out_bf16, pr.res_period = call["out_bf16"], 16 if call["res"] == 2 else 0
            pr.C, pr.ldc = BASE + call["c_off"], call["ldc"]
            pr.residual, pr.ldres = (BASE + call["res_off"] if call["res"] else 0), call["ldres"]
            pr.bias = BASE + call["bias_off"] if call["bias"] else 0
        entry = {"nt": H.PLAN_NT, "lnres": H.PLAN_LNRES, "geglu_fwd": H.PLAN_GEGLU_FWD, "geglu_bwd": H.PLAN_GEGLU_BWD}[e]
        p = H.GemmPlan()
        return L.mca_dbg_plan_gemm_nt(entry, C.byref(pr), cus, C.byref(p)), p


def as_launch(H, p, rows, K):
    """a plan in the recorded form: kernel, grid, block, LDS bytes and the kernel's integer arguments"""
    name = kernel_name(H, p)
    if name.startswith("gemm_tn"):
        ints = [rows, p.n, K, p.tiles_k, p.rows_per_split, p.dbg]
    else:
        ints = [rows, p.n, K, p.tiles_n, p.nwg] + ([p.dbg] if "persist" in name else [])
    return {"kernel": name, "grid": [p.grid_x, p.grid_y], "block": p.block, "lds": p.lds_bytes, "ints": ints}


def planned_launches(H, call, cus, knobs):
    """what the entry point would launch, launch by launch (the fall-backs are calls of another entry point)"""
    rc, p = plan_call(H, call, cus, knobs)
    if rc != 0:
        return rc, []
    e = call["entry"]
    if e == "tn":
        return 0, [as_launch(H, p, call["R"], call["K"])]
    if e == "tn_group":
        if p.grouped < 0:
            return p.grouped, []
        if not p.grouped:
            return 0, [planned_launches(H, GS.tn(call["R"], n, k), cus, knobs)[1][0] for n, k in call["members"]]
        tiles_k = [(k + 255) // 256 for _, k in call["members"]]
        first = [0]
        for (n, _), tk in zip(call["members"], tiles_k):
            first.append(first[-1] + (n + 255) // 256 * tk)
        assert first[-1] == p.part.tiles
        pt, ln = p.part, p.launch
        return 0, [{"kernel": kernel_name(H, ln), "grid": [ln.grid_x, ln.grid_y], "block": ln.block, "lds": ln.lds_bytes, "ints": [ln.dbg],
                    "group": dict(n=len(tiles_k), R=pt.R, tiles=pt.tiles, unit=pt.unit, n_full=pt.n_full, span=pt.span, own=pt.own,
                                  first_tile=first, tiles_k=tiles_k)}]
    if e == "geglu_fwd" and p.kernel == 0:          # the unfused pair: the plain GEMM over both halves (+ mca_geglu_fwd)
        return planned_launches(H, GS.nt(call["M"], 2 * call["N"], call["K"], out_bf16=1), cus, knobs)
    return 0, [as_launch(H, p, call["M"], call["K"])]


@pytest.fixture(scope="module")
def table():
    return json.load(open(os.path.join(REPO, "tests", "golden", "gemm_dispatch.json")))


def test_plans_equal_the_recorded_dispatch(H, table):
    """tests/golden/gemm_dispatch.json: kernel, grid, block, LDS bytes and integer kernel arguments of every launch, printed by the
    entry points' own decision code as it stood before the planners existed (commit 142a0d4), compiled on a CPU with the launch
    replaced by a print."""
    for row in table:
        case = row["case"]
        rc, launches = planned_launches(H, case, case["cus"], {int(k): v for k, v in case["knobs"].items()})
        assert rc == row["rc"] and launches == row["launches"], (case, rc, launches, row)


def test_recorded_dispatch_covers_the_suite_the_step_and_the_knobs(table):
    cases = [r["case"] for r in table]
    def has(call, cus, knobs=None):
        return dict(call, knobs={str(k): v for k, v in (knobs or {}).items()}, cus=cus) in cases
    from importlib import import_module
    S = import_module("mca-paper_amd.structure")
    assert S.FusionStructure([1500, 450, 450, 50], 88, (4, 3, 2), fcl=True).n_tokens == GS.CMU_TOKENS
    assert S.FusionStructure([1500] * 4, 88, (4, 3, 2), fcl=True).n_tokens == GS.LONG_TOKENS
    for cus in (256, 64):
        assert all(has(c, cus) for c in GS.suite_calls())
        assert all(has(c, cus) for T in GS.STEP_ROWS.values() for c in GS.step_calls(T))
    for k, v in [(1, 1), (3, 3), (4, 1), (5, 1), (5, 2), (6, 1), (6, 49), (6, -49), (7, 1), (7, 3), (10, 1), (11, 1)]:
        assert all(has(c, 256, {k: v}) for c in GS.step_calls(GS.STEP_ROWS["cmu_b32"])), (k, v)
    nt = [c for c in cases if c["entry"] == "nt"]
    assert {(c["out_bf16"], c["res"], c["bias"]) for c in nt} == {(o, r, b) for o in (0, 1) for r in (0, 1, 2) for b in (0, 1)}
    assert any(c["c_off"] % 16 for c in nt) and any(c["ldc"] % 4 for c in nt) and any(c["res_off"] % 16 for c in nt)


# ---- what the GPU tests' shapes reach: every kernel but the ones only a knob selects
KNOB_ONLY = {"gemm_nt_persist_kernel<2,false>", "gemm_nt_persist_kernel<2,true>"}          # knob 7 = 3 (A/B of the fp32 + residual form)

def reached(H, calls, cus=256, knobs=None):
    return {l["kernel"] for c in calls for l in planned_launches(H, c, cus, knobs)[1]}


def test_gemm_test_shapes_reach_every_production_kernel(H):
    every = {H.lib().mca_dbg_gemm_kernel_name(k).decode() for k in range(1, 31)}
    assert len(every) == 30 and H.lib().mca_dbg_gemm_kernel_name(31) == b"?"
    got = reached(H, GS.suite_calls())
    assert got == every - KNOB_ONLY, (sorted(every - KNOB_ONLY - got), sorted(got & KNOB_ONLY))


def test_gemm_test_shapes_have_the_properties_their_comments_claim(H):
    one = lambda call, **kn: planned_launches(H, call, 256, kn)[1]
    # persistent kernels, grouped column tiles (more than one group of PS_PANELS = 4 row panels)
    for M, N, K in [(4100, 1536, 320), (2600, 2816, 512)]:
        (l,) = one(GS.nt(M, N, K))
        assert l["kernel"] == "gemm_nt_persist_kernel<1,false>" and (M + 255) // 256 > 4
    # the bf16, no-bias 256 x 128 persistent kernel: N a multiple of 128 and not of 256
    (l,) = one(GS.nt(2100, 384, 320, out_bf16=1))
    assert l["kernel"] == "gemm_nt_persist_kernel<0,false>"
    # 280 tiles of 256 x 256 on 256 CUs: second tile per workgroup; the shortest k-loop the kernel takes
    for M, N, K in [(17920, 1024, 192), (17700, 1024, 256)]:
        (l,) = one(GS.nt(M, N, K, out_bf16=1))
        assert l["kernel"] == "gemm_nt_persist256_kernel<false>" and l["ints"][4] == 280 and l["grid"] == [256, 1]
    assert one(GS.nt(17920, 1024, 128, out_bf16=1))[0]["kernel"] != "gemm_nt_persist256_kernel<false>"
    # fused GEGLU forward, 363 tiles: a second tile per workgroup, in both persistent kernels
    (l,) = one(GS.fused("geglu_fwd", 8200, 1408, 192))
    assert l["kernel"] == "gemm_nt_persist256_kernel<true>" and l["ints"][4] == 363 and l["grid"] == [256, 1]
    (l,) = one(GS.fused("geglu_fwd", 2304, 448, 320))
    assert l["kernel"] == "gemm_nt_persist_kernel<4,false>"
    # fused GEGLU backward: the 256-row kernels from 40,960 rows on
    assert one(GS.fused("geglu_bwd", 41100, 384, 512))[0]["kernel"] == "gemm_nt_persist_kernel<3,false>"
    assert one(GS.fused("geglu_bwd", 41100, 384, 128))[0]["kernel"] == "gemm_nt_256_kernel<true,0,0,1>"
    assert one(GS.fused("geglu_bwd", 4100, 384, 512))[0]["kernel"] == "gemm_nt_glds_kernel<true,0,64,1>"
    # grouped weight gradient: 52 tiles = 4 whole splits + 48 spans; 48 tiles; a member the kernel does not take; too few rows
    R, ms = GS.TN_GROUP[1]
    (l,) = one(GS.tn_group(R, ms))
    g = l["group"]
    assert (g["tiles"], g["n_full"], l["grid"][0] - g["n_full"] * g["tiles"]) == (52, 4, 48)
    (l,) = one(GS.tn_group(*GS.TN_GROUP[0]))
    assert l["group"]["tiles"] == 48 and l["kernel"] == "gemm_tn_256x256_group_kernel"
    for R, ms in GS.TN_GROUP[4:]:
        ls = one(GS.tn_group(R, ms))
        assert len(ls) == len(ms) and all(l["kernel"] != "gemm_tn_256x256_group_kernel" for l in ls)
    # ... and with knob 3 (the test's second pass): uniform splits, no line
    for R, ms in GS.TN_GROUP[:4]:
        (l,) = one(GS.tn_group(R, ms), **{"3": GS.TN_GROUP_UNIFORM_SPLITS})
        assert l["group"]["span"] == 0 and l["grid"][0] == l["group"]["n_full"] * l["group"]["tiles"]


def test_gemm_edge_shapes_reach_what_they_are_listed_for(H):
    """the edge cases of tests/test_gemm_edges_gpu.py (gemm_shapes.EDGE_*), 256 CUs, all knobs 0"""
    one = lambda call, **kn: planned_launches(H, call, 256, kn)[1]
    name = lambda family, ob, res, tail: f"{family}<{'true' if ob else 'false'},{res},{tail}>"
    cases = {c["name"]: c for c in GS.EDGE_NT}
    assert len(cases) == len(GS.EDGE_NT)
    kernels = lambda case: [one(c)[0] for c in GS.edge_nt_calls(cases[case])]
    forms = lambda case: cases[case]["forms"]
    # the 128 x 128 kernel: one or two k-steps, a row tail, a column tile that ends inside a 4- and an 8-element piece (70) or
    # right behind a whole one (136 = 128 + 8); with ld = 70 a row's pointer is 16-byte aligned every second (fp32) / fourth (bf16) row
    for case in ("glds_tails", "glds_tails_periodic", "glds_strides"):
        c = cases[case]
        assert [l["kernel"] for l in kernels(case)] == [name("gemm_nt_glds_kernel", ob, res, "64,0") for ob, res, _ in forms(case)]
        assert c["M"] < 2048 and c["M"] % 128 in (2, 16) and c["N"] % 128 in (70, 8) and c["K"] in (64, 128)
    assert cases["glds_tails"]["ldc"] * 4 % 16 == 8 and cases["glds_tails"]["ldc"] * 2 % 16 == 12 and len(forms("glds_tails")) == 6
    assert len(forms("glds_tails_periodic")) == 8 and 70 % 4 and 70 % 8 and 136 % 128 == 8
    c = cases["glds_strides"]
    assert c["K"] < c["lda"] < c["ldb"] and c["N"] < c["ldres"] < c["ldc"] and all(l["grid"] == [4, 1] for l in kernels("glds_strides"))
    # the 3-stage 256-row kernel with one and two k-steps (it prefetches two ahead), N tail 8 and row tail 2; misaligned C,
    # residual and bias leave it on the plain <.., 0, 0> forms
    for case in ("nt256_k64", "nt256_k128", "nt256_k64_periodic", "nt256_c_misaligned", "nt256_res_bias_misaligned", "encoder_projection"):
        c = cases[case]
        assert [l["kernel"] for l in kernels(case)] == [name("gemm_nt_256_kernel", ob, res, "0,0") for ob, res, _ in forms(case)], case
        assert c["K"] // 64 <= 2 and c["M"] >= 2048 and all(l["grid"] == [(c["M"] + 255) // 256 * ((c["N"] + 127) // 128), 1] for l in kernels(case))
    assert len(forms("nt256_k64")) == 6 and len(forms("nt256_k64_periodic")) == 8 and cases["nt256_k64"]["N"] % 128 == 8
    # ... which an aligned C with the same strides would not all be: the planner's c16 / res16 branches decide
    c = cases["nt256_c_misaligned"]
    assert c["c_off"] == 1 and c["ldc"] % 8 == 0 and cases["nt256_res_bias_misaligned"]["res_off"] % 16 == 4
    assert one(GS.nt(2050, 256, 320, out_bf16=1, ldc=264))[0]["kernel"] == "gemm_nt_persist256_kernel<false>"
    assert one(GS.nt(2050, 256, 320, out_bf16=1, ldc=264, c_off=2))[0]["kernel"] == "gemm_nt_256_kernel<true,0,0,0>"
    # the residual prefetch, with strides; a misaligned residual falls back to the form without it
    assert {l["kernel"] for l in kernels("nt256_prefetch_strided")} == {"gemm_nt_256_kernel<false,1,1,0>"}
    assert {l["kernel"] for l in kernels("nt256_prefetch_refused")} == {"gemm_nt_256_kernel<false,1,0,0>"}
    assert cases["nt256_prefetch_strided"]["ldc"] == 132 == cases["nt256_prefetch_strided"]["ldres"]
    # the 256 x 128 persistent kernel, modes 0 and 1 without and with bias: 9 tiles, and 261 on a grid of 256
    want = ["gemm_nt_persist_kernel<0,false>", "gemm_nt_persist_kernel<0,true>", "gemm_nt_persist_kernel<1,false>", "gemm_nt_persist_kernel<1,true>"]
    for case, tiles in (("persist_9_tiles", 9), ("persist_261_tiles", 261)):
        ls = kernels(case)
        assert [l["kernel"] for l in ls] == want and all(l["ints"][4] == tiles and l["grid"] == [min(tiles, 256), 1] for l in ls)
        assert cases[case]["ldc"] == cases[case]["N"] + 8 and cases[case]["K"] == 320          # its shortest k-loop
    (l,) = kernels("persist256_261_tiles")
    assert l["kernel"] == "gemm_nt_persist256_kernel<false>" and l["ints"][4] == 261 and l["grid"] == [256, 1] and cases["persist256_261_tiles"]["K"] == 192
    # fused LayerNorm residual: the smallest shape the entry point takes
    (M, N, K, _, _), = GS.EDGE_NT_LNRES
    assert one(GS.fused("lnres", M, N, K))[0]["kernel"] == "gemm_nt_256_kernel<false,1,1,2>"
    for smaller in ((2047, N, K), (M, N - 64, K), (M, N, K - 64)):
        assert plan_call(H, GS.fused("lnres", *smaller))[0] == -3
    # fused GEGLU forward: the 256 x 256 kernel with 9 and 261 tiles, mode 4, and the unfused pair (the plain GEMM over both halves)
    got = [one(GS.fused("geglu_fwd", *s))[0] for s in GS.EDGE_GEGLU_FWD]
    assert [l["kernel"] for l in got] == ["gemm_nt_persist256_kernel<true>", "gemm_nt_persist256_kernel<true>", "gemm_nt_persist_kernel<4,false>",
                                          "gemm_nt_256_kernel<true,0,0,0>"]
    assert [l["ints"][4] for l in got[:3]] == [9, 261, 27] and got[3]["ints"][1] == 2 * 72
    assert plan_call(H, GS.fused("geglu_fwd", *GS.EDGE_GEGLU_FWD[3]))[1].kernel == 0
    # fused GEGLU backward: 128 x 128 with an ip tail, the 256-row kernel, persistent mode 3 with 161 and 322 tiles
    got = [one(GS.fused("geglu_bwd", *s))[0] for s in GS.EDGE_GEGLU_BWD]
    assert [l["kernel"] for l in got] == ["gemm_nt_glds_kernel<true,0,64,1>", "gemm_nt_256_kernel<true,0,0,1>", "gemm_nt_persist_kernel<3,false>",
                                          "gemm_nt_persist_kernel<3,false>"]
    assert got[0]["grid"] == [2, 1] and got[2]["ints"][4] == 161 and got[3]["ints"][4] == 322 and got[3]["grid"] == [256, 1]
    # weight gradients: fewer rows than one split; 2 splits x 2 tiles; 17 splits, the last one of 4 rows, N tail 8; 12 tiles, both tails
    got = [one(GS.tn(R, N, K))[0] for R, N, K, _, _ in GS.EDGE_TN]
    assert [l["kernel"] for l in got] == ["gemm_tn_kernel", "gemm_tn_kernel", "gemm_tn_256_kernel", "gemm_tn_256x256_kernel"]
    assert got[0]["grid"] == [1, 1] and got[0]["ints"][4] > 70
    assert got[1]["grid"] == [2, 2]
    assert got[2]["grid"][1] == 17 and 4100 - 16 * got[2]["ints"][4] == 4 and 520 % 256 == 8
    assert got[3]["grid"][0] == 12 and 776 % 256 == 8 and 520 % 256 == 8
    # grouped: 26 tiles = 2 whole splits of 1,664 rows + 157 span workgroups of the minimum span (the 26 x 772 rows left); knob 3: uniform splits
    (R, ms), = GS.EDGE_TN_GROUP
    (l,) = one(GS.tn_group(R, ms))
    g = l["group"]
    assert l["kernel"] == "gemm_tn_256x256_group_kernel" and (g["tiles"], g["n_full"], g["span"]) == (26, 2, 128)
    assert l["grid"][0] - g["n_full"] * g["tiles"] == 157 == -(-26 * (R - 2 * g["unit"]) // 128)
    (l,) = one(GS.tn_group(R, ms), **{"3": GS.TN_GROUP_UNIFORM_SPLITS})
    assert l["group"]["span"] == 0 and l["grid"][0] == l["group"]["n_full"] * 26
    # every kernel family is reached by an edge case as well
    fam = {k.split("<")[0] for k in reached(H, GS.edge_calls())}
    assert fam == {"gemm_nt_glds_kernel", "gemm_nt_256_kernel", "gemm_nt_persist_kernel", "gemm_nt_persist256_kernel", "gemm_tn_kernel",
                   "gemm_tn_256_kernel", "gemm_tn_256x256_kernel", "gemm_tn_256x256_group_kernel"}


def test_knob_only_kernels_are_selected_by_their_knob(H):
    assert reached(H, [GS.nt(4100, 1536, 320, res=1), GS.nt(4100, 1536, 320, res=1, bias=1)], knobs={7: 3}) == KNOB_ONLY


# ---- the grouped weight gradient's partition, in a stand-alone program under ASan + UBSan
def test_group_partition_covers_every_row_once(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gemm_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        f"-I{os.path.join(REPO, 'mca-paper_amd', 'csrc')}", os.path.join(REPO, "tests", "gemm_plan_check.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "1728 cases" in r.stdout and "0 failures" in r.stdout, r.stdout[-2000:]
