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
