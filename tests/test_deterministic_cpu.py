"""Deterministic mode without a GPU: the plans of the fixed-order weight-gradient forms (csrc/gemm_plan.h through the
mca_dbg_plan_gemm_tn_det / _group_det hooks) cover every (tile, row) exactly once with one workgroup per (tile, split) cell, the
size queries equal slots x floats of one partial, the default planners are what they were, and the MCA_DEBUG switch parses."""
import ctypes as C
import importlib
import json
import os
import shutil
import subprocess

import pytest

import gemm_shapes as GS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    importlib.import_module("mca-paper_amd.build").build()
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def det_plan(H, R, N, K):
    p = H.TnDetPlan()
    assert H.lib().mca_dbg_plan_gemm_tn_det(R, N, K, C.byref(p)) == 0
    return p


def check_single(H, R, N, K):
    """-> slots.  Split s of the grid reduces rows [s * rows_per_split, (s + 1) * rows_per_split) of every tile."""
    L = H.lib()
    p, plain = det_plan(H, R, N, K), H.GemmPlan()
    assert L.mca_dbg_plan_gemm_tn(R, N, K, C.byref(plain)) == 0
    same = ("kernel", "grid_x", "grid_y", "block", "lds_bytes", "n", "tiles_k", "rows_per_split", "dbg")
    assert all(getattr(p.launch, f) == getattr(plain, f) for f in same), (R, N, K)
    assert p.slots == p.launch.grid_y and p.slot_stride == N * K
    assert p.scratch_floats == (p.slots * N * K if p.slots > 1 else 0) == L.mca_gemm_tn_acc_det_scratch(R, N, K)
    rps = p.launch.rows_per_split
    bounds = [(s * rps, min(R, (s + 1) * rps)) for s in range(p.slots)]
    assert bounds[0][0] == 0 and bounds[-1][1] == R and all(b < e for b, e in bounds), (R, N, K, bounds)          # adjacent by construction
    tile_n, tile_k = (256, 256) if "256x256" in L.mca_dbg_gemm_kernel_name(p.launch.kernel).decode() else \
        (256, 128) if "256" in L.mca_dbg_gemm_kernel_name(p.launch.kernel).decode() else (128, 128)
    assert p.launch.grid_x == -(-N // tile_n) * -(-K // tile_k) and p.launch.tiles_k == -(-K // tile_k)          # every tile once per split
    return p.slots


def segments(part, lin):
    """mca_tn_group_segments (csrc/gemm_plan.h) for the uniform partition: workgroup lin is the cell (lin % tiles, lin // tiles)"""
    assert part.span == 0 and part.own == 0 and lin < part.n_full * part.tiles
    r0 = (lin // part.tiles) * part.unit
    return lin % part.tiles, r0, min(r0 + part.unit, part.R)


def check_group(H, R, members, cus):
    L = H.lib()
    n = len(members)
    N, K = (C.c_int64 * n)(*[m[0] for m in members]), (C.c_int64 * n)(*[m[1] for m in members])
    p = H.TnGroupDetPlan()
    assert L.mca_dbg_plan_gemm_tn_group_det(N, K, n, R, cus, C.byref(p)) == 0
    need = L.mca_gemm_tn_acc_group_det_scratch(N, K, n, R, cus)
    assert need == p.scratch_floats
    plain = H.TnGroupPlan()
    assert L.mca_dbg_plan_gemm_tn_group(N, K, n, R, cus, C.byref(plain)) == 0
    assert (p.plan.grouped == 1) == (plain.grouped == 1), "the deterministic form groups exactly what the plain form groups"
    if p.plan.grouped == 0:          # refused by the grouped kernel: single-problem deterministic plans, sharing the scratch
        assert need == max(L.mca_gemm_tn_acc_det_scratch(R, m[0], m[1]) for m in members)
        for m in members:
            check_single(H, R, m[0], m[1])
        return 0
    part, ln = p.plan.part, p.plan.launch
    tiles = sum(-(-m[0] // 256) * -(-m[1] // 256) for m in members)
    assert (part.tiles, part.R, part.span, part.own) == (tiles, R, 0, 0)
    assert p.slots == part.n_full and ln.grid_x == part.n_full * tiles and ln.grid_y == 1          # slot count = the grid's split count
    assert p.slot_stride == sum(m[0] * m[1] for m in members) and need == (p.slots * p.slot_stride if p.slots > 1 else 0)
    assert p.slots == 1 or ln.grid_x <= cus, "one round of workgroups"
    assert H.lib().mca_dbg_gemm_kernel_name(ln.kernel) == b"gemm_tn_256x256_group_kernel"
    nxt, seen = [0] * tiles, set()
    for lin in range(ln.grid_x):
        t, b, e = segments(part, lin)
        assert (t, lin // tiles) not in seen and b == nxt[t] and e > b, (R, members, lin)
        seen.add((t, lin // tiles)); nxt[t] = e
    assert nxt == [R] * tiles and len(seen) == tiles * p.slots
    return p.slots


def test_deterministic_plans_cover_every_tile_and_row_once(H):
    for R, N, K, _, _ in GS.TN_ACC:
        check_single(H, R, N, K)
    for cus in (256, 64):
        for R, ms in GS.TN_GROUP:
            check_group(H, R, [(m[0], m[1]) for m in ms], cus)
        for T in GS.STEP_ROWS.values():
            for c in GS.step_calls(T):
                if c["entry"] == "tn":
                    check_single(H, c["R"], c["N"], c["K"])
                elif c["entry"] == "tn_group":
                    assert check_group(H, c["R"], [tuple(m) for m in c["members"]], cus) >= 1
    # the shapes of tests/test_deterministic_gpu.py: kernel and split count as that file states them
    name = lambda R, N, K: H.lib().mca_dbg_gemm_kernel_name(det_plan(H, R, N, K).launch.kernel)
    assert name(1000, 200, 136) == b"gemm_tn_kernel" and check_single(H, 1000, 200, 136) == 4
    assert name(4160, 512, 256) == b"gemm_tn_256_kernel" and check_single(H, 4160, 512, 256) == 17
    assert name(4160, 1024, 512) == name(5000, 1365, 512) == b"gemm_tn_256x256_kernel"
    assert check_single(H, 4160, 1024, 512) >= 2 and check_single(H, 5000, 1365, 512) >= 2
    assert check_group(H, GS.TN_GROUP[3][0], [(m[0], m[1]) for m in GS.TN_GROUP[3][1]], 256) == 12
    assert check_group(H, 4160, [(1024, 512), (512, 1024)], 256) == 15
    assert check_group(H, GS.TN_GROUP[4][0], [(m[0], m[1]) for m in GS.TN_GROUP[4][1]], 256) == 0 == check_group(H, *[(300, [(512, 512), (512, 256)])][0], 256)


def test_deterministic_plans_follow_knob_3(H):
    with H.knobs(k3=3):
        assert check_single(H, 5000, 1024, 512) == 3
        assert check_group(H, 8200, [(m[0], m[1]) for m in GS.TN_GROUP[1][1]], 256) == 3


def test_plan_check_program_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "det_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        f"-I{os.path.join(REPO, 'mca-paper_amd', 'csrc')}", os.path.join(REPO, "tests", "det_plan_check.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "2010 cases, 0 failures" in r.stdout, r.stdout[-2000:]


def test_default_tn_planners_unchanged_with_the_mode_on(H, monkeypatch):
    """The mode is a host-side switch: the default planners do not read it.  The recorded dispatch of every weight-gradient
    entry (tests/golden/gemm_dispatch.json) is re-asserted with MCA_DEBUG=deterministic=1 in the environment."""
    T = importlib.import_module("test_gemm_plan_cpu")
    E = importlib.import_module("mca-paper_amd.engine")
    monkeypatch.setenv("MCA_DEBUG", "deterministic=1")
    assert E.debug_options()["deterministic"] is True
    rows = [r for r in json.load(open(os.path.join(REPO, "tests", "golden", "gemm_dispatch.json"))) if r["case"]["entry"] in ("tn", "tn_group")]
    assert len(rows) > 50
    for row in rows:
        case = row["case"]
        rc, launches = T.planned_launches(H, case, case["cus"], {int(k): v for k, v in case["knobs"].items()})
        assert rc == row["rc"] and launches == row["launches"], case


def test_debug_switch_parses(monkeypatch):
    E = importlib.import_module("mca-paper_amd.engine")
    monkeypatch.delenv("MCA_DEBUG", raising=False)
    assert E.debug_options()["deterministic"] is False
    monkeypatch.setenv("MCA_DEBUG", "deterministic=1")
    assert E.debug_options()["deterministic"] is True
    monkeypatch.setenv("MCA_DEBUG", "group_wgrad=0,deterministic=0")
    o = E.debug_options()
    assert o["deterministic"] is False and o["group_wgrad"] is False
    monkeypatch.setenv("MCA_DEBUG", "deterministic=1,determinstic=1")
    with pytest.raises(ValueError, match="unknown switch"):
        E.debug_options()


def test_small_scratch_queries(H):
    """host-only size queries of the column-partial forms: slots x slot floats, with the slab rules of elementwise.hip"""
    L = H.lib()
    assert L.mca_reduce_rows_det_scratch(20 * 15, 15, 512) == (512 // (15 * 2)) * 15 * 512
    assert L.mca_reduce_rows_det_scratch(12000, 1, 512) == 256 * 512
    assert L.mca_tab_value_bwd_det_scratch(1000, 128) == 500 * 2 * 128          # 2 rows per slab
    assert L.mca_layernorm_bwd_det_scratch(4099, 512) == 256 * 3 * 512          # general form: 1,025 four-row groups, capped at 256 workgroups
    assert L.mca_layernorm_bwd_det_scratch(1000, 512) == 250 * 3 * 512          # general 250 workgroups, trunk 125, params-only 32
    assert L.mca_layernorm_bwd_det_scratch(0, 512) == 0 and L.mca_gemm_tn_acc_det_scratch(16, 512, 512) == 0
