"""The task head without a GPU: every argument check of mca_task_head_fwd_bwd and of its workspace query (a call that must refuse
returns its code before anything is launched), readout_plan, the finetune: YAML keys, and the case table of the GPU test: its
coverage, and the fp32 restatement of the kernel against the float64 reference within the bounds the GPU test uses."""
import importlib

import pytest
import torch

import task_head_cases as TC
import task_head_util as TU
from util_small import small_config

CODES = {"BADARG": -1, "ALIGN": -2, "UNSUPPORTED": -3}
BASE = dict(name="args", b=5, L=7, D=128, R=5, slot=0, loss=TC.MSE, presence="mixed", n_valid=4, din="given", base=0.5, tw=1.0, acc=0,
            ld_labels=7, col_off=0)


@pytest.fixture(scope="module")
def hip():
    h = importlib.import_module("mca-paper_amd.hip")
    h.lib()
    return h


@pytest.fixture(scope="module")
def ft():
    return importlib.import_module("mca-paper_amd.finetune")


def base_call(hip):
    T = TU.setup(BASE, "cpu")
    O = TU.outputs(BASE, T, "cpu")
    return T, O, TU.fill_args(hip, BASE, T, O)


def refused(hip, a, O, code, what):
    import ctypes as C
    assert hip.lib().mca_task_head_fwd_bwd(C.byref(a), None) == CODES[code], what
    for k in ("pred", "loss", "gw", "gb", "ws"):
        assert (O[k].t.contiguous().view(torch.int32) == -1).all(), f"{what}: {k} was stored to"


def test_null_args_struct(hip):
    assert hip.lib().mca_task_head_fwd_bwd(None, None) == CODES["BADARG"]


@pytest.mark.parametrize("field,value,code", TC.REFUSED_SIZES, ids=[f"{f}={v}" for f, v, _ in TC.REFUSED_SIZES])
def test_refused_sizes(hip, field, value, code):
    T, O, a = base_call(hip)
    setattr(a, field, value)
    refused(hip, a, O, code, f"{field} = {value}")


@pytest.mark.parametrize("field", TC.REQUIRED_POINTERS)
def test_null_pointer_refused(hip, field):
    T, O, a = base_call(hip)
    setattr(a, field, None)
    refused(hip, a, O, "BADARG", f"{field} NULL")


def test_present_null_needs_any_bits_zero(hip):
    T, O, a = base_call(hip)
    a.present = None
    refused(hip, a, O, "BADARG", "present NULL with any_bits != 0")


@pytest.mark.parametrize("field", ["task_weight", "base_weight"])
def test_nan_weight_refused(hip, field):
    T, O, a = base_call(hip)
    setattr(a, field, float("nan"))
    refused(hip, a, O, "BADARG", f"{field} NaN")


def test_short_workspace_refused(hip):
    T, O, a = base_call(hip)
    a.workspace_bytes -= 4
    refused(hip, a, O, "BADARG", "a workspace one float short")


@pytest.mark.parametrize("field", TC.WIDE_POINTERS + TC.NARROW_POINTERS)
def test_misaligned_pointer_refused(hip, field):
    T, O, a = base_call(hip)
    setattr(a, field, getattr(a, field) + (4 if field in TC.WIDE_POINTERS else 2))
    refused(hip, a, O, "ALIGN", f"{field} misaligned")


def test_workspace_query(hip):
    q = hip.lib().mca_task_head_workspace_bytes
    for c in TC.CASES:
        assert q(c["b"], c["L"], c["D"]) == 4 * TU.workspace_floats(c), c["name"]
    assert q(64, 1, 4) == 4 * (4 + 4 + 4) and q(65, 1, 4) == 2 * q(64, 1, 4)
    assert q(1, 64, 1024) == 4 * (64 * 1024 + 64 + 4)
    for b, L, D in ((0, 1, 4), (-1, 1, 4), (1, 0, 4), (1, 65, 4), (1, 1, 0), (1, 1, 1028), (1, 1, 6)):
        assert q(b, L, D) == -1, (b, L, D)


# ---- the case table ---------------------------------------------------------------------------------------------------------
def test_table_covers_the_edges():
    C = TC.CASES
    assert len({c["name"] for c in C}) == len(C)
    assert {c["b"] for c in C} == {1, 5, 64, 65, 129} and {c["L"] for c in C} == {1, 7, 64}
    assert {c["D"] for c in C} == {4, 128, 516, 1024} and {c["R"] for c in C} == {1, 5}
    assert {(c["R"], c["slot"]) for c in C} == {(1, 0), (5, 0), (5, 4)}
    for loss in (TC.L1, TC.MSE, TC.BCE):
        assert {c["acc"] for c in C if c["loss"] == loss} == {0, 1}
        assert {c["presence"] for c in C if c["loss"] == loss} >= {"mixed"}
    assert {c["din"] for c in C} == {None, "given", "alias"} and all(c["base"] == 0.5 for c in C if c["din"])
    assert {c["presence"] for c in C} == {"null", "all", "mixed", "none"}
    assert any(c["ld_labels"] > c["L"] and c["col_off"] > 0 for c in C)
    assert any(c["ld_labels"] > c["L"] and c["col_off"] + c["L"] < c["ld_labels"] for c in C)
    # no case but the one meant to has zero valid rows
    assert TC.NO_VALID_ROW == [c["name"] for c in C if c["presence"] == "none"] and len(TC.NO_VALID_ROW) == 1
    for c in C:
        v = TU.valid_rows(c)
        assert int(v.sum()) == c["n_valid"] and (c["n_valid"] > 0 or c["presence"] == "none"), c["name"]
        if c["presence"] == "mixed":
            assert 0 < c["n_valid"] < c["b"] and not v.all() and v.any()
    # both comparisons occur: exact ones (a power-of-two scale) and bounded ones, for L1 and MSE each
    for loss in (TC.L1, TC.MSE):
        assert {TU.scale32(c)[1] for c in C if c["loss"] == loss and c["n_valid"]} == {True, False}


@pytest.mark.parametrize("case", TC.CASES, ids=[c["name"] for c in TC.CASES])
def test_operands_are_what_the_bounds_assume(case):
    T = TU.setup(case, "cpu")
    b, L, D, R = case["b"], case["L"], case["D"], case["R"]
    for k in ("pooled", "w"):
        assert (T[k] == T[k].round()).all() and T[k].abs().max() <= 2
    assert ((T["w"] != 0).sum(1) <= 8).all() and T["w"].shape == (L, D) and T["pooled"].shape == (b * R, D)
    win = T["labels"][:, case["col_off"]:case["col_off"] + L]
    assert torch.isfinite(win[T["valid"]]).all() and torch.isnan(win[~T["valid"]]).all()
    if T["present"] is not None:
        assert torch.equal((T["present"] & T["any_bits"]) != 0, T["valid"])
    if case["loss"] == TC.BCE:
        assert ((win[T["valid"]] == 0) | (win[T["valid"]] == 1)).all()


@pytest.mark.parametrize("case", TC.CASES, ids=[c["name"] for c in TC.CASES])
def test_emulation_meets_the_reference(case):
    T = TU.setup(case, "cpu")
    O = TU.outputs(case, T, "cpu")
    TU.emulate_into(case, T, O)
    TU.check(case, T, O, " (fp32 restatement)")


def test_check_sees_a_wrong_element():
    """the comparison is no rubber stamp: one element of each output moved by a part in a thousand fails it"""
    case = next(c for c in TC.CASES if c["b"] == 65 and c["loss"] == TC.BCE)
    T = TU.setup(case, "cpu")
    for k in ("pred", "loss", "d_pooled", "gw", "gb"):
        O = TU.outputs(case, T, "cpu")
        TU.emulate_into(case, T, O)
        flat = O[k].t[0]
        i = int(flat.abs().argmax())
        flat[i] = flat[i] * 1.001
        with pytest.raises(AssertionError):
            TU.check(case, T, O)


# ---- readout_plan and the YAML keys -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["mca", "zorro", "bimodal"])
def test_readout_plan(pkg, ft, variant):
    model = pkg.build_model(small_config(variant))
    slots = model.output_slots()
    names = model.modality_types
    for i, name in enumerate(names):
        assert ft.readout_plan(model, name) == (i, 1 << i)
    slot, bits = ft.readout_plan(model, "fusion")
    assert slot == len(names) == slots["fusion"] and bits == 0b111          # every variant's fusion token sees all three modalities
    for key, s in slots.items():
        if isinstance(key, frozenset):
            assert ft.readout_plan(model, key) == (s, sum(1 << m for m in key))
    with pytest.raises(KeyError) as e:
        ft.readout_plan(model, "smell")
    assert "audio" in str(e.value) and "fusion" in str(e.value)


def test_finetune_settings(ft):
    assert ft.finetune_settings({}) == ft.FINETUNE_DEFAULTS
    assert ft.finetune_settings({"finetune": None}) == ft.FINETUNE_DEFAULTS
    s = ft.finetune_settings({"finetune": {"loss_type": "BCE", "task": -1, "readout": "audio", "head_lr": "1e-3", "task_weight": 2,
                                           "contrastive_weight": 0.5, "head_warmup_steps": 3}})
    assert s == {"loss_type": "BCE", "task": -1, "readout": "audio", "head_lr": 1e-3, "task_weight": 2.0, "contrastive_weight": 0.5,
                 "head_warmup_steps": 3}
    s = ft.finetune_settings({"encoder_configs": {"audio": {}, "video": {}, "text": {}}, "finetune": {"readout": ["audio", "text"]}})
    assert s["readout"] == frozenset({0, 2})
    with pytest.raises(KeyError) as e:
        ft.finetune_settings({"finetune": {"task": 1, "los_type": "L1", "zeta": 0}})
    assert "los_type" in str(e.value) and "zeta" in str(e.value)
    with pytest.raises(ValueError):
        ft.finetune_settings({"finetune": [1, 2]})


def test_script_refuses_cache_and_graph(ft):
    ft.refuse_with(1, False)
    for n, graph in ((2, False), (1, True)):
        with pytest.raises(SystemExit) as e:
            ft.refuse_with(n, graph)
        assert "grad_cache_chunks" in str(e.value) and "--graph" in str(e.value)


def test_script_refuses_before_it_touches_the_gpu(tmp_path):
    """finetune_accel_gpu.py --graph, and an unknown finetune: key, end the run by their messages on a machine without a GPU"""
    import os
    import subprocess
    import sys
    import yaml
    from conftest import REPO
    cfg = small_config("mca")
    for tag, ft_keys, extra, words in (("graph", {}, ["--graph"], ("grad_cache_chunks", "--graph")), ("key", {"los_type": "L1"}, [], ("los_type",))):
        ypath = tmp_path / f"{tag}.yaml"
        ypath.write_text(yaml.safe_dump(dict(encoder_configs=cfg["encoder_configs"], output_dir=str(tmp_path / tag), finetune=ft_keys)))
        r = subprocess.run([sys.executable, os.path.join(REPO, "finetune_accel_gpu.py"), str(ypath), "--synthetic", "2", *extra],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and all(w in r.stderr for w in words), r.stderr[-2000:]
        assert not os.path.exists(tmp_path / tag)
