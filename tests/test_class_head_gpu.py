"""mca_class_head_fwd_bwd and mca_probe_head_ce_f32 (csrc/class_head.hip) through their raw entry points, element by element at their
edges: every operand inside a NaN frame, every output and the workspace inside a sentinel frame, the outputs against float64
(autograd of F.cross_entropy on the CPU) with the bounds of tests/class_head_util.py, twice, with the same bits both times; the
return codes of refused calls, after which no output word has changed."""
import ctypes as C
import importlib

import pytest
import torch

import class_head_cases as CC
import class_head_util as CU

pytestmark = pytest.mark.gpu
DEV = "cuda"
CODES = {"BADARG": -1, "ALIGN": -2, "UNSUPPORTED": -3}


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def launch(H, case, T):
    O = CU.outputs(case, T, DEV)
    a = CU.fill_args(H, case, T, O)
    H.call("mca_class_head_fwd_bwd", C.byref(a), H.stream_ptr())
    torch.cuda.synchronize()
    return O


@pytest.mark.parametrize("case", CC.CASES, ids=[c["name"] for c in CC.CASES])
def test_class_head_edges(H, case):
    T = CU.setup(case, DEV)
    ref = CU.reference(case, T)
    O = launch(H, case, T)
    CU.check(case, T, O, "", ref)
    O2 = launch(H, case, T)
    CU.check(case, T, O2, " (second launch)", ref)
    CU.same_bits(O, O2, case["name"])


def test_uncounted_labels_are_never_read(H):
    """other values in the labels of rows that are invalid by presence and in the columns outside the window: no output bit changes"""
    case = next(c for c in CC.CASES if c["junk"])
    T = CU.setup(case, DEV)
    O = launch(H, case, T)
    keep = T["labels"][:, case["col_off"]][T["valid"]].clone()
    T["labels"].fill_(1e30)
    T["labels"][:, case["col_off"]][T["valid"]] = keep
    O2 = launch(H, case, T)
    CU.same_bits(O, O2, case["name"])


def test_refused_calls_launch_nothing(H):
    """device outputs prefilled with the sentinel stay untouched by calls that return a code"""
    case = next(c for c in CC.CASES if c["b"] == 5 and c["din"] == "given" and c["presence"] == "mixed")
    T = CU.setup(case, DEV)
    for field, value, code in CC.REFUSED_SIZES + [(p, None, "BADARG") for p in CC.REQUIRED_POINTERS] + [("workspace_bytes", 4, "BADARG")]:
        O = CU.outputs(case, T, DEV)
        a = CU.fill_args(H, case, T, O)
        setattr(a, field, value)
        assert H.lib().mca_class_head_fwd_bwd(C.byref(a), H.stream_ptr()) == CODES[code], (field, value)
        torch.cuda.synchronize()
        for k in CU.KEYS + ("ws",):
            assert (O[k].buf == O[k].buf[0]).all(), f"{field} = {value}: {k} was stored to"


@pytest.mark.parametrize("case", CC.PROBE_CASES, ids=[c["name"] for c in CC.PROBE_CASES])
def test_probe_head_ce_edges(H, case):
    T = CU.probe_setup(case, DEV)
    assert H.lib().mca_probe_head_blocks(case["B"]) == CU.cdiv(case["B"], 4)
    outs = []
    for what in ("", " (second launch)"):
        O = CU.probe_outputs(case, DEV)
        H.call("mca_probe_head_ce_f32", *CU.probe_args(H, case, T, O))
        torch.cuda.synchronize()
        CU.probe_check(case, T, O, what)
        outs.append(O)
    CU.same_bits(outs[0], outs[1], case["name"], CU.PROBE_KEYS)


def test_probe_head_ce_refusals(H):
    c = next(c for c in CC.PROBE_CASES if c["da"] and c["dz"] and c["B"] == 5 and c["K"] == 1024)
    T = CU.probe_setup(c, DEV)
    over = [({f: (c["K"] - 1 if v == "K-1" else v)}, code) for f, v, code in CC.PROBE_REFUSED] + [({f: None}, "BADARG") for f in CC.PROBE_REQUIRED_POINTERS]
    for kw, code in over:
        O = CU.probe_outputs(c, DEV)
        assert H.lib().mca_probe_head_ce_f32(*CU.probe_args(H, c, T, O, **kw)) == CODES[code], kw
        torch.cuda.synchronize()
        for k in CU.PROBE_KEYS:
            assert (O[k].buf == O[k].buf[0]).all(), f"{kw}: {k} was stored to"
