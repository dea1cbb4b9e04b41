"""mca_task_head_fwd_bwd (csrc/task_head.hip) through its raw entry point, element by element at its edges: every operand inside a
NaN frame, every output and the workspace inside a sentinel frame, pred, loss, d_pooled, gw and gb against float64 with the bounds of
tests/task_head_util.py (exact wherever the scale is a power of two), twice, with the same bits both times.  The labels of invalid
rows and the label columns outside the window hold NaN.  Only valid calls are launched (the refusals: tests/test_task_head_cpu.py)."""
import ctypes as C
import importlib

import pytest
import torch

import task_head_cases as TC
import task_head_util as TU

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def launch(H, case, T):
    O = TU.outputs(case, T, DEV)
    a = TU.fill_args(H, case, T, O)
    H.call("mca_task_head_fwd_bwd", C.byref(a), H.stream_ptr())
    torch.cuda.synchronize()
    return O


@pytest.mark.parametrize("case", TC.CASES, ids=[c["name"] for c in TC.CASES])
def test_task_head_edges(H, case):
    T = TU.setup(case, DEV)
    O = launch(H, case, T)
    TU.check(case, T, O)
    O2 = launch(H, case, T)
    TU.check(case, T, O2, " (second launch)")
    TU.same_bits(O, O2, case["name"])


def test_invalid_rows_labels_are_never_read(H):
    """other values in the labels of invalid rows and in the columns outside the window: no output bit changes"""
    case = next(c for c in TC.CASES if c["presence"] == "mixed" and c["ld_labels"] > c["L"] and c["b"] == 65)
    T = TU.setup(case, DEV)
    O = launch(H, case, T)
    keep = T["labels"][:, case["col_off"]:case["col_off"] + case["L"]][T["valid"]].clone()
    T["labels"].fill_(1e30)
    win = T["labels"][:, case["col_off"]:case["col_off"] + case["L"]]
    win[T["valid"]] = keep
    O2 = launch(H, case, T)
    TU.same_bits(O, O2, case["name"])
