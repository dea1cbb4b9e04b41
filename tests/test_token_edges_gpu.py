"""The token-table kernels (csrc/embedding.hip: mark, renormalise the marked rows, gather; the table gradient with fp32 atomics
and in the fixed order of its sort + sum) element by element at their edges: every output inside a sentinel frame (destination,
table, dtable, marker, flag word, a det scratch of exactly the reported size), every input inside NaN or, the indices, inside
out-of-range values (tests/token_edge_util.py); integer data where that makes the result exact in any order, the header's order
restated in fp32 and compared bitwise, a float64 reference and a derived bound otherwise (docs/parity.md, "Token tables: every
element, at the edges").  The grid and the pass counts every listed case reaches are asserted without a GPU in
tests/test_token_edges_cpu.py, which also shows every bound satisfiable.  Only valid calls are launched: the frames exist so that a
stray access lands in memory the test owns."""
import importlib

import pytest
import torch

import token_cases as TC
import token_edge_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def ids(cases):
    return [c["name"] for c in cases]


def by_name(cases, name):
    return next(c for c in cases if c["name"] == name)


@pytest.mark.parametrize("case", TC.LOOKUP, ids=ids(TC.LOOKUP))
def test_lookup_edges(H, case):
    def launch(c, T):
        H.call("mca_embedding_lookup", *U.lookup_args(c, T), H.stream_ptr())
        torch.cuda.synchronize()
    U.lookup_case(case, "cuda", launch)


@pytest.mark.parametrize("case", TC.GRAD, ids=ids(TC.GRAD))
def test_table_gradient_edges(H, case):
    def launch(c, T, O, det, ib):
        if det:
            need = H.lib().mca_embedding_scatter_add_det_scratch(c["tokens"])
            assert need == O["scratch"].cols          # the scratch is exactly the reported size
            H.call("mca_embedding_scatter_add_det", *U.grad_args(c, T, O, ib), O["scratch"].data_ptr(), need, H.stream_ptr())
        else:
            H.call("mca_embedding_scatter_add", *U.grad_args(c, T, O, ib), H.stream_ptr())
        torch.cuda.synchronize()
    U.grad_case(case, "cuda", launch)


def test_refusals_move_no_byte(H):
    """every refused argument of the three entry points, a scratch one float short and rows == 0: the return code, and not one byte
    of any output or scratch moved (MCA_E_UNSUPPORTED needs 2^31 tokens and is not tested)"""
    L = H.lib()
    case = by_name(TC.LOOKUP, "oob-68x10-a1c1-i64")
    T = U.lookup_setup(case, "cuda")
    before = U.lookup_snapshot(T)
    for name, rc, want in U.lookup_refusals(L, case, T, H.stream_ptr()):
        assert rc == want, f"lookup: {name}: {rc}, want {want}"
    torch.cuda.synchronize()
    for k, b in before.items():
        assert torch.equal(T[k].buf, b), f"lookup: {k} moved in a refused or empty call"
    g = by_name(TC.GRAD, "mixed-129x257-pad5")
    T = U.grad_setup(g, "cuda", False)
    O = U.grad_outputs(g, T, "cuda", True)
    before = {k: O[k].buf.clone() for k in ("dtable", "scratch")}
    for name, rc, want in U.grad_refusals(L, g, T, O, H.stream_ptr()):
        assert rc == want, f"{name}: {rc}, want {want}"
    torch.cuda.synchronize()
    for k, b in before.items():
        assert torch.equal(O[k].buf, b), f"{k} moved in a refused or empty call"


def test_print_worst_ratios(H):
    """last in the file: how much of each bound the kernels use over all cases (pytest -s shows it)"""
    for k in sorted(U.WORST):
        print(f"worst |kernel - ref| / bound  {k:24s} {U.WORST[k]:.3f}")
    assert U.WORST
