"""The evaluation kernels (csrc/evaluate.hip) through their raw entry points, element by element at their edges: every operand with
a leading dimension above its columns inside a NaN frame, every output and workspace inside a sentinel frame, integer data wherever
that makes the result exact, a float64 reference and a derived bound otherwise (tests/eval_edge_util.py, tests/eval_cases.py;
docs/parity.md, "Evaluation kernels: every element, at the edges").  Only valid calls are launched."""
import importlib

import pytest
import torch

import eval_cases as EC
import eval_edge_util as E

pytestmark = pytest.mark.gpu
F32, I32 = torch.float32, torch.int32
BADARG, UNSUPPORTED = -1, -3
DEV = "cuda"


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def ids(cases):
    return [c["name"] for c in cases]


def p(t):
    return None if t is None else t.data_ptr()


def ld(t):
    return t.stride(0)


def sync():
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", EC.NORMALIZE, ids=ids(EC.NORMALIZE))
def test_rows_normalize_edges(H, case):
    T, O = E.normalize_setup(case, DEV)
    H.call("mca_rows_normalize_f32", p(T["x"]), ld(T["x"]), O["y"].data_ptr(), O["y"].ld, case["n"], case["d"], H.stream_ptr())
    sync()
    E.normalize_check(case, T, O)


def test_rows_normalize_no_rows(H):
    T, O = E.normalize_setup(dict(n=1, d=5), DEV)
    assert H.lib().mca_rows_normalize_f32(p(T["x"]), ld(T["x"]), O["y"].data_ptr(), O["y"].ld, 0, 5, H.stream_ptr()) == 0
    sync()
    E.untouched(O["y"], "n = 0")


def rank_args(H, c, T, O):
    return (p(T["q"]), ld(T["q"]), p(T["qidx"]), c["nq"], p(T["t"]), ld(T["t"]), c["nt"], c["d"], O["s_true"].data_ptr(), O["rank"].data_ptr(), H.stream_ptr())


@pytest.mark.parametrize("case", EC.RANK, ids=ids(EC.RANK))
def test_cosine_rank_edges(H, case):
    T, O = E.rank_setup(case, DEV)
    H.call("mca_cosine_rank_f32", *rank_args(H, case, T, O))
    sync()
    E.rank_check(case, T, O)


def test_cosine_rank_more_queries_than_targets_refused(H):
    c = dict(name="rank-refused", nq=5, nt=5, d=4, gather=False)
    T, O = E.rank_setup(c, DEV)
    assert H.lib().mca_cosine_rank_f32(*rank_args(H, dict(c, nt=4), T, O)) == BADARG
    sync()
    E.untouched(O["rank"], "refused rank"), E.untouched(O["s_true"], "refused s_true")


def pair_args(H, c, T, O, n_partials):
    x = T["x"]
    return (p(x), ld(x) if x is not None else 0, c["n"], c["d"], E.PAIR_T, O["partials"].data_ptr(), n_partials, O["sum"].data_ptr(), O["value"].data_ptr(),
            H.stream_ptr())


@pytest.mark.parametrize("case", EC.PAIR, ids=ids(EC.PAIR))
def test_pair_gauss_edges(H, case):
    T, O = E.pair_setup(case, DEV)
    need = H.lib().mca_pair_gauss_workspace(case["n"])
    assert need == E.pair_tiles(case["n"]) ** 2
    H.call("mca_pair_gauss_sum_f32", *pair_args(H, case, T, O, need))
    sync()
    E.pair_check(case, T, O)


def test_pair_gauss_short_workspace_refused(H):
    c = dict(name="pair-short", n=65, d=3)
    T, O = E.pair_setup(c, DEV, short=1)
    assert H.lib().mca_pair_gauss_sum_f32(*pair_args(H, c, T, O, 3)) == BADARG
    sync()
    for k in ("partials", "sum", "value"):
        E.untouched(O[k], f"refused {k}")


@pytest.mark.parametrize("case", EC.PROBE_NT, ids=ids(EC.PROBE_NT))
def test_probe_nt_edges(H, case):
    T, O = E.nt_setup(case, DEV)
    H.call("mca_probe_nt_f32", p(T["x"]), ld(T["x"]), p(T["xidx"]), p(T["w"]), ld(T["w"]), p(T["bias"]), O["y"].data_ptr(), O["y"].ld, case["M"], case["N"],
           case["K"], case["act"], case["p"], E.SEED, E.STEP, H.stream_ptr())
    sync()
    E.nt_check(case, T, O)


def head_args(H, c, T, O, K=None, L=None):
    return (p(T["a"]), ld(T["a"]), p(T["aidx"]), K or c["K"], p(T["w"]), p(T["bias"]), L or c["L"], p(T["labels"]), p(T["yidx"]), c["B"], c["loss"],
            O["pred"].data_ptr(), p(O["dz"]), p(O["da"]), E.DACT, O["loss_part"].data_ptr(), H.stream_ptr())


@pytest.mark.parametrize("case", EC.PROBE_HEAD, ids=ids(EC.PROBE_HEAD))
def test_probe_head_edges(H, case):
    T, O = E.head_setup(case, DEV)
    assert H.lib().mca_probe_head_blocks(case["B"]) == EC.cdiv(case["B"], 4)
    H.call("mca_probe_head_f32", *head_args(H, case, T, O))
    sync()
    E.head_check(case, T, O)


def test_probe_head_limits_refused(H):
    c = dict(name="head-refused", K=8, L=4, B=3, loss=EC.MSE, dz=1, da=1, aidx=0, yidx=0)
    T, O = E.head_setup(c, DEV)
    assert H.lib().mca_probe_head_f32(*head_args(H, c, T, O, K=1025)) in (UNSUPPORTED, BADARG)          # lda < K is asked first
    T["a"] = E.framed_in(torch.zeros(3, 8, device=DEV), 1100)
    assert H.lib().mca_probe_head_f32(*head_args(H, c, T, O, K=1025)) == UNSUPPORTED
    assert H.lib().mca_probe_head_f32(*head_args(H, c, T, O, L=65)) == UNSUPPORTED
    sync()
    for k in ("pred", "dz", "da", "loss_part"):
        E.untouched(O[k], f"refused {k}")


def tn_args(H, c, T, O, n_partials):
    return (p(T["a"]), ld(T["a"]), p(T["b"]), ld(T["b"]), p(T["bidx"]), c["R"], c["N"], c["K"], O["partials"].data_ptr(), n_partials, O["gw"].data_ptr(),
            O["gb"].data_ptr(), H.stream_ptr())


@pytest.mark.parametrize("case", EC.PROBE_TN, ids=ids(EC.PROBE_TN))
def test_probe_tn_edges(H, case):
    T, O = E.tn_setup(case, DEV)
    assert H.lib().mca_probe_tn_workspace(case["R"], case["N"], case["K"]) == O["need"]
    H.call("mca_probe_tn_f32", *tn_args(H, case, T, O, O["need"]))
    sync()
    E.tn_check(case, T, O)


def test_probe_tn_short_workspace_refused(H):
    c = dict(name="tn-short", R=129, N=3, K=2, gather=0)
    T, O = E.tn_setup(c, DEV, short=1)
    assert H.lib().mca_probe_tn_f32(*tn_args(H, c, T, O, O["need"] - 1)) == BADARG
    sync()
    for k in ("partials", "gw", "gb"):
        E.untouched(O[k], f"refused {k}")


@pytest.mark.parametrize("n", EC.LOSS_ACCUM)
def test_probe_loss_accum_edges(H, n):
    """integer partials and a count of 8: the sum and the quotient are exact, on top of an accumulator that starts at 5"""
    part = E.framed_in(E.ints((1, n), E.gen(47, DEV), 9), n + E.PAD)
    acc = E.out(1, 1, DEV)
    acc.t.fill_(5.0)
    for k in (1, 2):
        H.call("mca_probe_loss_accum", p(part), n, 8, acc.data_ptr(), H.stream_ptr())
        sync()
        assert float(acc.t[0, 0]) == 5.0 + k * float(part.double().sum()) / 8
    E.assert_guard_intact(acc, "acc")


def test_print_worst_ratios():
    """last in the file: the largest error / bound ratio of every bounded quantity over the cases above (pytest -s shows it)"""
    seen = {k: v for k, v in E.WORST.items() if k.startswith("eval ")}
    for k in sorted(seen):
        print(f"worst |got - ref| / bound  {k:28s} {seen[k]:.3f}")
    assert seen
