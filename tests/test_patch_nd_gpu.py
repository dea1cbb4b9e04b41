"""`mca_patch_nd_ln_fwd` on the GPU, through the C ABI, element by element inside NaN frames and sentinel guards, with guard rows
between the channel planes and the frames (tests/patch_nd_cases.py: cases, data, framing; tests/patch_cases.py: the checks, float64
references and bounds, which are the matrix kernel's because the normalising stage is).  The step that uses it:
tests/test_patch_nd_step_gpu.py."""
import importlib

import pytest
import torch

import patch_cases as pc
import patch_nd_cases as nd
from row_edge_util import WORST

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    importlib.import_module("mca-paper_amd")
    return importlib.import_module("mca-paper_amd.hip")


def stream():
    return torch.cuda.current_stream().cuda_stream


def launch(H, T, O):
    H.call("mca_patch_nd_ln_fwd", *nd.args(T, O), stream())
    torch.cuda.synchronize()


@pytest.fixture()
def form(H, request):
    H.lib().mca_debug_set(13, nd.FORMS[request.param])
    yield request.param
    H.lib().mca_debug_set(13, 0)


@pytest.mark.parametrize("form", list(nd.FORMS), indirect=True)
@pytest.mark.parametrize("c", nd.CASES, ids=nd.case_id)
def test_kernel_plain_data(H, c, form):
    """statistics and xn_bf16 of every row (the plain data excludes none: cap MAX_EXCLUDED asserted), with xp and without, at a row
    stride of W + 3 (scalar accesses) and W + 4 (16-byte accesses where p2 % 4 == 0)"""
    gen = torch.Generator(device="cuda").manual_seed(5)
    rows = nd.plain_rows(c, gen)
    for extra, with_xp in ((3, True), (3, False), (4, True), (4, False)):
        T, O = nd.setup(c, rows, gen, ldv_extra=extra, with_xp=with_xp)
        launch(H, T, O)
        live, skipped = pc.check(T, O, f"{nd.case_id(c)} {form} plain ldv = W + {extra}{'' if with_xp else ', xp NULL'}", cap=pc.MAX_EXCLUDED)
        assert live > 0 and skipped == 0
    print({k: round(v, 3) for k, v in WORST.items() if k.startswith("patch_ln")})


@pytest.mark.parametrize("form", list(nd.FORMS), indirect=True)
@pytest.mark.parametrize("c", nd.CASES, ids=nd.case_id)
def test_kernel_special_patches(H, c, form):
    """every row of the case as every kind of patch_nd_cases.KINDS ("one channel all pad, the others real" among them: not masked,
    statistics checked): xp and padmask exact, all-pad rows exact, the rest within bounds"""
    gen = torch.Generator(device="cuda").manual_seed(6)
    for v in range(nd.N_KINDS):
        T, O = nd.setup(c, nd.special_rows(c, v, gen), gen, ldv_extra=3 + v % 2, with_xp=v % 4 < 2)
        launch(H, T, O)
        pc.check(T, O, f"{nd.case_id(c)} {form} special {v}")


@pytest.mark.parametrize("form", list(nd.FORMS), indirect=True)
@pytest.mark.parametrize("c", nd.DEGENERATE, ids=nd.case_id)
def test_one_plane_matches_the_matrix_kernel_bit_for_bit(H, c, form):
    """C = T = pt = 1: all five outputs equal mca_patch_ln_fwd's on the same matrix, compared as integers (scalar and 16-byte paths)"""
    gen = torch.Generator(device="cuda").manual_seed(8)
    for v, extra in ((None, 3), (None, 4), (0, 3), (3, 4), (5, 4)):
        rows = nd.plain_rows(c, gen) if v is None else nd.special_rows(c, v, gen)
        T, O = nd.setup(c, rows, gen, ldv_extra=extra)
        _, M = nd.setup(c, rows, gen, ldv_extra=extra)
        launch(H, T, O)
        H.call("mca_patch_ln_fwd", *nd.matrix_args(T, M), stream())
        torch.cuda.synchronize()
        pc.check(T, O, f"{nd.case_id(c)} {form} N-D")
        for k, it in (("xp", torch.int32), ("xn", torch.int16), ("mean", torch.int32), ("rstd", torch.int32), ("mask", torch.uint8)):
            a, b = O[k].t.contiguous().view(it), M[k].t.contiguous().view(it)
            assert torch.equal(a, b), f"{nd.case_id(c)} {form} variant {v} ldv = W + {extra}: {k} differs from mca_patch_ln_fwd in {int((a != b).sum())} elements"


def test_kernel_refusals_leave_the_outputs_untouched(H):
    """a host-side check that launches nothing: MCA_E_BADARG, every sentinel intact"""
    c = (2, 2, 4, 4, 2, 2, 2, 2)          # C = 2, T = 4, H = W = 8: P = 64
    gen = torch.Generator(device="cuda").manual_seed(7)
    T, O = nd.setup(c, nd.plain_rows(c, gen), gen, ldv_extra=4)
    L = H.lib()
    base = list(nd.args(T, O))
    BADARG = -1          # MCA_E_BADARG (include/mca_hip.h)

    def rc(**kw):
        a = list(base)
        for k, v in kw.items():
            a[nd.ARG[k]] = v
        return L.mca_patch_nd_ln_fwd(*a, stream())
    bad = dict(T=dict(T=5), H=dict(H=9), W=dict(W=9), ldv=dict(ldv=7), fstride=dict(fstride=7 * T["ldv"] + 7), cstride=dict(cstride=3 * T["fstride"] + 7 * T["ldv"] + 7),
               bstride=dict(bstride=T["cstride"] + 3 * T["fstride"] + 7 * T["ldv"] + 7), cols_pad=dict(cols_pad=63), ld_bf16=dict(ld_bf16=63),
               **{k: {k: None} for k in ("values", "gamma", "beta", "xn", "mean", "rstd", "mask")})
    for what, kw in bad.items():
        assert rc(**kw) == BADARG, what
    torch.cuda.synchronize()
    for k in ("xp", "xn", "mean", "rstd", "mask"):
        t = O[k].t
        it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
        assert bool((t.contiguous().view(it) == (255 if it == torch.uint8 else -1)).all()), f"{k}: stored to by a refused call"
        pc.assert_guard_intact(O[k], k)
    assert rc() == 0          # the same arguments unchanged are accepted
    torch.cuda.synchronize()
    pc.check(T, O, "accepted call")


@pytest.mark.parametrize("c", [(5, 5, 41, 1, 1, 1, 2, 1), (8, 2, 16, 8, 1, 1, 2, 1)], ids=["P1025", "P2048"])
def test_more_than_1024_elements_is_refused(H, c):
    """P = 1025 and P = 2048 with every other argument valid: buffers, strides, cols_pad and ld_bf16 are those of the case itself, so
    the check on P is the only one that can refuse (at these sizes span * PS still fits the LDS budget, and a launch would cover
    only 1024 columns of each patch).  MCA_E_BADARG, every output still the sentinel."""
    d = nd.dims(c)
    assert d["P"] in (1025, 2048) and d["kp"] >= d["P"]
    gen = torch.Generator(device="cuda").manual_seed(9)
    T, O = nd.setup(c, nd.plain_rows(c, gen), gen, ldv_extra=4)
    assert H.lib().mca_patch_nd_ln_fwd(*nd.args(T, O), stream()) == -1          # MCA_E_BADARG (include/mca_hip.h)
    torch.cuda.synchronize()
    for k in ("xp", "xn", "mean", "rstd", "mask"):
        t = O[k].t
        it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
        assert bool((t.contiguous().view(it) == (255 if it == torch.uint8 else -1)).all()), f"{k}: stored to by a refused call"
        pc.assert_guard_intact(O[k], k)
