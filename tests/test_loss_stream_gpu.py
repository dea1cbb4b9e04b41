"""mca_contrastive_stream_fwd_bwd (csrc/loss_stream.hip) element by element: every case of tests/loss_stream_cases.py at every rank,
every input inside a frame, every output and the workspace inside a sentinel frame and the workspace pre-filled with NaN bytes (no
word of it may be read before it is written), w exactly, the row statistics, the losses and d_pooled against the float64
restatement of csrc/loss.hip's formulas within the bounds derived in docs/parity.md ("Streaming contrastive loss: every element"),
two launches byte for byte, then one production shape against the same reference and against the dense kernel.
tests/test_loss_stream_cpu.py shows without a GPU that the cases reach their paths and that the bounds are satisfiable.  Only valid
calls are launched."""
import importlib

import pytest
import torch

import loss_stream_cases as SC
import loss_stream_util as SU
import row_edge_util as RU
from gemm_edge_util import _framed

pytestmark = pytest.mark.gpu
F32, I32 = torch.float32, torch.int32
BADARG, UNSUPPORTED = -1, -3
CASE_INDEX = {c["name"]: i for i, c in enumerate(SC.CASES)}
OUT_KEYS = ("term_loss", "loss", "dls", "d_pooled")


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def framed_ints(t):
    flat = t.reshape(1, -1).to(I32)
    _, _, view = _framed(1, flat.shape[1], flat.shape[1] + 3, I32, "cuda", 0xFF, 0)
    view.copy_(flat)
    return view


class Launch:
    """the framed operands of one case on the device, and fresh sentinel-framed outputs for every call; the workspace is exactly
    mca_contrastive_stream_workspace_bytes long, so the guard begins where the kernel's right to write ends"""

    def __init__(self, H, d):
        self.H, self.d = H, d
        self.pooled = RU.vec_framed(d["pooled"].reshape(-1).cuda())
        self.present = framed_ints(d["present"])
        self.terms = framed_ints(torch.tensor(d["terms"], dtype=torch.int64))
        self.s = RU.vec_framed(d["s"].reshape(1).cuda())
        self.lay = H.contrastive_stream_layout(d["B"], d["T"])
        self.ws_bytes = H.lib().mca_contrastive_stream_workspace_bytes(d["B"], d["T"], d["R"], d["D"])
        assert self.ws_bytes % 4 == 0 and self.ws_bytes >= self.lay["w"][0] + self.lay["w"][1]

    def outputs(self):
        d, g = self.d, lambda n: RU.guarded_out(1, n, n + 3, F32, device="cuda")
        O = dict(term_loss=g(d["T"]), loss=g(1), dls=g(1), d_pooled=g(d["b_local"] * d["R"] * d["D"]), ws=g(self.ws_bytes // 4))
        O["ws"].t.view(I32).fill_(-1)          # 0xFF bytes: a NaN wherever the kernel reads a word it has not written
        return O

    def args(self, O, r, **over):
        d = self.d
        a = dict(pooled=self.pooled.data_ptr(), present=self.present.data_ptr(), terms=self.terms.data_ptr(), T=d["T"], s=self.s.data_ptr(), B=d["B"],
                 b_local=d["b_local"], row0=r * d["b_local"], R=d["R"], D=d["D"], term_loss=O["term_loss"].data_ptr(), loss=O["loss"].data_ptr(),
                 d_pooled=O["d_pooled"].data_ptr(), dls=O["dls"].data_ptr(), ws=O["ws"].data_ptr(), ws_bytes=self.ws_bytes)
        a.update(over)
        return tuple(a.values()) + (self.H.stream_ptr(),)

    def run(self, r):
        """-> (the CPU tensors check() takes, the guarded outputs)"""
        d, O = self.d, self.outputs()
        self.H.call("mca_contrastive_stream_fwd_bwd", *self.args(O, r))
        torch.cuda.synchronize()
        T, B, W = d["T"], d["B"], d["W"]
        ws = O["ws"].t[0]
        part = lambda k: ws[self.lay[k][0] // 4:(self.lay[k][0] + self.lay[k][1]) // 4]
        assert (part("w")[T * W:].view(I32) == -1).all(), "the w region past its T W words is untouched"
        assert (part("red")[3 * T * W:].view(I32) == -1).all(), "the reduction region past its 3 T W words is untouched"
        assert (ws[(self.lay["w"][0] + self.lay["w"][1]) // 4:].view(I32) == -1).all(), "the workspace past its regions is untouched"
        o = dict(w=part("w")[:T * W].reshape(T, W).cpu(), lse=part("lse").reshape(2, T, B).cpu(), erat=part("erat").reshape(2, T, B).cpu(),
                 diag=part("diag").reshape(T, B).cpu(), term_loss=O["term_loss"].t[0].cpu(), loss=O["loss"].t[0, 0].cpu(), dls=O["dls"].t[0, 0].cpu(),
                 d_pooled=O["d_pooled"].t[0].reshape(d["b_local"], d["R"], d["D"]).cpu())
        for k, gd in O.items():
            RU.assert_guard_intact(gd, f"{d['name']} rank {r}: {k}")
        return o, O


def same_bytes(a, b, keys):
    return all(torch.equal(a[k].contiguous().view(I32), b[k].contiguous().view(I32)) for k in keys)


@pytest.mark.parametrize("case", SC.CASES, ids=[c["name"] for c in SC.CASES])
def test_stream_edges(H, case):
    d = SU.make_data(case, CASE_INDEX[case["name"]])
    ref = SU.reference(d)
    L = Launch(H, d)
    first = None
    for r in range(d["W"]):
        o, _ = L.run(r)
        same = first is not None and same_bytes(o, first, ("w", "lse", "erat", "diag"))
        SU.check(d, ref, r, o, common=not same)
        first = first or o
    again, _ = L.run(0)          # a second launch, into fresh NaN-filled buffers: the same bytes everywhere
    assert same_bytes(again, first, ("w", "lse", "erat", "diag") + OUT_KEYS), f"{d['name']}: two launches differ"


def test_refusals_write_nothing(H):
    """a short workspace and a bad row0 are bad arguments, D past the accepted set is unsupported: nothing is written"""
    d = SU.make_data(dict(name="refusals", terms=SC.TERMS3, R=3, B=6, D=7, b_local=2, kind="exact", present={}))
    L = Launch(H, d)
    O = L.outputs()
    f = H.lib().mca_contrastive_stream_fwd_bwd
    for over in (dict(ws_bytes=L.ws_bytes - 1), dict(row0=1), dict(b_local=4), dict(ws=None)):
        assert f(*L.args(O, 0, **over)) == BADARG, over
    assert f(*L.args(O, 0, D=SC.DMAX + 1, ws_bytes=1 << 40)) == UNSUPPORTED
    torch.cuda.synchronize()
    for k, gd in O.items():
        RU.assert_guard_intact(gd, k)
        assert (gd.t.view(I32) == -1).all(), k
    o, _ = L.run(1)          # and the same operands are a valid call
    SU.check(d, SU.reference(d), 1, o)


@pytest.fixture(scope="module")
def production():
    terms, R = SC.cmu_terms()
    p = SC.PRODUCTION
    d = SU.make_data(dict(name="production", terms=terms, R=R, B=p["B"], D=p["D"], b_local=p["b_local"], kind=p["kind"],
                         present={i: 1 + (i * 7 + 3) % 15 for i in range(p["B"])}), 99)          # every non-empty set of the four modalities
    return d, SU.reference(d)


def test_production_shape_against_reference(H, production):
    d, ref = production
    o, _ = Launch(H, d).run(0)
    SU.check(d, ref, 0, o)


def test_production_shape_against_dense_kernel(H, production):
    """the two kernels agree within the sum of their bounds, element by element"""
    d, ref = production
    stream_b, dense_b = ref["ranks"][0], ref["dense_ranks"][0]          # this kernel's bounds and the dense kernel's
    o, _ = Launch(H, d).run(0)
    T, B, R, D = d["T"], d["B"], d["R"], d["D"]
    dev = "cuda"
    ws = torch.empty(H.lib().mca_contrastive_workspace_bytes(B, T), dtype=torch.uint8, device=dev)
    terms = torch.tensor(d["terms"], dtype=torch.int64).to(I32).to(dev)
    out = dict(term_loss=torch.empty(T, device=dev), loss=torch.empty(1, device=dev), d_pooled=torch.empty(B, R, D, device=dev), dls=torch.empty(1, device=dev))
    pooled, present, s = d["pooled"].to(dev), d["present"].to(dev), d["s"].reshape(1).to(dev)
    H.call("mca_contrastive_fwd_bwd", pooled.data_ptr(), present.data_ptr(), terms.data_ptr(), T, s.data_ptr(), B, B, 0, R, D,
           out["term_loss"].data_ptr(), out["loss"].data_ptr(), out["d_pooled"].data_ptr(), out["dls"].data_ptr(), ws.data_ptr(), H.stream_ptr())
    torch.cuda.synchronize()
    live = dense_b["live"]
    assert live.all(), "four modalities, every term has valid rows"
    both = lambda k: stream_b[k] + dense_b[k]
    SU.close(o["term_loss"], out["term_loss"].cpu().double(), both("term_tol"), "term_loss, stream against dense", None, ("term",))
    SU.close(o["loss"].reshape(1), out["loss"].cpu().double(), both("loss_tol").reshape(1), "loss, stream against dense", None, ("element",))
    SU.close(o["dls"].reshape(1), out["dls"].cpu().double(), both("dls_tol").reshape(1), "d_logit_scale, stream against dense", None, ("element",))
    SU.close(o["d_pooled"], out["d_pooled"].cpu().double(), both("d_pooled_tol"), "d_pooled, stream against dense", None, ("row", "slot", "column"))


def test_print_worst_ratios():
    """last in the file: the largest error / bound ratio of every bounded quantity over the cases above (pytest -s shows it)"""
    seen = {k: v for k, v in SU.WORST.items() if k.startswith("stream ")}
    for k in sorted(seen):
        print(f"worst |got - ref| / bound  {k:24s} {seen[k]:.3f}")
    assert seen
