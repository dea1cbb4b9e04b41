"""mca_contrastive_fwd_bwd (csrc/loss.hip) element by element at the edges of its five kernels: every case of tests/loss_cases.py at
every rank, every input inside a frame, every output and the workspace inside a sentinel frame, w exactly, and stats, dG, the
losses and d_pooled against the float64 restatement within the bounds derived in docs/parity.md ("Contrastive loss: every element,
at the edges"); d_pooled also against the kernel's own dG, which isolates dpooled_kernel.  The workspace regions are read where
mca_dbg_contrastive_layout says they are.  tests/test_loss_edges_cpu.py shows without a GPU that the cases reach their paths, that
the checker finds planted faults and that the bounds are satisfiable.  Only valid calls are launched."""
import importlib

import pytest
import torch

import loss_cases as LC
import loss_edge_util as U
import row_edge_util as RU
from gemm_edge_util import _framed

pytestmark = pytest.mark.gpu
F32, I32 = torch.float32, torch.int32
BADARG, UNSUPPORTED = -1, -3
CASE_INDEX = {c["name"]: i for i, c in enumerate(LC.CASES)}


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def framed_ints(t):
    """an int32 tensor of any shape, flat inside a frame of 0xFF bytes (a stray present word has every bit, a stray slot is -1)"""
    flat = t.reshape(1, -1).to(I32)
    _, _, view = _framed(1, flat.shape[1], flat.shape[1] + 3, I32, "cuda", 0xFF, 0)
    view.copy_(flat)
    return view


class Launch:
    """the framed operands of one case on the device, and fresh sentinel-framed outputs for every call"""

    def __init__(self, H, d):
        self.H, self.d = H, d
        self.pooled = RU.vec_framed(d["pooled"].reshape(-1).cuda())
        self.present = framed_ints(d["present"])
        self.terms = framed_ints(torch.tensor(d["terms"], dtype=torch.int64))          # mca_loss_term: four 32-bit words
        self.s = RU.vec_framed(d["s"].reshape(1).cuda())
        self.lay = H.contrastive_layout(d["B"], d["T"])
        self.ws_bytes = H.lib().mca_contrastive_workspace_bytes(d["B"], d["T"])
        assert self.ws_bytes % 4 == 0 and self.ws_bytes >= self.lay["w"][0] + self.lay["w"][1]

    def outputs(self):
        d, g = self.d, lambda n: RU.guarded_out(1, n, n + 3, F32, device="cuda")
        return dict(term_loss=g(d["T"]), loss=g(1), dls=g(1), d_pooled=g(d["b_local"] * d["R"] * d["D"]), ws=g(self.ws_bytes // 4))

    def args(self, O, r, **over):
        d = self.d
        a = dict(pooled=self.pooled.data_ptr(), present=self.present.data_ptr(), terms=self.terms.data_ptr(), T=d["T"], s=self.s.data_ptr(), B=d["B"],
                 b_local=d["b_local"], row0=r * d["b_local"], R=d["R"], D=d["D"], term_loss=O["term_loss"].data_ptr(), loss=O["loss"].data_ptr(),
                 d_pooled=O["d_pooled"].data_ptr(), dls=O["dls"].data_ptr(), ws=O["ws"].data_ptr())
        a.update(over)
        return tuple(a.values()) + (self.H.stream_ptr(),)

    def run(self, r):
        """-> (the CPU tensors check() takes, the guarded outputs)"""
        d, O = self.d, self.outputs()
        self.H.call("mca_contrastive_fwd_bwd", *self.args(O, r))
        torch.cuda.synchronize()
        T, B, W = d["T"], d["B"], d["W"]
        ws = O["ws"].t[0]
        part = lambda k: ws[self.lay[k][0] // 4:(self.lay[k][0] + self.lay[k][1]) // 4]
        wreg = part("w")
        assert (wreg[T * W:].view(I32) == -1).all(), "the w region past its T W words is untouched"
        assert (ws[(self.lay["w"][0] + self.lay["w"][1]) // 4:].view(I32) == -1).all(), "the workspace past its three regions is untouched"
        o = dict(w=wreg[:T * W].reshape(T, W).cpu(), stats=part("stats").reshape(T, B, 4).cpu(), dG=part("G").reshape(T, B, B).cpu(),
                 term_loss=O["term_loss"].t[0].cpu(), loss=O["loss"].t[0, 0].cpu(), dls=O["dls"].t[0, 0].cpu(),
                 d_pooled=O["d_pooled"].t[0].reshape(d["b_local"], d["R"], d["D"]).cpu())
        for k, gd in O.items():
            RU.assert_guard_intact(gd, f"{d['name']} rank {r}: {k}")
        return o, O


@pytest.mark.parametrize("case", LC.CASES, ids=[c["name"] for c in LC.CASES])
def test_contrastive_edges(H, case):
    d = U.make_data(case, CASE_INDEX[case["name"]])
    ref = U.reference(d)
    L = Launch(H, d)
    first = None
    for r in range(d["W"]):
        o, _ = L.run(r)
        # w, stats and dG do not depend on row0: a later rank's are checked again only if they are not bitwise the first rank's
        same = first is not None and all(torch.equal(o[k].view(I32), first[k].view(I32)) for k in ("w", "stats", "dG"))
        U.check(d, ref, r, o, common=not same)
        first = first or o


def test_lds_limit_refused(H):
    """T W = 5040 needs 60480 bytes of LDS: unsupported, and nothing is written"""
    r = LC.LDS_REFUSED
    d = U.make_data(dict(name="lds-refused", terms=[LC.TERMS3[t % 3] for t in range(r["T"])], R=3, B=r["B"], D=3, b_local=r["b_local"], kind="exact", present={}))
    L = Launch(H, d)
    O = L.outputs()
    assert H.lib().mca_contrastive_fwd_bwd(*L.args(O, 0)) == UNSUPPORTED
    torch.cuda.synchronize()
    for k, gd in O.items():
        RU.assert_guard_intact(gd, k)
        assert (gd.t.view(I32) == -1).all(), k


def test_argument_refusals(H):
    """B % b_local, row0 % b_local, row0 + b_local > B, non-positive sizes and a null pointer for each argument: bad argument, nothing written"""
    d = U.make_data(dict(name="refusals", terms=LC.TERMS3, R=3, B=6, D=7, b_local=2, kind="exact", present={}))
    L = Launch(H, d)
    O = L.outputs()
    bad = [dict(b_local=4), dict(row0=1), dict(row0=3), dict(row0=6), dict(row0=-2), dict(b_local=0), dict(T=0), dict(B=0), dict(R=0), dict(D=0)]
    bad += [{k: None} for k in ("pooled", "present", "terms", "s", "term_loss", "loss", "d_pooled", "dls", "ws")]
    for over in bad:
        assert H.lib().mca_contrastive_fwd_bwd(*L.args(O, 0, **over)) == BADARG, over
    torch.cuda.synchronize()
    for k, gd in O.items():
        RU.assert_guard_intact(gd, k)
        assert (gd.t.view(I32) == -1).all(), k
    o, _ = L.run(1)          # and the same operands are a valid call
    U.check(d, U.reference(d), 1, o)


def test_print_worst_ratios():
    """last in the file: the largest error / bound ratio of every bounded quantity over the cases above (pytest -s shows it)"""
    seen = {k: v for k, v in U.WORST.items() if k.startswith("loss ")}
    for k in sorted(seen):
        print(f"worst |got - ref| / bound  {k:24s} {seen[k]:.3f}")
    assert seen
