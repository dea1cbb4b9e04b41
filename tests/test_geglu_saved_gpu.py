"""The saved-factor GEGLU forms on the GPU (include/mca_hip.h: mca_gemm_nt_geglu_fwd_saved / _bwd_saved and their stand-alone
siblings), every element, inside the guards of tests/gemm_edge_util.py.  Which kernel each shape reaches is asserted without a
GPU in tests/test_geglu_saved_cpu.py, which also shows that the bounds used here are satisfiable and tight."""
import copy
import importlib

import pytest
import torch

import gemm_edge_util as U
import geglu_saved_util as S
from util_small import small_config, rel_err, to_device

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FWD, BWD = S.FWD, S.BWD


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    hip = importlib.import_module("mca-paper_amd.hip")
    hip.lib()
    return hip


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("rows,ip,D", FWD)
def test_forward_saved(H, rows, ip, D):
    """Every M here is no multiple of 256: the row tail, the partner exchange and a walk over several tiles.  g of the saved form
    is bit-equal to g of the unsaved form; s meets the bound of geglu_saved_util.saved_ref against the float64 factors of the
    unsaved form's h (itself bit-exact: W1 = integers / 16); nothing outside s and g is stored to."""
    fusedk = rows >= 2048 and D >= 192
    ldh, ldg = (2 * ip + 8, ip + 8) if fusedk else (2 * ip, ip)          # the unfused pair takes packed rows only
    gn = gen(43)
    x, w1 = U.int_bf16(rows, D, D + 8, gn), U.int_bf16(2 * ip, D, D + 16, gn, scale=2.0 ** -4)
    out = {}
    for form in ("mca_gemm_nt_geglu_fwd", "mca_gemm_nt_geglu_fwd_saved"):
        h, g = U.guarded_out(rows, 2 * ip, ldh, BF, device="cuda"), U.guarded_out(rows, ip, ldg, BF, device="cuda")
        H.call(form, x.data_ptr(), D + 8, w1.data_ptr(), D + 16, h.data_ptr(), ldh, g.data_ptr(), ldg, ip, rows, D, H.stream_ptr())
        out[form] = (h, g)
    torch.cuda.synchronize()
    (h, g), (s, g_saved) = out["mca_gemm_nt_geglu_fwd"], out["mca_gemm_nt_geglu_fwd_saved"]
    U.assert_exact(h.t, U.matmul64(x, w1).to(BF), "h of the unsaved form")
    assert torch.equal(bits(g_saved.t), bits(g.t)), f"g differs at {int((bits(g_saved.t) != bits(g.t)).sum())} elements"
    ref, tol = S.saved_ref(h.t, ip)
    worst = float(((s.t.double() - ref).abs() / tol.clamp_min(1e-300)).max())          # (both halves of h zero: bound 0, difference 0)
    print(f"saved forward {rows, ip, D}: largest |s - ref| / bound = {worst:.4f}")
    U.assert_close_elementwise(s.t, ref, tol, "s")
    U.assert_guard_intact(s, "s")
    U.assert_guard_intact(g_saved, "g")


@pytest.mark.parametrize("rows,ip", [(3, 1416), (4099, 2056)])
def test_standalone_forward_saved(H, rows, ip):
    """mca_geglu_fwd_saved: h -> s in place, g bit-equal to mca_geglu_fwd's (a second pass of the grid at the larger shape)"""
    gn = gen(5)
    h = (torch.randn(rows, 2 * ip, device="cuda", generator=gn) * 2).to(BF)
    g, g_saved = U.guarded_out(rows, ip, ip, BF, device="cuda"), U.guarded_out(rows, ip, ip, BF, device="cuda")
    s = U.guarded_out(rows, 2 * ip, 2 * ip, BF, device="cuda")
    s.t.copy_(h)
    H.call("mca_geglu_fwd", h.data_ptr(), g.data_ptr(), rows, ip, H.stream_ptr())
    H.call("mca_geglu_fwd_saved", s.data_ptr(), g_saved.data_ptr(), rows, ip, H.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(bits(g_saved.t), bits(g.t))
    U.assert_close_elementwise(s.t, *S.saved_ref(h, ip), "s")
    U.assert_guard_intact(s, "s")
    U.assert_guard_intact(g_saved, "g")


# ------------------------------------------------------------------------------------------------ backward
def backward_case(rows, ip, D, ldh):
    gn = gen(41)
    h = torch.randn(rows, 2 * ip, device="cuda", generator=gn).to(BF)
    s = S.factors64(h, ip).to(BF)          # the matching factors: exact, rounded once
    dx, w2T = U.int_bf16(rows, D, D, gn), U.int_bf16(ip, D, D + 8, gn, scale=2.0 ** -4)
    return U.framed_copy(h, ldh), U.framed_copy(s, ldh), dx, w2T


@pytest.mark.parametrize("rows,ip,D", BWD)
def test_backward_saved(H, rows, ip, D):
    """dg = dx . w2T^T is exact (w2T = integers / 16) and so is the fp32 product dg * s: dh must EQUAL bf16(dg * s), the stored s
    times dg rounded once, at every element - the last row tile and all three column tiles of ip = 384 included.  Against the
    unsaved backward on the matching h: within 2^-7 |dh| + the absolute floor of the unsaved form's own bound."""
    ldh = 2 * ip + 8
    h, s, dx, w2T = backward_case(rows, ip, D, ldh)
    dh, dh_saved = U.guarded_out(rows, 2 * ip, ldh, BF, device="cuda"), U.guarded_out(rows, 2 * ip, ldh, BF, device="cuda")
    args = lambda src, dst: (dx.data_ptr(), D, w2T.data_ptr(), D + 8, src.data_ptr(), dst.data_ptr(), ldh, ip, rows, D, H.stream_ptr())
    H.call("mca_gemm_nt_geglu_bwd", *args(h, dh))
    H.call("mca_gemm_nt_geglu_bwd_saved", *args(s, dh_saved))
    torch.cuda.synchronize()
    dg = U.matmul64(dx, w2T)
    prod = torch.cat([dg, dg], 1) * s.double()
    assert (prod.float().double() == prod).all()
    U.assert_exact(dh_saved.t, prod.to(BF), "dh of the saved form")
    U.assert_guard_intact(dh_saved, "dh")
    tol = S.bwd_vs_unsaved_tol(dh.t, dg, h, ip)
    print(f"saved backward {rows, ip, D}: largest |dh_saved - dh| / bound = {float(((dh_saved.t.double() - dh.t.double()).abs() / tol.clamp_min(1e-300)).max()):.4f}")
    U.assert_close_elementwise(dh_saved.t, dh.t.double(), tol, "dh against the unsaved form")


@pytest.mark.parametrize("rows,ip", [(3, 1416), (4099, 2056)])
def test_standalone_backward_saved(H, rows, ip):
    gn = gen(6)
    s = (torch.randn(rows, 2 * ip, device="cuda", generator=gn)).to(BF)
    dg = (torch.randn(rows, ip, device="cuda", generator=gn) * 3).to(BF)
    dh = U.guarded_out(rows, 2 * ip, 2 * ip, BF, device="cuda")
    H.call("mca_geglu_bwd_saved", dg.data_ptr(), s.data_ptr(), dh.data_ptr(), rows, ip, H.stream_ptr())
    torch.cuda.synchronize()
    prod = torch.cat([dg, dg], 1).double() * s.double()          # 8 x 8 significant bits: exact in fp32
    U.assert_exact(dh.t, prod.to(BF), "dh")
    U.assert_guard_intact(dh, "dh")


# ------------------------------------------------------------------------------------------------ step
@pytest.fixture(scope="module")
def steps(H):
    """one forward + backward of the small configuration with the flag on, and two with it off; computed once"""
    P = importlib.import_module("mca-paper_amd")
    cfg = small_config("mca")
    batch = to_device(P.data.synthetic_batch(cfg, 6, seed=5, p_drop=0.3), "cuda")

    def run(flag):
        torch.manual_seed(43)
        model = P.MCA(**copy.deepcopy(cfg)).cuda()
        eng = model.engine
        eng.geglu_saved_factors = flag
        H.profile_start({"mca_gemm_nt_geglu_fwd", "mca_gemm_nt_geglu_bwd"})
        try:
            out = model(batch)
            out["loss"].backward()
        finally:
            launched = H.profile_stop()
        torch.cuda.synchronize()
        holds = {a["h_holds"] for a in eng.workspace(6)["layers"]}
        tensors = {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}
        return dict(out=tensors, grads={n: p.grad.detach().clone() for n, p in model.named_parameters()}, launched=launched, holds=holds,
                    depth=cfg["depth"])
    return dict(on=run(True), off=run(False), off2=run(False))


def test_step_forward_is_bit_equal(steps):
    on, off = steps["on"], steps["off"]
    assert on["holds"] == {"s"} and off["holds"] == {"h"}
    assert set(on["out"]) == set(off["out"]) and "loss" in on["out"] and len(on["out"]) > 1          # the loss and the pooled outputs
    for k, v in off["out"].items():
        assert torch.equal(on["out"][k], v), k


def test_step_profile_keys_are_those_of_the_unsaved_forms(steps):
    for run in (steps["on"], steps["off"]):
        assert set(run["launched"]) == {"mca_gemm_nt_geglu_fwd", "mca_gemm_nt_geglu_bwd"}
        assert all(v[0] == run["depth"] for v in run["launched"].values())


def test_step_gradients(steps):
    """The forward is bit-equal, so the gradients differ only through dh.  Per element, dh of the saved form is
    bf16(dg * bf16(f)) against bf16(dg * f) of the unsaved form: three bf16 roundings apart at most (one on the factor, the final one
    of either form), 3 * 2^-9 of the value with a bf16 rounding counted as 2^-9 of the value (its typical size; include/mca_hip.h
    counts it so).  Every gradient is
    linear in the dh of the layers above it, so to first order - and taking the perturbations to add up no more coherently than the
    signal does - a gradient moves by at most depth * 3 * 2^-9 of its norm.  On top of that the two runs draw the order of their
    fp32 atomics independently: twice the largest spread between two flag-off runs."""
    on, off, off2 = steps["on"], steps["off"], steps["off2"]
    spread = max(rel_err(off2["grads"][n], off["grads"][n]) for n in off["grads"])
    bound = 2 * spread + on["depth"] * 3 * 2.0 ** -9
    worst = {n: rel_err(on["grads"][n], off["grads"][n]) for n in off["grads"]}
    print(f"saved step: spread of two flag-off runs {spread:.3e}, bound {bound:.3e}, largest gradient difference {max(worst.values()):.3e}")
    assert spread <= 1e-3, spread
    for n, d in worst.items():
        assert d <= bound, (n, d, bound)
    assert max(worst.values()) > 0          # the flag did something


def test_a_flag_switched_between_forward_and_backward_is_refused(H):
    P = importlib.import_module("mca-paper_amd")
    cfg = small_config("mca")
    batch = to_device(P.data.synthetic_batch(cfg, 6, seed=5, p_drop=0.3), "cuda")
    for first, attr in ((True, "geglu_saved_factors"), (False, "geglu_saved_factors"), (True, "fuse_geglu_bwd")):
        torch.manual_seed(43)
        model = P.MCA(**copy.deepcopy(cfg)).cuda()
        eng = model.engine
        eng.geglu_saved_factors = first
        out = model(batch)
        setattr(eng, attr, not getattr(eng, attr))
        with pytest.raises(AssertionError, match="GEGLU buffer"):
            out["loss"].backward()
        torch.cuda.synchronize()
