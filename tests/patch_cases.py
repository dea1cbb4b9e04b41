"""Cases, data and checks of `mca_patch_ln_fwd` (tests/test_patch_encoder_gpu.py launches the library; tests/test_patch_encoder_cpu.py
runs the same drivers on the fp32 restatement below: every bound is satisfiable, and the data keeps the precondition's cap, without a
GPU).  Framing, float64 references and bounds are those of tests/row_edge_util.py (docs/parity.md, "Row and streaming kernels"): the
kernel's reduction is at most 16 sequential adds per lane and the 6 shuffle levels of a wavefront sum, which is what MEAN_REL and
RSTD_REL assume.

Two kinds of data per case.
  "plain"    every patch 2 randn + 0.5, re-centred where its |mean| exceeds 3.5 standard deviations (ln_input's rule), then patch 1
             all pad (more than one patch) and the last sample all pad (more than one sample).  The statistics and xn_bf16 of every
             non-pad row that meets row_edge_util's precondition (|mean| <= 4 std) are checked; at most MAX_EXCLUDED of the non-pad
             rows may miss it (here: none do).
  "special"  variant v of N_KINDS: row r is of kind (r + v) % N_KINDS (KINDS below), and in variant 0 the last sample is all pad.
             Over the variants every row of every case is of every kind.  xp, padmask and the all-pad rows are exact; a row that
             meets the precondition is checked like a plain one, the others (a lone real value among pads: |mean| / std = sqrt(P - 1);
             a constant row; a NaN) only for xp, padmask and the zero columns."""
import torch

from patch_twin import patches
from row_edge_util import BF, EPS, F32, assert_exact, assert_guard_intact, close, framed_in, guarded_out, ln_fwd_emulate32, ln_fwd_stats_ref, ln_fwd_y_ref, vec_framed

PAD = -10000.0
# (p1, p2, H/p1, W/p2, b).  The last two: a patch row wider than one workgroup's span (4 patches at P = 1024, 64 patches below
# P = 65), so that a row is cut into two spans and the second one is partial.
CASES = [(2, 3, 3, 5, 3), (16, 16, 2, 3, 2), (8, 20, 2, 2, 2), (32, 32, 1, 2, 1), (1, 64, 4, 1, 2), (64, 1, 1, 4, 2), (4, 4, 1, 1, 5),
         (32, 32, 1, 5, 1), (2, 3, 2, 70, 1)]
# the library's A/B forms (knob 13 of mca_debug_set; +-c caps the span at c patches, negative = direct): the product form, one patch per workgroup (every patch row cut into spans),
# and the wavefront-per-patch form that reads global memory directly (measured against the staged form in profiles/patch_encoder.md)
FORMS = {"staged": 0, "span1": 1, "direct": -64, "direct_span1": -1}
KINDS = ("all pad", "one real value, first", "one real value, last", "real with one pad value", "all nextafter(pad)",
         "real with a NaN", "real", "all pad but one nextafter(pad)")
N_KINDS = len(KINDS)
MAX_EXCLUDED = 0.05


def case_id(c):
    return "p%dx%d_g%dx%d_b%d" % c


def dims(c):
    p1, p2, gh, gw, b = c
    return dict(p1=p1, p2=p2, H=p1 * gh, W=p2 * gw, b=b, n=gh * gw, P=p1 * p2, kp=(p1 * p2 + 63) // 64 * 64, rows=b * gh * gw)


def unpatch(rows, c):
    """the inverse of patch_twin.patches: (b n, P) -> (b, H, W)"""
    p1, p2, gh, gw, b = c
    return rows.reshape(b, gh, gw, p1, p2).permute(0, 1, 3, 2, 4).reshape(b, gh * p1, gw * p2).contiguous()


def plain_rows(c, gen):
    d = dims(c)
    x = torch.randn(d["rows"], d["P"], generator=gen, device=gen.device) * 2 + 0.5
    xd = x.double()
    far = xd.mean(1).abs() > 3.5 * xd.std(1, unbiased=False)
    x[far] = (xd[far] - xd[far].mean(1, keepdim=True)).float()
    if d["rows"] > 1:
        x[1] = PAD
    if d["b"] > 1:
        x[-d["n"]:] = PAD
    return x


def special_rows(c, variant, gen):
    d = dims(c)
    P = d["P"]
    x = torch.randn(d["rows"], P, generator=gen, device=gen.device) * 2 + 0.5
    near = float(torch.nextafter(torch.tensor(PAD), torch.tensor(0.0)))
    for r in range(d["rows"]):
        k = (r + variant) % N_KINDS
        if k == 0:
            x[r] = PAD
        elif k in (1, 2):
            keep = float(x[r, 0])
            x[r] = PAD
            x[r, 0 if k == 1 else P - 1] = keep
        elif k == 3:
            x[r, (r * 7 + 3) % P] = PAD
        elif k == 4:
            x[r] = near
        elif k == 5:
            x[r, (r * 5 + 1) % P] = float("nan")
        elif k == 7:
            x[r] = PAD
            x[r, (r * 3 + 2) % P] = near
    if variant == 0:
        x[-d["n"]:] = PAD
    return x


def setup(c, rows, gen, ldv_extra=3, with_xp=True):
    """framed operands and guarded outputs of one launch of the (rows, P) patch rows `rows`"""
    d, dev = dims(c), gen.device
    ldv = d["W"] + ldv_extra
    vals = unpatch(rows, c)
    assert torch.equal(patches(vals, d["p1"], d["p2"]).reshape(d["rows"], d["P"]).view(torch.int32), rows.view(torch.int32))
    T = dict(d, ldv=ldv, x=rows, values=framed_in(vals.reshape(d["b"] * d["H"], d["W"]), ldv),
             gamma=vec_framed(torch.randn(d["P"], generator=gen, device=dev)), beta=vec_framed(torch.randn(d["P"], generator=gen, device=dev)))
    ld_bf = d["kp"] + 8
    O = dict(xp=guarded_out(d["rows"], d["P"], d["P"], F32, device=dev) if with_xp else None,
             xn=guarded_out(d["rows"], d["kp"], ld_bf, BF, device=dev), ld_bf=ld_bf,
             **{k: guarded_out(1, d["rows"], d["rows"] + 3, dt, device=dev) for k, dt in (("mean", F32), ("rstd", F32), ("mask", torch.uint8))})
    return T, O


def args(T, O):
    """mca_patch_ln_fwd's arguments up to the stream"""
    return (T["values"].data_ptr(), T["H"] * T["ldv"], T["ldv"], T["b"], T["H"], T["W"], T["p1"], T["p2"], T["gamma"].data_ptr(), T["beta"].data_ptr(),
            PAD, EPS, None if O["xp"] is None else O["xp"].data_ptr(), O["xn"].data_ptr(), O["ld_bf"], T["kp"], O["mean"].data_ptr(),
            O["rstd"].data_ptr(), O["mask"].data_ptr())


def emulate_into(T, O):
    """the CPU stand-in of the launch: the kernel's formula in fp32 torch, stored where the kernel stores"""
    x, P = T["x"], T["P"]
    pad = (x == PAD).all(1)
    mean, rstd, _, xn = ln_fwd_emulate32(x, T["gamma"], T["beta"], None, None)
    rs0 = torch.rsqrt(torch.tensor(EPS, dtype=F32))
    O["mean"].t[0].copy_(torch.where(pad, torch.tensor(PAD), mean))
    O["rstd"].t[0].copy_(torch.where(pad, rs0, rstd))
    O["mask"].t[0].copy_(pad.to(torch.uint8))
    O["xn"].t[:, :P] = torch.where(pad[:, None], T["beta"].to(BF)[None, :], xn)
    O["xn"].t[:, P:] = 0
    if O["xp"] is not None:
        O["xp"].t.copy_(x)


def checkable(x):
    """(pad rows, rows whose statistics the bounds cover: not pad, no NaN, |mean| <= 4 std with std > 0)"""
    pad = (x == PAD).all(1)
    xd = x.double()
    std = xd.std(1, unbiased=False) if x.shape[1] > 1 else torch.zeros_like(xd[:, 0])
    ok = ~pad & ~torch.isnan(x).any(1) & (std > 0) & (xd.mean(1).abs() <= 4 * std)
    return pad, ok


def check(T, O, what, cap=None):
    """every output of one launch.  cap: the largest fraction of the non-pad rows that may miss the precondition (None: no limit).
    -> (non-pad rows, rows among them the statistics were not checked on)"""
    x, P, kp, rows = T["x"], T["P"], T["kp"], T["rows"]
    pad, ok = checkable(x)
    n_live, n_skip = int((~pad).sum()), int((~pad & ~ok).sum())
    if cap is not None:
        assert n_skip <= cap * n_live, f"{what}: {n_skip} of {n_live} non-pad rows miss the precondition"
    if O["xp"] is not None:
        assert_exact(O["xp"].t.view(torch.int32), x.view(torch.int32), f"{what}: xp (as bits)")
    assert_exact(O["mask"].t[0], pad.to(torch.uint8), f"{what}: padmask (row = 0, column = the row)")
    mean_k, rstd_k, xn = O["mean"].t[0], O["rstd"].t[0], O["xn"].t
    if pad.any():
        assert_exact(mean_k[pad], torch.full_like(mean_k[pad], PAD), f"{what}: mean of all-pad rows")
        r0 = 1.0 / torch.sqrt(torch.tensor(EPS, dtype=F32, device=x.device).double())          # (EPS as the fp32 the kernel receives)
        assert bool(((rstd_k[pad].double() - r0).abs() <= 2.0 ** -23 * r0).all()), f"{what}: rstd of all-pad rows is rsqrt(eps) to one ulp"
        want = T["beta"].to(BF)[None, :].expand(int(pad.sum()), P)
        assert_exact(xn[pad][:, :P].view(torch.int16), want.contiguous().view(torch.int16), f"{what}: xn_bf16 of all-pad rows is bf16(beta) (as bits)")
    if ok.any():
        xo = x[ok]
        mean, tol_m, rstd, tol_r = ln_fwd_stats_ref(xo)
        close(mean_k[ok], mean, tol_m, f"{what}: mean (row = 0, column = the checked row)", "patch_ln mean")
        close(rstd_k[ok], rstd, tol_r, f"{what}: rstd (row = 0, column = the checked row)", "patch_ln rstd")
        _, _, yb, tol_yb = ln_fwd_y_ref(xo, T["gamma"], T["beta"], None, None, mean_k[ok], rstd_k[ok])
        close(xn[ok][:, :P], yb, tol_yb, f"{what}: xn_bf16", "patch_ln xn_bf16")
    if kp > P:
        assert_exact(xn[:, P:], torch.zeros_like(xn[:, P:]), f"{what}: xn_bf16 columns [P, kp)")
    for k in ("xp", "xn", "mean", "rstd", "mask"):
        if O[k] is not None:
            assert_guard_intact(O[k], f"{what}: {k}")
    return n_live, n_skip
