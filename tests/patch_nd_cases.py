"""Cases, data and framing of `mca_patch_nd_ln_fwd` (tests/test_patch_nd_gpu.py launches the library; tests/test_patch_nd_cpu.py runs
the same drivers on patch_cases' fp32 restatement).  The checks are patch_cases.check unchanged: the kernel's normalising stage is
the matrix kernel's (at most 16 sequential adds per lane and the 6 shuffle levels of a wavefront sum), so the references and bounds
of tests/row_edge_util.py (docs/parity.md, "Row and streaming kernels") hold for it as they stand.

Framing: every (sample, channel, frame) plane of H rows is followed by GUARD NaN rows inside one NaN frame with row stride ldv, so
the frame, channel and batch strides all step over guard rows; a gather that leaves its plane reads a NaN.

Data: patch_cases' "plain" rows (none misses the precondition) and its "special" kinds plus one more, rotated over the rows:
  "one channel all pad"   channel (r mod C) of the patch is -10000, the others real: not masked; |mean| / std = 1 / sqrt(C - 1), so
                          the statistics are checked (for C = 1 the kind is an all-pad patch)."""
import torch

import patch_cases as pc
from patch_nd_twin import patches_nd, unpatch_nd
from row_edge_util import BF, F32, framed_in, guarded_out, vec_framed

PAD = pc.PAD
GUARD = 2
# (C, pt, p1, p2, gt, gh, gw, b): the smallest shapes at which each mechanism can fail
CASES = [(3, 1, 2, 3, 1, 3, 5, 3),          # image, P = 18, scalar path, odd p2
         (3, 1, 16, 16, 1, 2, 3, 2),        # image, P = 768, float4 path
         (5, 1, 3, 4, 1, 2, 2, 2),          # image, P = 60, float4 path with P below one 64-column pad
         (4, 1, 16, 16, 1, 1, 5, 1),        # image, P = 1024, a 5-patch row cut into a span of 4 and a partial span
         (16, 1, 1, 64, 1, 4, 1, 2),        # image, many channels, p1 = 1
         (64, 1, 1, 1, 1, 2, 3, 2),         # image, P made of channels alone, one float per run
         (3, 1, 2, 3, 1, 2, 70, 1),         # image, 70 patches wide, more than a 64-patch span
         (3, 2, 2, 3, 2, 2, 3, 2),          # video, P = 36, scalar
         (3, 2, 8, 8, 2, 1, 2, 1),          # video, P = 384, float4
         (2, 4, 8, 16, 1, 1, 5, 1),         # video, P = 1024, span cut
         (2, 3, 1, 4, 3, 1, 1, 2)]          # video, temporal patches only
# C = T = pt = 1: the outputs of mca_patch_ln_fwd on the same matrix, bit for bit
DEGENERATE = [(1, 1, 4, 5, 1, 2, 2, 2), (1, 1, 16, 16, 1, 2, 3, 2)]
# knob 13 of mca_debug_set as this kernel honours it: |c| caps the span at c patches; it has no wavefront-per-patch form
FORMS = {"staged": 0, "span1": 1}
KINDS = pc.KINDS + ("one channel all pad",)
N_KINDS = len(KINDS)


def case_id(c):
    return "c%d_p%dx%dx%d_g%dx%dx%d_b%d" % c


def dims(c):
    C, pt, p1, p2, gt, gh, gw, b = c
    P, n = C * pt * p1 * p2, gt * gh * gw
    return dict(C=C, pt=pt, p1=p1, p2=p2, T=pt * gt, H=p1 * gh, W=p2 * gw, b=b, n=n, P=P, kp=(P + 63) // 64 * 64, rows=b * n,
                patch=(pt, p1, p2), grid=(gt, gh, gw))


def flat(c):
    """the patch_cases case with the same (rows, P) patch rows: patch_cases' data rules see rows only"""
    d = dims(c)
    return (1, d["P"], 1, d["n"], d["b"])


def plain_rows(c, gen):
    return pc.plain_rows(flat(c), gen)


def special_rows(c, variant, gen):
    """row r is of kind (r + variant) % N_KINDS; in variant 0 the last sample is all pad"""
    d = dims(c)
    P, C = d["P"], d["C"]
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
        elif k == 8:
            x[r].view(C, P // C)[r % C] = PAD          # (element order: the channel is the slowest axis of a patch)
    if variant == 0:
        x[-d["n"]:] = PAD
    return x


def setup(c, rows, gen, ldv_extra=3, with_xp=True):
    """framed operands and guarded outputs of one launch of the (rows, P) patch rows `rows`"""
    d, dev = dims(c), gen.device
    b, C, T, H, W = d["b"], d["C"], d["T"], d["H"], d["W"]
    ldv = W + ldv_extra
    vals = unpatch_nd(rows, C, d["patch"], d["grid"], b)
    assert torch.equal(patches_nd(vals, d["patch"]).reshape(d["rows"], d["P"]).view(torch.int32), rows.view(torch.int32))
    planes = torch.full((b * C * T, H + GUARD, W), float("nan"), device=dev)
    planes[:, :H] = vals.reshape(b * C * T, H, W)
    fs = (H + GUARD) * ldv
    T_ = dict(d, ldv=ldv, fstride=fs, cstride=T * fs, bstride=C * T * fs, x=rows, values=framed_in(planes.reshape(-1, W), ldv),
              gamma=vec_framed(torch.randn(d["P"], generator=gen, device=dev)), beta=vec_framed(torch.randn(d["P"], generator=gen, device=dev)))
    ld_bf = d["kp"] + 8
    O = dict(xp=guarded_out(d["rows"], d["P"], d["P"], F32, device=dev) if with_xp else None,
             xn=guarded_out(d["rows"], d["kp"], ld_bf, BF, device=dev), ld_bf=ld_bf,
             **{k: guarded_out(1, d["rows"], d["rows"] + 3, dt, device=dev) for k, dt in (("mean", F32), ("rstd", F32), ("mask", torch.uint8))})
    return T_, O


ARG = dict(values=0, bstride=1, cstride=2, fstride=3, ldv=4, b=5, C=6, T=7, H=8, W=9, pt=10, p1=11, p2=12, gamma=13, beta=14, xp=17,
           xn=18, ld_bf16=19, cols_pad=20, mean=21, rstd=22, mask=23)


def args(T, O):
    """mca_patch_nd_ln_fwd's arguments up to the stream (ARG: their positions)"""
    return (T["values"].data_ptr(), T["bstride"], T["cstride"], T["fstride"], T["ldv"], T["b"], T["C"], T["T"], T["H"], T["W"], T["pt"],
            T["p1"], T["p2"], T["gamma"].data_ptr(), T["beta"].data_ptr(), PAD, pc.EPS, None if O["xp"] is None else O["xp"].data_ptr(),
            O["xn"].data_ptr(), O["ld_bf"], T["kp"], O["mean"].data_ptr(), O["rstd"].data_ptr(), O["mask"].data_ptr())


def matrix_args(T, O):
    """mca_patch_ln_fwd's arguments for the same operands (C = T = pt = 1: one plane per sample)"""
    assert T["C"] == T["T"] == T["pt"] == 1
    return (T["values"].data_ptr(), T["bstride"], T["ldv"], T["b"], T["H"], T["W"], T["p1"], T["p2"], T["gamma"].data_ptr(),
            T["beta"].data_ptr(), PAD, pc.EPS, None if O["xp"] is None else O["xp"].data_ptr(), O["xn"].data_ptr(), O["ld_bf"], T["kp"],
            O["mean"].data_ptr(), O["rstd"].data_ptr(), O["mask"].data_ptr())


def gather_restated(T):
    """the kernel's addressing restated on the framed buffer itself: row ((s gt + ti) gh + hi) gw + wi, element
    ((c pt + dt) p1 + r) p2 + col  =  values[s, c, ti pt + dt, hi p1 + r, wi p2 + col] through the four strides"""
    v = T["values"]
    base = torch.as_strided(v, (T["b"], T["C"], T["T"], T["H"], T["W"]), (T["bstride"], T["cstride"], T["fstride"], T["ldv"], 1),
                            v.storage_offset())
    return patches_nd(base, T["patch"]).reshape(T["rows"], T["P"])
