"""References, derived bounds and checkers of the attention edge tests (tests/test_attention_edges_gpu.py; checked themselves by
tests/test_attention_edges_cpu.py; docs/parity.md, "Attention edges").  Plain torch on any device, no fixtures.

Every tensor here is in HEAD FORM (b, heads, rows, 64); heads4() / rows2() convert from and to the (b * rows, heads * 64) matrices
the kernels read and write.  The references compute in float64 from the STORED operands - q' (the pre-scaled q, log2 domain), k, v,
dO as bf16, o as bf16, lse as fp32 - so that a kernel and its reference share every input, and the backward is isolated from the
forward (it is given the kernel's own o, lse, delta and dvmean, each checked before).

    S  = q' k^T                  P  = 2^(S - lse) on pairs that are allowed and not padded, else 0 (0 on uniform rows: lse = +inf)
    dP = dO v^T                  delta = rowsum(dO o)             dS = P (dP - delta)
    dq = scale dS k              dk = ln2 dS^T q'                 dv = P^T dO + dvmean        (dvmean on EVERY key row)

Where the kernels round: dS once to bf16 in the dq pass; P and dS in the dkv pass and the one-pass kernels; P in the forward;
every output once to bf16 (not the fp32 dq form); everything else is fp32.  With u = 2^-8 the bf16 unit round-off, R = 2u = 2^-7 is
allowed per rounding (a rounding boundary may flip).  A 64-term fp32 dot product is within DOT = 2^-18 of the sum of its terms'
magnitudes; an n-term fp32 sum adds n ACC = n 2^-24 of the same absolute sum.  With sa_ij = sum_d |q'_id k_jd|:

    e_ij = R + ln2 DOT sa_ij                                            relative error of P
    a_ij = e_ij |dS_ij| + DOT P_ij (sum_d |dO_id v_jd| + |delta_i|)     absolute error of dS
    dq   : R |dq| + scale sum_j (a_ij + nk ACC |dS_ij|) |k_jd|          (fp32 form: 2^-22 |dq| in place of R |dq|)
    dk   : R |dk| + ln2 sum_i (a_ij + nq ACC |dS_ij|) |q'_id|
    dv   : R |dv| + sum_i (e_ij + nq ACC) P_ij |dO_id| + 2^-22 |dvmean_d|
    o    : R |o| + (R + nk ACC) sum_j P_ij |v_jd|;  uniform rows: R |o| + nk ACC mean_j |v_jd| around the float64 mean of V

A bound of 0 (dk of a padded key, dq of a row without a visible key) means the output must be exactly 0.  Two checks per tensor:
every element within its bound (NaN fails), and every row - 64 columns of one (sample, head, row or key) - with
||got - ref||_2 <= ROW_LIMIT ||bound||_2: an error of a few % of a whole row sits inside the worst-case element bound, not
inside half of its norm.  ROW_LIMIT is twice what emulate_* (fp32, rounded where the kernels round) reaches on the CPU."""
import math

import numpy as np
import torch

import attention_cases as AC

LN2 = 0.6931471805599453
LOG2E = 1.4426950408889634
SCALE = 0.125
C2 = SCALE * LOG2E          # what the stored q carries (MCA_ATTN_Q_PRESCALED)
R = 2.0 ** -7               # allowed per bf16 rounding: two unit round-offs
DOT = 2.0 ** -18            # 64 fp32 unit round-offs: a 64-term dot product accumulated in fp32
ACC = 2.0 ** -24            # one fp32 unit round-off
F32_OUT = 2.0 ** -22        # an fp32 output (dq in its fp32 form, dvmean): the scale multiply, the last additions
ROW_LIMIT = 0.5
SHOW = 8


def bf(x):
    return x.to(torch.bfloat16)


def heads4(x, b, heads=AC.HEADS):
    """(b * n, heads * 64) or (b, n, heads * 64), any strides -> (b, heads, n, 64) float64"""
    x = x.double().reshape(b, -1, heads, AC.DH)
    return x.permute(0, 2, 1, 3).contiguous()


def rows2(x4):
    """(b, heads, n, 64) -> (b * n, heads * 64)"""
    b, h, n, d = x4.shape
    return x4.permute(0, 2, 1, 3).reshape(b * n, h * d)


# ---- operands
def make_operands(case, variant="mca", pool=False, device="cpu"):
    """The operands of a case as the kernels store them (drawn on the CPU from the case's seed, so that the CPU and the GPU
    tests see the same numbers): randn as bf16, q pre-scaled by C2, dO randn."""
    c = AC.CASES[case]
    st = AC.structure(case, variant)
    pad = AC.padding(case)
    b, N, D = pad.shape[0], pad.shape[1], AC.HEADS * AC.DH
    g = torch.Generator().manual_seed(c["seed"] + (7 if pool else 0) + (13 if variant == "zorro" else 0))
    qkv = bf(torch.randn(b, N, 3 * D, generator=g))
    qkv[:, :, :D] = bf(qkv[:, :, :D].float() * C2)
    qmask = st.qmask_pool if pool else st.qmask_attn
    nq = len(qmask)
    qsrc = bf(torch.randn(nq, D, generator=g) * C2) if pool else None
    d_o = bf(torch.randn(b, nq, D, generator=g))
    blk = torch.from_numpy(AC.blocked(st, pad, pool))[:, None]          # (b, 1, nq, N)
    ops = dict(case=case, variant=variant, pool=pool, st=st, b=b, N=N, D=D, nq=nq, heads=AC.HEADS, pad=torch.from_numpy(pad),
               qkv=qkv, qsrc=qsrc, d_o=d_o, blk=blk, qmask_np=qmask)
    for k_, v_ in list(ops.items()):
        if torch.is_tensor(v_):
            ops[k_] = v_.to(device)
    return ops


def head_operands(ops):
    """(q', k, v, dO) in head form, float64; q' has batch 1 for the pooling query (q_bstride = 0)"""
    b, D = ops["b"], ops["D"]
    q = heads4(ops["qsrc"][None], 1) if ops["pool"] else heads4(ops["qkv"][:, :, :D], b)
    return q, heads4(ops["qkv"][:, :, D:2 * D], b), heads4(ops["qkv"][:, :, 2 * D:], b), heads4(ops["d_o"], b)


# ---- float64 references with their bounds
def forward_ref(q, k, v, blk):
    """dense softmax in float64 -> dict(o, o_bound, lse (+inf on uniform rows), lse_bound, uniform (b, 1, nq))
    lse_bound (log2 units): the fp32 score error through the softmax weights, sum_j P_ij DOT sa_ij; the row sum: nk additions, one
    ulp per exp2 and per rescale of a key tile, (nk + 2 tiles + 4) ACC relative, times log2 e; log2 and the last addition, 2^-22 of
    the magnitudes involved."""
    nk = k.shape[2]
    S = q @ k.transpose(-1, -2)
    uni = blk.all(-1)
    Sm = S.masked_fill(blk, float("-inf"))
    m = Sm.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    E = torch.exp2(Sm - m)
    l = E.sum(-1, keepdim=True)
    unie = uni[..., None].expand_as(l)
    P = torch.where(unie, torch.zeros_like(E), E / torch.where(unie, torch.ones_like(l), l))
    lse = torch.where(unie, torch.full_like(l, float("inf")), m + torch.log2(torch.where(unie, torch.ones_like(l), l)))[..., 0]
    o = P @ v
    vmean, vabs = v.mean(2, keepdim=True), v.abs().mean(2, keepdim=True)
    o = torch.where(unie, vmean.expand_as(o), o)
    o_bound = R * o.abs() + torch.where(unie, (nk * ACC * vabs).expand_as(o), (R + nk * ACC) * (P @ v.abs()))
    sa = q.abs() @ k.abs().transpose(-1, -2)
    lse_fin = torch.where(uni.expand_as(lse), torch.zeros_like(lse), lse)
    lse_bound = DOT * (P * sa).sum(-1) + LOG2E * (nk + 2 * ((nk + 63) // 64) + 4) * ACC + F32_OUT * (lse_fin.abs() + math.log2(nk))
    return dict(o=o, o_bound=o_bound, lse=lse, lse_bound=lse_bound, uniform=uni.expand_as(lse), P=P)


def delta_ref(d_o, o):
    """(delta, bound): the float64 row sum of dO o and DOT sum_d |dO o|"""
    t = d_o * o
    return t.sum(-1), DOT * t.abs().sum(-1)


def dvmean_ref(d_o, lse, nk):
    """(dvmean (b, h, 1, 64), bound): (1 / nk) sum of dO over the uniform rows; nq fp32 additions and the multiply"""
    uni = torch.isinf(lse)[..., None].double()
    nq = d_o.shape[2]
    return (d_o * uni).sum(2, keepdim=True) / nk, (nq + 2) * ACC * (d_o.abs() * uni).sum(2, keepdim=True) / nk


def backward_ref(q, k, v, d_o, lse, delta, dvmean, blk, scale=SCALE, dq_f32=False):
    """float64 gradients from the stored operands and the KERNEL's lse (b, h, nq), delta (b, h, nq), dvmean (b, h, 1, 64)
    -> dict(dq, dk, dv, dq_bound, dk_bound, dv_bound); dq per sample (for the pooling query too: q has batch 1)"""
    nq, nk = d_o.shape[2], k.shape[2]
    lse, delta, dvmean = lse.double()[..., None], delta.double()[..., None], dvmean.double()
    S = q @ k.transpose(-1, -2)
    P = torch.exp2(S - lse).masked_fill(blk, 0.0)
    dP = d_o @ v.transpose(-1, -2)
    dS = P * (dP - delta)
    dq, dk, dv = scale * (dS @ k), LN2 * (dS.transpose(-1, -2) @ q), P.transpose(-1, -2) @ d_o + dvmean
    sa = q.abs() @ k.abs().transpose(-1, -2)
    e = R + LN2 * DOT * sa
    a = e * dS.abs() + DOT * P * (d_o.abs() @ v.abs().transpose(-1, -2) + delta.abs())
    dq_b = (F32_OUT if dq_f32 else R) * dq.abs() + scale * ((a + nk * ACC * dS.abs()) @ k.abs())
    dk_b = R * dk.abs() + LN2 * ((a + nq * ACC * dS.abs()).transpose(-1, -2) @ q.abs())
    dv_b = R * dv.abs() + ((e + nq * ACC) * P).transpose(-1, -2) @ d_o.abs() + F32_OUT * dvmean.abs()
    return dict(dq=dq, dk=dk, dv=dv, dq_bound=dq_b, dk_bound=dk_b, dv_bound=dv_b)


# ---- fp32 emulations that round where the kernels round (the CPU test shows the bounds satisfiable with them)
def emulate_forward(q, k, v, blk):
    """-> (o bf16, lse fp32): fp32 scores, fp32 row sum of the unrounded P, P rounded to bf16 for P V, o rounded once"""
    q, k, v = q.float(), k.float(), v.float()
    Sm = (q @ k.transpose(-1, -2)).masked_fill(blk, float("-inf"))
    uni = blk.all(-1, keepdim=True)
    m = Sm.amax(-1, keepdim=True)
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    E = torch.exp2(Sm - m0)
    l = E.sum(-1, keepdim=True)
    o = (bf(E).float() @ v) / torch.where(uni, torch.ones_like(l), l)
    o = torch.where(uni.expand(*o.shape[:3], 1), v.mean(2, keepdim=True).expand_as(o), o)
    lse = torch.where(uni, torch.full_like(l, float("inf")), m0 + torch.log2(torch.where(uni, torch.ones_like(l), l)))[..., 0]
    return bf(o), lse.expand(o.shape[0], o.shape[1], -1).contiguous()


def emulate_prep(d_o, o, lse, nk):
    """-> (delta fp32 (b, h, nq), dvmean fp32 (b, h, 1, 64))"""
    d_o, o = d_o.float(), o.float()
    uni = torch.isinf(lse)[..., None].float()
    return (d_o * o).sum(-1), (d_o * uni).sum(2, keepdim=True) * (1.0 / nk)


def emulate_backward(q, k, v, d_o, lse, delta, dvmean, blk, scale=SCALE, dq_f32=False, lse_shift=None, skip=None):
    """-> (dq bf16 | fp32, dk bf16, dv bf16).  Mutations for the CPU test: lse_shift = (sample, head, row, amount) computes that row
    with lse + amount; skip = (sample, head, row0, rows, key0, keys) leaves those keys out of those rows' dq."""
    q, k, v, d_o = q.float(), k.float(), v.float(), d_o.float()
    lse = lse.float().clone()
    if lse_shift is not None:
        lse[lse_shift[0], lse_shift[1], lse_shift[2]] += lse_shift[3]
    s = q @ k.transpose(-1, -2) - lse[..., None]
    P = torch.exp2(s).masked_fill(blk, 0.0)
    dS = P * (d_o @ v.transpose(-1, -2) - delta.float()[..., None])
    Pb, dSb = bf(P).float(), bf(dS).float()
    dSq = dSb
    if skip is not None:
        s_, h_, r0, rn, k0, kn = skip
        dSq = dSb.clone()
        dSq[s_, h_, r0:r0 + rn, k0:k0 + kn] = 0.0
    dq = scale * (dSq @ k)
    dk = LN2 * (dSb.transpose(-1, -2) @ q)
    dv = Pb.transpose(-1, -2) @ d_o + dvmean.float()
    return (dq if dq_f32 else bf(dq)), bf(dk), bf(dv)


# ---- checkers
STATS = {}          # label -> [largest element ratio, largest row ratio] seen by check_rows (docs/parity.md quotes them)


def _where(bad, got, ref, bound, names):
    idx = bad.nonzero()[:SHOW].tolist()
    items = [tuple(i) + (float(got[tuple(i)]), float(ref[tuple(i)]), float(bound[tuple(i)])) for i in idx]
    return f"{int(bad.sum())} of {bad.numel()} elements outside their bound; first ({', '.join(names)}, got, want, bound): {items}"


def check_elements(got, ref, bound, what, names=("sample", "head", "row")):
    """|got - ref| <= bound at every element (float64; NaN fails; a bound of 0 asks for the exact value); returns the largest
    |got - ref| / bound"""
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    got, ref, bound = got.double(), ref.double(), bound.double()
    diff = (got - ref).abs()
    bad = ~(diff <= bound)
    if bad.any():
        raise AssertionError(f"{what}: " + _where(bad, got, ref, bound, names))
    ratio = torch.where(bound > 0, diff / bound.clamp_min(1e-300), torch.zeros_like(diff))
    return float(ratio.max()) if ratio.numel() else 0.0


def check_rows(got, ref, bound, what, label=None, row_limit=ROW_LIMIT, row_name="row"):
    """Both checks on a (b, heads, rows, 64) tensor: every element within its bound, and every (sample, head, row) with
    ||got - ref||_2 <= row_limit ||bound||_2 over the 64 columns.  Returns (largest element ratio, largest row ratio) and keeps
    the maxima per label in STATS."""
    assert got.dim() == 4 and got.shape[-1] == AC.DH, (what, got.shape)
    got, ref, bound = got.double(), ref.double(), bound.double()
    el = check_elements(got, ref, bound, what, names=("sample", "head", row_name, "column"))
    num, den = (got - ref).norm(dim=-1), bound.norm(dim=-1)
    ratio = torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(num))          # (den == 0: the elements were compared exactly)
    bad = ~(ratio <= row_limit)
    if bad.any():
        idx = bad.nonzero()[:SHOW].tolist()
        items = [tuple(i) + (round(float(ratio[tuple(i)]), 3),) for i in idx]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} rows beyond {row_limit} of their bound's norm (every element "
                             f"inside its bound; largest element ratio {el:.3f}); first (sample, head, {row_name}, ratio): {items}")
    rw = float(ratio.max()) if ratio.numel() else 0.0
    if label is not None:
        old = STATS.get(label, [0.0, 0.0])
        STATS[label] = [max(old[0], el), max(old[1], rw)]
    return el, rw


def check_forward(o4, lse, ref, what, label=None):
    """o by element and row; isinf(lse) == the reference's uniform rows exactly; lse of the other rows within lse_bound"""
    uni = ref["uniform"]
    got_uni = torch.isinf(lse) & (lse > 0)
    if not torch.equal(got_uni, uni):
        idx = (got_uni != uni).nonzero()[:SHOW].tolist()
        raise AssertionError(f"{what}: uniform rows (lse = +inf) differ from the reference's; first (sample, head, row): {idx}")
    fin = ~uni
    lse_d = torch.where(fin, lse.double(), torch.zeros_like(ref["lse"]))
    lse_r = torch.where(fin, ref["lse"], torch.zeros_like(ref["lse"]))
    el_l = check_elements(lse_d, lse_r, ref["lse_bound"], what + " lse")
    worst = float((lse_d - lse_r).abs().max())
    el, rw = check_rows(o4, ref["o"], ref["o_bound"], what + " o", label=None if label is None else label + " o")
    if label is not None:
        old = STATS.get(label + " lse", [0.0, 0.0])
        STATS[label + " lse"] = [max(old[0], el_l), max(old[1], worst)]          # (second figure: largest |lse - ref| in log2 units)
    return el, rw, el_l


def check_backward(dq4, dk4, dv4, ref, what, label=None):
    """dq (or None), dk, dv (or None for both) against backward_ref's result, both checks each"""
    out = {}
    if dq4 is not None:
        out["dq"] = check_rows(dq4, ref["dq"], ref["dq_bound"], what + " dq", None if label is None else label + " dq")
    if dk4 is not None:
        out["dk"] = check_rows(dk4, ref["dk"], ref["dk_bound"], what + " dk", None if label is None else label + " dk", row_name="key")
        out["dv"] = check_rows(dv4, ref["dv"], ref["dv_bound"], what + " dv", None if label is None else label + " dv", row_name="key")
    return out


def stats_table():
    return "\n".join(f"{k:40s} element {v[0]:.3f}  row {v[1]:.3g}" for k, v in sorted(STATS.items()))
