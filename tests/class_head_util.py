"""Helpers of the class-head kernels' edge tests (csrc/class_head.hip): the operands of a case inside frames, the float64 reference
(torch's own F.cross_entropy under autograd, and the closed forms of include/mca_hip.h that the CPU test holds against it), and the
per-element bounds.  Plain functions on any device; the references run on the CPU.

Operands are small integers as in task_head_util: pooled in {-2 .. 2}, w in {-2 .. 2} * w_scale with at most 8 non-zeros a row, bias
small integers, so every logit is an exact integer (|z| <= 8 * 4 * w_scale + 3), the row maximum m is exact and z - m is exact.
What rounds is the softmax and what follows.  With U the unit round-off, U' = 1.001 U, Ee = 2 EXPF_ULP U the relative error of expf
and El = 2 LOGF_ULP U that of logf (1 ulp <= 2 U relative, as eval_edge_util counts it), for ANY summation order:
  S = sum_c e_c     positive addends over 6 tree levels: relative Es = Ee + 6 U'
  lse = m + logf(S) Es (the error of S passes through the logarithm's derivative 1 / S) + El log S + U |lse| + 64 TINY (underflow)
  nll = lse - z_y   tol(lse) + U |nll|
  p = e / S         (Ee + Es + U) p + TINY
  row loss          (1 - eps) cw_y nll: three more roundings; the smoothing sum sum_c cw_c (lse - z_c) has positive addends: a
                    rounding each, 6 tree levels; (eps / C) and the product two more; one for the sum of the two terms
  W                 positive addends: ceil(b / 256) a lane + 6 tree levels + 2 across the waves: relative Kw U'
  loss[0]           sum_s tol(row_s) / W + (16 rows of a wave + 2 + the workgroups + the division + 1 + Kw) U' loss
  dz                the two bracketed terms of the header from tol(p), each rounding counted, times fl(task_weight / W): the
                    division, the product and W's own error (2 + Kw) U' |dz|
  gw, gb, d_pooled  as task_head_util states them, from tol(dz)
No figure for logf is to be found in the ROCm installation's documents, so LOGF_ULP is eval_edge_util's LOG1PF_ULP."""
import numpy as np
import torch
import torch.nn.functional as F

import class_head_cases as CC
from eval_edge_util import EXPF_ULP, LOG1PF_ULP, PAD, TINY, U, framed_i32, gather_index, gen, ints, out
from gemm_edge_util import assert_exact, assert_guard_intact
from row_edge_util import close, framed_in

F32, F64, I32 = torch.float32, torch.float64, torch.int32
U1 = 1.001 * U
LOGF_ULP = LOG1PF_ULP
EE, EL = 2 * EXPF_ULP * U, 2 * LOGF_ULP * U
ES = EE + 6 * U1
ANY_BITS = 0b101          # modalities 0 and 2 feed the readout slot; bit 1 alone does not make a row valid
DACT = 2.0
KEYS = ("pred", "loss", "d_pooled", "gw", "gb")


def cdiv(a, b):
    return (a + b - 1) // b


def workspace_floats(c):
    return cdiv(c["b"], CC.ROWS_PER_BLOCK) * (c["C"] * c["D"] + 4 * cdiv(c["C"], 4) + 4)


def eps32(c):
    """the label smoothing as the kernel receives it"""
    return float(np.float32(c["eps"]))


def row_plan(c):
    """-> (valid (b,) bool, y (b,) float): the valid rows spread over the batch; of the valid rows n_unlabelled carry -1 and the
    others a class: 0, C - 1 and 1 (the class of weight 0 under "zero1") come first, so each is present wherever the count allows.
    The labels of invalid rows are NaN (junk: NaN and values >= C in turn)."""
    b, C, nv, nu = c["b"], c["C"], c["n_valid"], c["n_unlabelled"]
    g = torch.Generator().manual_seed(11 + b + C)
    order = torch.randperm(b, generator=g)
    valid = torch.zeros(b, dtype=torch.bool)
    valid[order[:nv]] = True
    y = torch.full((b,), float("nan"))
    if c["junk"]:
        y[order[nv::2]] = float(C + 3)
    counted = order[:nv - nu]
    cls = torch.randint(0, C, (nv - nu,), generator=g)
    cls[:3] = torch.tensor([0, C - 1, 1])[:min(3, nv - nu)]
    y[counted] = cls.float()
    y[order[nv - nu:nv]] = -1.0
    return valid, y


def setup(c, dev):
    """-> T: the operands (framed views) of case c"""
    b, C, D, R = c["b"], c["C"], c["D"], c["R"]
    g = gen(67, dev)
    pooled = ints((b * R, D), g, 2)
    w = torch.zeros(C, D, device=dev)
    for l in range(C):
        cols = torch.unique(torch.cat([torch.tensor([0, D - 1], device=dev), torch.randint(0, D, (6,), generator=g, device=dev)]))
        w[l, cols] = ints((cols.numel(),), g, 2) * c["w_scale"]
    bias = ints((C,), g, 3)
    valid, y = row_plan(c)
    valid, y = valid.to(dev), y.to(dev)
    labels = torch.full((b, c["ld_labels"]), float("nan"), device=dev)          # the other columns are never read
    labels[:, c["col_off"]] = y
    T = dict(pooled=framed_in(pooled, D), w=framed_in(w, D), bias=framed_in(bias.reshape(1, -1), C + PAD)[0],
             labels=framed_in(labels, c["ld_labels"]), valid=valid, y=y, present=None, any_bits=0, din=None, gw0=None, gb0=None, cw=None)
    if c["cw"]:
        cw = 0.5 + 1.5 * torch.rand(C, generator=g, device=dev)
        cw[1] = 0.0
        T["cw"] = framed_in(cw.reshape(1, -1), C + PAD)[0]
    if c["presence"] != "null":
        other = torch.randint(0, 2, (b,), generator=g, device=dev) * 0b010
        mine = torch.tensor([0b001, 0b100, 0b101], device=dev)[torch.randint(0, 3, (b,), generator=g, device=dev)]
        T["present"] = framed_i32(torch.where(valid, mine | other, other))
        T["any_bits"] = ANY_BITS
    if c["din"]:
        T["din"] = framed_in(ints((b * R, D), g, 4), D)
    if c["acc"]:
        T["gw0"], T["gb0"] = ints((C, D), g, 3), ints((C,), g, 3)
    return T


def outputs(c, T, dev, short=0):
    """-> O: fresh guarded outputs (gw / gb hold their initial values when the case accumulates, d_pooled holds d_pooled_in when
    the case aliases them) and the workspace, `short` floats below the query"""
    b, C, D, R = c["b"], c["C"], c["D"], c["R"]
    O = dict(pred=out(b, C, dev, ld=C), loss=out(1, 3, dev, ld=3), d_pooled=out(b * R, D, dev, ld=D), gw=out(C, D, dev, ld=D),
             gb=out(1, C, dev, ld=C), ws=out(1, workspace_floats(c) - short, dev, ld=workspace_floats(c) - short))
    if c["acc"]:
        O["gw"].t.copy_(T["gw0"]); O["gb"].t[0].copy_(T["gb0"])
    if c["din"] == "alias":
        O["d_pooled"].t.copy_(T["din"])
    return O


def fill_args(hip, c, T, O):
    a = hip.ClassHeadArgs()
    p = lambda t: None if t is None else t.data_ptr()
    a.pooled, a.present, a.any_bits = p(T["pooled"]), p(T["present"]), T["any_bits"]
    a.b, a.R, a.D, a.slot = c["b"], c["R"], c["D"], c["slot"]
    a.w, a.bias, a.C = p(T["w"]), p(T["bias"]), c["C"]
    a.labels, a.ld_labels = T["labels"].data_ptr() + 4 * c["col_off"], c["ld_labels"]
    a.class_weights, a.label_smoothing = p(T["cw"]), c["eps"]
    a.task_weight, a.base_weight = c["tw"], c["base"]
    a.d_pooled_in = O["d_pooled"].data_ptr() if c["din"] == "alias" else p(T["din"])
    a.pred, a.loss, a.d_pooled = O["pred"].data_ptr(), O["loss"].data_ptr(), O["d_pooled"].data_ptr()
    a.gw, a.gb, a.accumulate = O["gw"].data_ptr(), O["gb"].data_ptr(), c["acc"]
    a.workspace, a.workspace_bytes = O["ws"].data_ptr(), 4 * O["ws"].cols
    return a


def _cpu(c, T, dt):
    """the operands of the references, on the CPU in dtype dt"""
    b, C, D, R, slot = c["b"], c["C"], c["D"], c["R"], c["slot"]
    f = lambda t: t.detach().cpu().to(dt)
    x = f(T["pooled"]).view(b, R, D)[:, slot]
    cw = f(T["cw"]) if T["cw"] is not None else torch.ones(C, dtype=dt)
    din = f(T["din"]).view(b, R, D) if c["din"] else torch.zeros(b, R, D, dtype=dt)
    gw0 = f(T["gw0"]) if c["acc"] else torch.zeros(C, D, dtype=dt)
    gb0 = f(T["gb0"]) if c["acc"] else torch.zeros(C, dtype=dt)
    valid, y = T["valid"].cpu(), T["y"].cpu()
    counted = valid & (y >= 0) & (y < C) & (y == y.floor())
    return x, f(T["w"]), f(T["bias"]), cw, din, gw0, gb0, valid, y, counted


def formulas(c, T, dt=F64, wrong=None):
    """The closed forms of include/mca_hip.h evaluated in dtype dt on the CPU -> every output and the intermediates the bounds need.
    wrong: one of the mistakes the CPU test shows the bound to catch."""
    b, C, D, R, slot = c["b"], c["C"], c["D"], c["R"], c["slot"]
    x, w, bias, cw, din, gw0, gb0, valid, y, counted = _cpu(c, T, dt)
    if wrong == "count_unlabelled":
        counted = valid & ((y == -1) | counted)
    yi = torch.where(counted, y, torch.zeros_like(y)).clamp_min(0).long()
    if wrong == "label_off":
        yi = (yi + 1) % C
    eps = torch.tensor(eps32(c), dtype=dt)
    z = x @ w.t() + bias[None, :]
    m = z.max(1, keepdim=True).values
    e = torch.exp(z) if wrong == "no_max" else torch.exp(z - m)
    S = e.sum(1, keepdim=True)
    lse = (torch.log(S) if wrong == "no_max" else m + torch.log(S))[:, 0]
    p = e / S
    cm = counted.to(dt)
    cwy = cw[yi] * cm
    W = cwy.sum()
    n = int(counted.sum())
    div = torch.tensor(float(n * C), dtype=dt) if wrong == "div_nC" else W
    onehot = F.one_hot(yi, C).to(dt)
    nll = lse - z.gather(1, yi[:, None])[:, 0]
    hard, soft = 1 - eps, eps / C
    cws = torch.ones_like(cw) if wrong == "smooth_nocw" else cw
    t1 = hard * cwy * nll
    ssum = (cws[None, :] * (lse[:, None] - z)).sum(1)
    t2 = soft * ssum * cm
    row = t1 + t2
    d1 = p - onehot
    a1 = hard * cwy[:, None] * d1
    d2 = p * cws.sum() - cws[None, :]
    a2 = soft * d2 * cm[:, None]
    inner = a1 + a2
    pos = bool(div > 0)
    sc = torch.tensor(c["tw"], dtype=dt) / div if pos else torch.zeros((), dtype=dt)
    dz = inner * sc
    loss = row.sum() / div if pos else torch.zeros((), dtype=dt)
    base = c["base"] if c["din"] else 0.0
    dp = base * din
    dp[:, slot] += dz @ w
    return dict(pred=z, loss=torch.stack([loss, torch.tensor(float(n), dtype=dt), W]), d_pooled=dp.reshape(b * R, D), gw=gw0 + dz.t() @ x,
                gb=gb0 + dz.sum(0), dz=dz, x=x, w=w, cw=cw, cwy=cwy, W=W, sc=sc, S=S[:, 0], lse=lse, nll=nll, p=p, t1=t1, t2=t2, ssum=ssum,
                a1=a1, a2=a2, d1=d1, d2=d2, inner=inner, cm=cm, hard=hard, soft=soft, z=z, dp_base=base * din, gw0=gw0, gb0=gb0, n=n)


def autograd_reference(c, T):
    """THE reference: float64 torch on the CPU, F.cross_entropy(weight, label_smoothing, ignore_index=-100, reduction="mean") over
    the rows with every uncounted label mapped to -100, autograd for dz, gw, gb and d_pooled"""
    b, C, D, R, slot = c["b"], c["C"], c["D"], c["R"], c["slot"]
    x, w, bias, cw, din, gw0, gb0, valid, y, counted = _cpu(c, T, F64)
    pooled = T["pooled"].detach().cpu().double().view(b, R, D).clone().requires_grad_(True)
    w, bias = w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    z = pooled[:, slot] @ w.t() + bias[None, :]
    z.retain_grad()
    n = int(counted.sum())
    target = torch.where(counted, y, torch.full_like(y, -100.0)).long()
    base = c["base"] if c["din"] else 0.0
    if n:
        loss = F.cross_entropy(z, target, weight=cw, label_smoothing=eps32(c), ignore_index=-100, reduction="mean")
        (c["tw"] * loss).backward()
        dz, gw, gb, dpg, lossv = z.grad, w.grad, bias.grad, pooled.grad, loss.detach()
    else:
        dz, gw, gb, dpg, lossv = torch.zeros_like(z), torch.zeros_like(w), torch.zeros_like(bias), torch.zeros_like(pooled), torch.zeros((), dtype=F64)
    Wv = (cw[target.clamp_min(0)] * counted.double()).sum()
    return dict(pred=z.detach(), loss=torch.stack([lossv, torch.tensor(float(n), dtype=F64), Wv]), d_pooled=(base * din + dpg).reshape(b * R, D),
                gw=gw0 + gw, gb=gb0 + gb, dz=dz)


def bounds(c, f, z_tol=None):
    """{output: per-element bound, None = exact} from the float64 closed forms f (the module docstring derives every term).
    z_tol (b, C): the logits are rounded dot products with this error (general data) instead of exact integers.  With zm its row
    maximum, the row maximum and lse move by at most zm, z_y by zm more, and p_c = exp(z_c - lse) by the factor exp(2 zm)."""
    b, C = c["b"], c["C"]
    nblk = cdiv(b, CC.ROWS_PER_BLOCK)
    kw = cdiv(b, 256) + 8
    cm, cw, cwy, p, hard, soft = f["cm"], f["cw"], f["cwy"], f["p"], float(f["hard"]), float(f["soft"])
    zm = torch.zeros(b, dtype=F64) if z_tol is None else z_tol.max(1).values
    lse_tol = 1.001 * ES + EL * torch.log(f["S"]) + U * f["lse"].abs() + 64 * TINY + zm + 2 * U * f["z"].abs().max(1).values * (z_tol is not None)
    nll_tol = lse_tol + U * f["nll"].abs() + zm
    p_tol = 1.001 * (EE + ES + U) * p + TINY + torch.expm1(2 * zm)[:, None] * p
    t1_tol = hard * cwy * nll_tol + 3 * U1 * f["t1"].abs()
    ssum_tol = (cw[None, :] * (lse_tol[:, None] + zm[:, None] + U1 * (f["lse"][:, None] - f["z"]).abs())).sum(1) + 7 * U1 * f["ssum"].abs()
    t2_tol = (soft * ssum_tol + 2 * U1 * (soft * f["ssum"]).abs()) * cm
    row_tol = t1_tol + t2_tol + U1 * (f["t1"] + f["t2"]).abs()
    W = float(f["W"])
    loss = f["loss"][0]
    tol = dict(pred=z_tol)
    k_loss = 16 + 2 + nblk + 1 + 1 + kw
    zero = torch.zeros((), dtype=F64)
    tol["loss"] = torch.stack([row_tol.sum() / W + k_loss * U1 * loss.abs() if W > 0 else zero, zero, kw * U1 * f["W"]])
    a1_tol = hard * cwy[:, None] * (p_tol + U * f["d1"].abs()) + 4 * U1 * f["a1"].abs()
    cw_sum = float(cw.sum())
    d2_tol = cw_sum * p_tol + 7 * U1 * p * cw_sum + U * f["d2"].abs()
    a2_tol = (soft * d2_tol + 2 * U1 * (soft * f["d2"]).abs()) * cm[:, None]
    inner_tol = a1_tol + a2_tol + U1 * (f["a1"].abs() + f["a2"].abs())
    sc = float(f["sc"])
    dz, x, w = f["dz"], f["x"], f["w"]
    dz_tol = inner_tol * abs(sc) + (2 + kw) * U1 * dz.abs()
    k = CC.ROWS_PER_BLOCK + nblk + 1
    tol["gw"] = dz_tol.t() @ x.abs() + k * U1 * (dz.abs().t() @ x.abs() + f["gw0"].abs())
    tol["gb"] = dz_tol.sum(0) + k * U1 * (dz.abs().sum(0) + f["gb0"].abs())
    dp_tol = torch.zeros_like(f["dp_base"])
    dp_tol[:, c["slot"]] = dz_tol @ w.abs() + (C + 1) * U1 * (dz.abs() @ w.abs() + f["dp_base"][:, c["slot"]].abs())
    tol["d_pooled"] = dp_tol.reshape(-1, dp_tol.shape[-1])
    tol["dz"] = dz_tol
    return tol


def general_reference(x, w, bias, y, valid, cw=None, eps=0.0, tw=1.0):
    """The class head on GENERAL fp32 data (the step tests: native pooled tokens): {output: (float64 reference, bound)} for pred,
    loss, dz, gw and gb of x (b, D), w (C, D), bias (C), y (b,) class indices or negatives, valid (b,) bool.  A logit is now a
    rounded dot product, |z_err| <= (D + 8) U' (sum_k |x_k w_k| + |bias|) as in task_head_util.head_reference."""
    b, D = x.shape
    C = w.shape[0]
    c = dict(b=b, C=C, D=D, R=1, slot=0, eps=eps, tw=tw, din=None, acc=0, base=0.0)
    T = dict(pooled=x.cpu(), w=w.cpu(), bias=bias.cpu(), cw=None if cw is None else cw.cpu(), valid=valid.cpu(), y=y.cpu().float(), din=None)
    f = formulas(c, T)
    z_tol = (D + 8) * U1 * (f["x"].abs() @ f["w"].abs().t() + bias.detach().cpu().double().abs()[None, :])
    tol = bounds(c, f, z_tol)
    return {k: (f[k], tol[k]) for k in ("pred", "loss", "dz", "gw", "gb")} | {"w": f["w"]}


def reference(c, T):
    """{output: (float64 reference from autograd, bound or None = exact)}"""
    ref, tol = autograd_reference(c, T), bounds(c, formulas(c, T))
    return {k: (ref[k], tol[k]) for k in KEYS}


def check_values(c, T, got, what="", ref=None):
    """got: {output: tensor} in the outputs' shapes, on any device"""
    ref, name = ref or reference(c, T), c["name"] + what
    for k in KEYS:
        want, tol = ref[k]
        g = got[k].detach().cpu()
        want = want.reshape(g.shape)
        assert torch.isfinite(g).all(), f"{name}: {k} is not finite"
        if tol is None:
            assert_exact(g.float(), want.float(), f"{name}: {k}")
        else:
            close(g, want, tol.reshape(g.shape), f"{name}: {k}", f"class head {k}")
    if c["n_valid"] == c["n_unlabelled"]:
        zero_g = (got["gw"].cpu() == (T["gw0"].cpu() if c["acc"] else 0)).all() and (got["gb"].cpu().reshape(-1) == (T["gb0"].cpu() if c["acc"] else 0)).all()
        assert (got["loss"].cpu() == 0).all() and zero_g, f"{name}: nothing is counted, yet a loss or a gradient"


def check(c, T, O, what="", ref=None):
    check_values(c, T, {k: O[k].t for k in KEYS}, what, ref)
    for k in KEYS + ("ws",):
        assert_guard_intact(O[k], f"{c['name']}{what}: {k}")
    assert (O["ws"].t.view(I32) != -1).all(), f"{c['name']}{what}: every word of a workspace of exactly the reported size is written"


def same_bits(O1, O2, name, keys=KEYS):
    for k in keys:
        if O1[k] is None:
            continue
        assert torch.equal(O1[k].t.contiguous().view(I32), O2[k].t.contiguous().view(I32)), f"{name}: {k} differs between two launches"


# ------------------------------------------------------------------------------------------------ mca_probe_head_ce_f32
PROBE_KEYS = ("pred", "dz", "da", "loss_part")


def probe_setup(c, dev):
    K, C, B, ldy = c["K"], c["C"], c["B"], c["ldy"]
    g = gen(71, dev)
    a_rows, y_rows = (B + 3 if c["aidx"] else B), (B + 2 if c["yidx"] else B)
    a = ints((a_rows, K), g, 2)
    w = ints((C, K), g, 1)
    bias = ints((C,), g, 3)
    aidx = gather_index(B, a_rows) if c["aidx"] else torch.arange(B)
    yidx = gather_index(B, y_rows) if c["yidx"] else torch.arange(B)
    a[aidx[0]] = 0.0          # batch row 0: a == 0, so z = bias and da is exactly 0
    ylab = torch.randint(0, C, (y_rows,), generator=torch.Generator().manual_seed(5 + B + C)).float()          # by LABEL row: yidx repeats one
    ylab[yidx[0]] = 0.0
    if B > 1 and yidx[B - 2] != yidx[0]:
        ylab[yidx[B - 2]] = float(C - 1)
    if c["bad"]:
        ylab[yidx[1]], ylab[yidx[2]] = float(C), 0.5
    y = ylab[yidx]
    labels = torch.full((y_rows, ldy), float("nan"), device=dev)          # only the last column is the label column
    labels[:, ldy - 1] = ylab.to(dev)
    T = dict(a=framed_in(a, K + PAD), w=framed_in(w, K), bias=framed_in(bias.reshape(1, -1), C + PAD)[0], labels=framed_in(labels, ldy),
             aidx=framed_i32(aidx.to(dev)) if c["aidx"] else None, yidx=framed_i32(yidx.to(dev)) if c["yidx"] else None, y=y)
    return T


def probe_outputs(c, dev):
    K, C, B = c["K"], c["C"], c["B"]
    return dict(pred=out(B, C, dev, ld=C), dz=out(B, C, dev, ld=C) if c["dz"] else None, da=out(B, K, dev, ld=K) if c["da"] else None,
                loss_part=out(1, cdiv(B, 4), dev))


def probe_args(H, c, T, O, **over):
    """the argument list of mca_probe_head_ce_f32; over: replaced sizes / NULL pointers of the refusal tests"""
    p = lambda t: None if t is None else t.data_ptr()
    v = dict(a=p(T["a"]), lda=c["K"] + PAD, aidx=p(T["aidx"]), K=c["K"], w=p(T["w"]), bias=p(T["bias"]), C=c["C"],
             labels=T["labels"].data_ptr() + 4 * (c["ldy"] - 1), ldy=c["ldy"], yidx=p(T["yidx"]), B=c["B"], pred=p(O["pred"]), dz=p(O["dz"]),
             da=p(O["da"]), dact=DACT, loss_part=p(O["loss_part"]))
    v.update(over)
    return [v[k] for k in ("a", "lda", "aidx", "K", "w", "bias", "C", "labels", "ldy", "yidx", "B", "pred", "dz", "da", "dact", "loss_part")] \
        + [H.stream_ptr() if torch.cuda.is_available() else None]


def probe_formulas(c, T, dt=F64):
    """nn.CrossEntropyLoss() on the batch rows whose label is a class index (the divisor stays B), closed forms in dtype dt"""
    B, C = c["B"], c["C"]
    f = lambda t: t.detach().cpu().to(dt)
    a = f(T["a"])[T["aidx"].cpu().long()] if T["aidx"] is not None else f(T["a"])
    w = f(T["w"])
    lab = T["labels"].detach().cpu()[:, c["ldy"] - 1]
    y = lab[T["yidx"].cpu().long()] if T["yidx"] is not None else lab[:B]          # as the kernel gathers them
    assert torch.equal(y, T["y"])
    ok = (y >= 0) & (y < C) & (y == y.floor())
    yi = torch.where(ok, y, torch.zeros_like(y)).long()
    z = a @ w.t() + f(T["bias"])[None, :]
    m = z.max(1, keepdim=True).values
    e = torch.exp(z - m)
    S = e.sum(1, keepdim=True)
    lse = m[:, 0] + torch.log(S[:, 0])
    p = e / S
    okf = ok.to(dt)
    nll = (lse - z.gather(1, yi[:, None])[:, 0]) * okf
    inv = torch.tensor(float(np.float32(1) / np.float32(B)), dtype=dt)
    d1 = (p - F.one_hot(yi, C).to(dt)) * okf[:, None]
    dz = d1 * inv
    da = torch.where(a > 0, (dz @ w) * DACT, torch.zeros(B, c["K"], dtype=dt))
    pad = torch.zeros(cdiv(B, 4) * 4, dtype=dt)
    pad[:B] = nll
    return dict(pred=z, dz=dz, da=da, loss_part=pad.reshape(-1, 4).sum(1), a=a, w=w, S=S[:, 0], lse=lse, nll=nll, p=p, d1=d1, inv=float(inv), ok=okf)


def probe_autograd(c, T):
    """torch's own: B * mean-reduced cross_entropy over the rows with a class index, divided by B again"""
    f = probe_formulas(c, T)
    z = f["pred"].clone().requires_grad_(True)
    ok = f["ok"].bool()
    target = torch.where(ok, T["y"], torch.full_like(T["y"], -100.0)).long()
    assert ok.any()
    rows = F.cross_entropy(z, target, ignore_index=-100, reduction="none")
    (rows.sum() * f["inv"]).backward()
    return dict(rows=rows.detach(), dz=z.grad)


def probe_reference(c, T):
    f = probe_formulas(c, T)
    B, C = c["B"], c["C"]
    lse_tol = 1.001 * ES + EL * torch.log(f["S"]) + U * f["lse"].abs() + 64 * TINY
    nll_tol = (lse_tol + U * f["nll"].abs()) * f["ok"]
    p_tol = 1.001 * (EE + ES + U) * f["p"] + TINY
    dz_tol = ((p_tol + U * f["d1"].abs()) * f["inv"] + 2 * U * f["dz"].abs()) * f["ok"][:, None]
    w = f["w"]
    da_tol = torch.where(f["a"] > 0, DACT * (dz_tol @ w.abs() + (C + 2) * U * (f["dz"].abs() @ w.abs())), torch.zeros_like(f["da"]))
    pad = torch.zeros(cdiv(B, 4) * 4, dtype=F64)
    pad[:B] = nll_tol
    part_tol = pad.reshape(-1, 4).sum(1) + 3 * U1 * f["loss_part"].abs()
    return dict(pred=(f["pred"], None), dz=(f["dz"], dz_tol), da=(f["da"], da_tol), loss_part=(f["loss_part"], part_tol)), f


def probe_check_values(c, T, got, what=""):
    ref, f = probe_reference(c, T)
    name = c["name"] + what
    for k in PROBE_KEYS:
        if got.get(k) is None:
            continue
        want, tol = ref[k]
        g = got[k].detach().cpu()
        g = g.reshape(want.shape)
        assert torch.isfinite(g).all(), f"{name}: {k} is not finite"
        if tol is None:
            assert_exact(g.float(), want.float(), f"{name}: {k}")
        else:
            close(g, want, tol, f"{name}: {k}", f"probe ce head {k}")
    if got.get("da") is not None:
        assert (got["da"].cpu()[f["a"] <= 0] == 0).all(), f"{name}: da is exactly 0 where a <= 0"
    if c["bad"] and got.get("dz") is not None:
        assert (got["dz"].cpu()[1:3] == 0).all(), f"{name}: a row whose label is no class index has a gradient"


def probe_check(c, T, O, what=""):
    probe_check_values(c, T, {k: (None if O[k] is None else (O[k].t if k != "loss_part" else O[k].t[0])) for k in PROBE_KEYS}, what)
    for k in PROBE_KEYS:
        if O[k] is not None:
            assert_guard_intact(O[k], f"{c['name']}{what}: {k}")
