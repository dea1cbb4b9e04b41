"""Helpers of the task-head kernel's edge tests: the operands of a case inside frames, the float64 reference of
mca_task_head_fwd_bwd as include/mca_hip.h states it, the bounds, and an fp32 restatement of the kernel (csrc/task_head.hip) that the
CPU test holds against the reference before the table meets the GPU.  Plain functions on any device.

Operands are small integers: pooled in {-2 .. 2}, w in {-2 .. 2} with at most 8 non-zeros a row (the first and the last column among
them), bias and labels small integers, so every logit is an exact integer with |z| <= 8 * 4 + 3, every L1 / MSE element loss an exact
integer and, where fl(task_weight / n) is a power of two, dz and every sum of the kernel exact whatever its order: those outputs are
compared with assert_exact.  Otherwise (n no power of two, BCE) the bounds below hold for ANY summation order of at most K_ROUND
roundings on a path, from the unit round-off U alone:
  dz        two roundings (the scale's division, the product): (2U + U^2) |dz|; BCE adds the expf / log1pf terms of eval_edge_util.head_ref
  gw, gb    sum_s tol(dz_s) |x_s| + K U' sum_s |dz_s x_s|, K = 64 rows of a workgroup + the workgroups + the accumulate add
  d_pooled  sum_l tol(dz_l) |w_l| + (L + 1) U' (sum_l |dz_l w_l| + |base d_in|)
  loss      sum tol(le) / n + K_LOSS U' loss, K_LOSS = 6 tree levels + 16 rows of a wave + 2 + the workgroups + the division + 1
with U' = 1.001 U (k U / (1 - k U) for k <= 200)."""
import math

import numpy as np
import torch

import task_head_cases as TC
from eval_edge_util import EXPF_ULP, LOG1PF_ULP, PAD, PLANT_Z, TINY, U, framed_i32, gen, ints, out
from gemm_edge_util import assert_exact, assert_guard_intact
from row_edge_util import close, framed_in

F32, F64, I32 = torch.float32, torch.float64, torch.int32
U1 = 1.001 * U
ANY_BITS = 0b101          # modalities 0 and 2 feed the readout slot; bit 1 alone does not make a row valid


def cdiv(a, b):
    return (a + b - 1) // b


def workspace_floats(c):
    return cdiv(c["b"], TC.ROWS_PER_BLOCK) * (c["L"] * c["D"] + 4 * cdiv(c["L"], 4) + 4)


def valid_rows(c):
    """(b,) bool on the CPU: which rows are valid; the valid ones are spread over the batch, the last row among them when any is"""
    b, nv = c["b"], c["n_valid"]
    v = torch.zeros(b, dtype=torch.bool)
    if nv:
        order = torch.randperm(b, generator=torch.Generator().manual_seed(7 + b))
        v[order[:nv]] = True
        if not v[b - 1]:
            v[order[0]], v[b - 1] = False, True
    return v


def setup(c, dev):
    """-> T: the operands (framed views) of case c"""
    b, L, D, R, slot = c["b"], c["L"], c["D"], c["R"], c["slot"]
    g = gen(61, dev)
    pooled = ints((b * R, D), g, 2)
    w = torch.zeros(L, D, device=dev)
    for l in range(L):
        cols = torch.unique(torch.cat([torch.tensor([0, D - 1], device=dev), torch.randint(0, D, (6,), generator=g, device=dev)]))
        w[l, cols] = ints((cols.numel(),), g, 2)
    valid = valid_rows(c).to(dev)
    x = pooled.view(b, R, D)[:, slot]
    if c["loss"] == TC.BCE:
        bias = torch.tensor([PLANT_Z[l % len(PLANT_Z)] for l in range(L)], device=dev)
        y = torch.randint(0, 2, (b, L), generator=g, device=dev).float()
    else:
        bias = ints((L,), g, 3)
        y = ints((b, L), g, 4)
        last = int(valid.nonzero()[-1]) if valid.any() else 0
        y[last] = x[last] @ w.t() + bias          # e == 0 at every label of the last valid row: sign(0) = 0
    labels = torch.full((b, c["ld_labels"]), float("nan"), device=dev)          # columns outside the window are never read
    labels[:, c["col_off"]:c["col_off"] + L] = y
    labels[~valid] = float("nan")                                               # nor are the labels of an invalid row
    T = dict(pooled=framed_in(pooled, D), w=framed_in(w, D), bias=framed_in(bias.reshape(1, -1), L + PAD)[0],
             labels=framed_in(labels, c["ld_labels"]), valid=valid, present=None, any_bits=0, din=None, gw0=None, gb0=None)
    if c["presence"] != "null":
        other = torch.randint(0, 2, (b,), generator=g, device=dev) * 0b010
        mine = torch.tensor([0b001, 0b100, 0b101], device=dev)[torch.randint(0, 3, (b,), generator=g, device=dev)]
        T["present"] = framed_i32(torch.where(valid, mine | other, other))
        T["any_bits"] = ANY_BITS
    if c["din"]:
        T["din"] = framed_in(ints((b * R, D), g, 4), D)
    if c["acc"]:
        T["gw0"], T["gb0"] = ints((L, D), g, 3), ints((L,), g, 3)
    return T


def outputs(c, T, dev, short=0):
    """-> O: fresh guarded outputs (gw / gb hold their initial values when the case accumulates, d_pooled holds d_pooled_in when
    the case aliases them) and the workspace, `short` floats below the query"""
    b, L, D, R = c["b"], c["L"], c["D"], c["R"]
    O = dict(pred=out(b, L, dev, ld=L), loss=out(1, 2, dev, ld=2), d_pooled=out(b * R, D, dev, ld=D), gw=out(L, D, dev, ld=D),
             gb=out(1, L, dev, ld=L), ws=out(1, workspace_floats(c) - short, dev, ld=workspace_floats(c) - short))
    if c["acc"]:
        O["gw"].t.copy_(T["gw0"]); O["gb"].t[0].copy_(T["gb0"])
    if c["din"] == "alias":
        O["d_pooled"].t.copy_(T["din"])
    return O


def fill_args(hip, c, T, O):
    a = hip.TaskHeadArgs()
    p = lambda t: None if t is None else t.data_ptr()
    a.pooled, a.present, a.any_bits = p(T["pooled"]), p(T["present"]), T["any_bits"]
    a.b, a.R, a.D, a.slot = c["b"], c["R"], c["D"], c["slot"]
    a.w, a.bias, a.L = p(T["w"]), p(T["bias"]), c["L"]
    a.labels, a.ld_labels, a.loss_type = T["labels"].data_ptr() + 4 * c["col_off"], c["ld_labels"], c["loss"]
    a.task_weight, a.base_weight = c["tw"], c["base"]
    a.d_pooled_in = O["d_pooled"].data_ptr() if c["din"] == "alias" else p(T["din"])
    a.pred, a.loss, a.d_pooled = O["pred"].data_ptr(), O["loss"].data_ptr(), O["d_pooled"].data_ptr()
    a.gw, a.gb, a.accumulate = O["gw"].data_ptr(), O["gb"].data_ptr(), c["acc"]
    a.workspace, a.workspace_bytes = O["ws"].data_ptr(), 4 * O["ws"].cols
    return a


def scale32(c):
    """the kernel's fl(task_weight / (n_valid * L)) and whether it is a power of two (then every L1 / MSE result is exact)"""
    if c["n_valid"] == 0:
        return 0.0, True
    s = float(np.float32(c["tw"]) / (np.float32(c["n_valid"]) * np.float32(c["L"])))
    return s, math.frexp(s)[0] == 0.5


def _window(c, T):
    return T["labels"][:, c["col_off"]:c["col_off"] + c["L"]]


def reference(c, T):
    """{output: (float64 reference, bound or None = exact)} for pred (b, L), loss (2,), d_pooled (b*R, D), gw (L, D), gb (L,)"""
    b, L, D, R, slot = c["b"], c["L"], c["D"], c["R"], c["slot"]
    dev = T["pooled"].device
    valid, nv = T["valid"], c["n_valid"]
    x = T["pooled"].view(b, R, D)[:, slot].double()
    w = T["w"].double()
    z = x @ w.t() + T["bias"].double()[None, :]
    y = torch.where(valid[:, None], _window(c, T).double(), torch.zeros(b, L, dtype=F64, device=dev))
    e = z - y
    n = nv * L
    _, pow2 = scale32(c)
    sc = c["tw"] / n if n else 0.0
    zero = torch.zeros_like(z)
    if c["loss"] == TC.L1:
        le, le_tol, g, g_tol = e.abs(), zero, torch.sign(e), zero
    elif c["loss"] == TC.MSE:
        le, le_tol, g, g_tol = e * e, zero, 2 * e, zero
    else:
        sp = torch.log1p(torch.exp(-z.abs()))
        lin = z.clamp_min(0) - z * y
        le = lin + sp
        le_tol = 2 * (EXPF_ULP + LOG1PF_ULP) * U * sp + 3 * U * (lin.abs() + sp) + TINY
        s = torch.sigmoid(z)
        g = s - y
        g_tol = 2 * EXPF_ULP * U * s * (1 - s) + 3 * U * s + U * g.abs() + TINY
    vm = valid[:, None].double()
    le, le_tol, dz = le * vm, le_tol * vm, g * vm * sc
    exact = c["loss"] != TC.BCE and pow2
    dz_tol = (g_tol * vm * sc + (2 * U + U * U) * dz.abs()) if not exact else zero
    nblk = cdiv(b, TC.ROWS_PER_BLOCK)
    ref = dict(pred=(z, None))
    loss = le.sum() / n if n else torch.zeros((), dtype=F64, device=dev)
    k_loss = 6 + 16 + 2 + nblk + 1 + 1
    loss_tol = None if exact else torch.stack([le_tol.sum() / max(n, 1) + k_loss * U1 * loss.abs(), torch.zeros((), dtype=F64, device=dev)])
    ref["loss"] = (torch.stack([loss, torch.tensor(float(nv), dtype=F64, device=dev)]), loss_tol)
    k = TC.ROWS_PER_BLOCK + nblk + 1
    gw, gb = dz.t() @ x, dz.sum(0)
    gw0 = T["gw0"].double() if c["acc"] else torch.zeros_like(gw)
    gb0 = T["gb0"].double() if c["acc"] else torch.zeros_like(gb)
    ref["gw"] = (gw0 + gw, None if exact else dz_tol.t() @ x.abs() + k * U1 * (dz.abs().t() @ x.abs() + gw0.abs()))
    ref["gb"] = (gb0 + gb, None if exact else dz_tol.sum(0) + k * U1 * (dz.abs().sum(0) + gb0.abs()))
    base = c["base"] if c["din"] else 0.0
    dp = base * T["din"].double().view(b, R, D) if c["din"] else torch.zeros(b, R, D, dtype=F64, device=dev)
    dp_tol = torch.zeros_like(dp)
    if not exact:
        dp_tol[:, slot] = dz_tol @ w.abs() + (L + 1) * U1 * (dz.abs() @ w.abs() + dp[:, slot].abs())
    dp[:, slot] += dz @ w
    ref["d_pooled"] = (dp.view(b * R, D), None if exact else dp_tol.view(b * R, D))
    return ref


def head_reference(x, w, bias, y, valid, loss, tw=1.0):
    """The head on GENERAL fp32 data (the step tests: native pooled tokens): float64 references and bounds of pred, the loss, dz, gw
    and gb for x (b, D), w (L, D), bias (L), y (b, L), valid (b,) bool.  On top of the bounds above a logit is now a rounded dot
    product: |z_err| <= (D + 8) U' (sum_k |x_k w_k| + |bias|) for any order of its D + 1 additions and the 6 tree levels, which
    reaches dz through the loss's derivative (2 for MSE, at most 1/4 for BCE)."""
    x, w, bias, y = x.double(), w.double(), bias.double(), y.double()
    b, D = x.shape
    L = w.shape[0]
    nv = int(valid.sum())
    n = nv * L
    sc = tw / n if n else 0.0
    z = x @ w.t() + bias[None, :]
    z_tol = (D + 8) * U1 * (x.abs() @ w.abs().t() + bias.abs()[None, :])
    y = torch.where(valid[:, None], y, torch.zeros_like(y))
    e = z - y
    assert loss in (TC.MSE, TC.BCE)          # (L1's sign at a logit within its own error has no useful bound)
    if loss == TC.MSE:
        le, le_tol, g, g_tol = e * e, 2 * e.abs() * z_tol + z_tol * z_tol + U * e * e, 2 * e, 2 * z_tol + 2 * U * e.abs()
    else:
        sp = torch.log1p(torch.exp(-z.abs()))
        lin = z.clamp_min(0) - z * y
        le = lin + sp
        le_tol = 2 * (EXPF_ULP + LOG1PF_ULP) * U * sp + 3 * U * (lin.abs() + sp) + TINY + z_tol
        s = torch.sigmoid(z)
        g = s - y
        g_tol = 2 * EXPF_ULP * U * s * (1 - s) + 3 * U * s + U * g.abs() + TINY + 0.25 * z_tol
    vm = valid[:, None].double()
    le, le_tol, dz = le * vm, le_tol * vm, g * vm * sc
    dz_tol = g_tol * vm * sc + (2 * U + U * U) * dz.abs()
    nblk = cdiv(b, TC.ROWS_PER_BLOCK)
    k = TC.ROWS_PER_BLOCK + nblk + 1
    lossv = le.sum() / n if n else le.sum() * 0
    return dict(pred=(z, z_tol), loss=(lossv, le_tol.sum() / max(n, 1) + (6 + 16 + 2 + nblk + 2) * U1 * lossv.abs()), dz=(dz, dz_tol),
                gw=(dz.t() @ x, dz_tol.t() @ x.abs() + k * U1 * (dz.abs().t() @ x.abs())),
                gb=(dz.sum(0), dz_tol.sum(0) + k * U1 * dz.abs().sum(0)), w=w)


def _fma(a, x, acc):
    """fl(a * x + acc) with one rounding (the product of two fp32 numbers is exact in float64; the double rounding of the sum is
    inside every bound above)"""
    return (a.double() * x.double() + acc.double()).float()


def emulate_into(c, T, O):
    """csrc/task_head.hip restated in fp32 torch, stored into O as the kernel stores: the reference's own check on the CPU"""
    b, L, D, R, slot = c["b"], c["L"], c["D"], c["R"], c["slot"]
    dev = T["pooled"].device
    valid = T["valid"]
    x = T["pooled"].view(b, R, D)[:, slot]
    w = T["w"]
    z = x @ w.t() + T["bias"][None, :]          # integers: exact in any order
    y = torch.where(valid[:, None], _window(c, T), torch.zeros(b, L, device=dev))
    e = z - y
    if c["loss"] == TC.L1:
        le, g = e.abs(), torch.sign(e)
    elif c["loss"] == TC.MSE:
        le, g = e * e, 2.0 * e
    else:
        le = z.clamp_min(0) - z * y + torch.log1p(torch.exp(-z.abs()))
        g = 1.0 / (1.0 + torch.exp(-z)) - y
    sc, _ = scale32(c)
    vm = valid[:, None]
    dz = torch.where(vm, g * torch.tensor(sc, dtype=F32, device=dev), torch.zeros_like(g))
    le = torch.where(vm, le, torch.zeros_like(le))
    O["pred"].t.copy_(z)
    nblk = cdiv(b, TC.ROWS_PER_BLOCK)
    gw, gb, ls = torch.zeros(L, D, device=dev), torch.zeros(L, device=dev), torch.zeros((), device=dev)
    for blk in range(nblk):
        pw, pb = torch.zeros(L, D, device=dev), torch.zeros(L, device=dev)
        for s in range(blk * TC.ROWS_PER_BLOCK, min(b, (blk + 1) * TC.ROWS_PER_BLOCK)):
            pw = _fma(dz[s][:, None], x[s][None, :], pw)
            pb = pb + dz[s]
        gw, gb, ls = gw + pw, gb + pb, ls + le[blk * TC.ROWS_PER_BLOCK:(blk + 1) * TC.ROWS_PER_BLOCK].sum()
    if c["acc"]:
        gw, gb = gw + T["gw0"], gb + T["gb0"]
    O["gw"].t.copy_(gw); O["gb"].t[0].copy_(gb)
    nv = c["n_valid"]
    O["loss"].t[0].copy_(torch.stack([ls / float(nv * L) if nv else torch.zeros((), device=dev), torch.tensor(float(nv), device=dev)]))
    dx = torch.zeros(b, D, device=dev)
    for l in range(L):
        dx = _fma(dz[:, l, None], w[l][None, :], dx)
    base = torch.tensor(c["base"] if c["din"] else 0.0, dtype=F32, device=dev)
    din = T["din"].view(b, R, D) if c["din"] else torch.zeros(b, R, D, device=dev)
    add = torch.zeros(b, R, D, device=dev)
    add[:, slot] = dx
    O["d_pooled"].t.copy_(_fma(base, din, add).view(b * R, D))
    O["ws"].t.fill_(0.0)


def check(c, T, O, what=""):
    ref, name = reference(c, T), c["name"] + what
    for k in ("pred", "loss", "d_pooled", "gw", "gb"):
        want, tol = ref[k]
        got = O[k].t
        want = want.reshape(got.shape)
        assert torch.isfinite(got).all(), f"{name}: {k} is not finite"
        if tol is None:
            assert_exact(got, want.float(), f"{name}: {k}")
        else:
            close(got, want, tol.reshape(got.shape), f"{name}: {k}", f"task head {k}")
        assert_guard_intact(O[k], f"{name}: {k}")
    assert (O["ws"].t.view(I32) != -1).all(), f"{name}: every word of a workspace of exactly the reported size is written"
    assert_guard_intact(O["ws"], f"{name}: workspace")
    if c["n_valid"] == 0:
        assert (O["loss"].t == 0).all() and (O["gw"].t == 0).all() and (O["gb"].t == 0).all(), f"{name}: no valid row, yet a loss or gradient"


def same_bits(O1, O2, name):
    for k in ("pred", "loss", "d_pooled", "gw", "gb"):
        assert torch.equal(O1[k].t.contiguous().view(I32), O2[k].t.contiguous().view(I32)), f"{name}: {k} differs between two launches"
