"""Helpers of the row-kernel edge tests (tests/test_row_edges_gpu.py; checked themselves by tests/test_row_edges_cpu.py): the
framing of tests/gemm_edge_util.py (inputs inside NaN, outputs inside a sentinel), the float64 references of the LayerNorm,
streaming and optimizer kernels, the element-wise bounds derived in docs/parity.md ("Row and streaming kernels"), and fp32
restatements of the kernels' formulas that show every bound satisfiable without a GPU.  Plain functions on any device."""
import torch

from gemm_edge_util import (BF16_STEP, GUARD_ROWS, LN_REL, SENTINEL, SHOW, _framed, assert_close_elementwise, assert_exact,  # noqa: F401
                            assert_guard_intact, framed_copy, geglu_bwd_ref, geglu_fwd_ref, guarded_out, ln_stats32)

EPS = 1e-5
MEAN_REL = 2.0 ** -19          # at most 16 sequential adds, 6 shuffle levels and a division, relative to mean_j |x_j|
RSTD_REL = 2.0 ** -18          # the same for the squares + the subtraction, the square and a one-ulp rsqrtf, relative to rstd
SUM_ULP = 2.0 ** -24           # one fp32 rounding, relative to the partial sum it rounds
F32, BF = torch.float32, torch.bfloat16


# ------------------------------------------------------------------------------------------------ framing
IN_NAN = {4: (torch.int32, 0x7FC00BAD), 2: (torch.int16, 0x7FC1)}          # the NaN of an input frame, by element size


def framed_in(src, ld, byte_off=0):
    """framed_copy with ANOTHER NaN in the frame than the outputs' sentinel.  A NaN keeps its bits through a kernel's arithmetic and
    through the truncating side of a bf16 rounding, so a kernel that reads the 0xFF.. frame of an input and stores the result into
    the 0xFF.. guard of an output would store what is there already: the one stray store the guards could not see."""
    view = framed_copy(src, ld, byte_off)
    it, bits = IN_NAN[view.element_size()]
    rows = view.shape[0]
    whole = torch.as_strided(view, (rows + 2 * GUARD_ROWS, ld), (ld, 1), view.storage_offset() - GUARD_ROWS * ld)
    whole.view(it)[torch.isnan(whole)] = bits
    assert torch.isnan(whole[:GUARD_ROWS]).all() and torch.isnan(whole[-GUARD_ROWS:]).all() and torch.isnan(whole[:, src.shape[1]:]).all()
    view.copy_(src)
    return view


def nan_rows_(view, mask):
    """masked rows of an input hold NaN: a kernel that loads them and does not select them away poisons its output"""
    if mask is not None:
        view[mask.bool()] = float("nan")
    return view


def int_rows(rows, cols, ld, gen, amp, byte_off=0):
    """[rows, cols] fp32 integers in {-amp .. amp} inside a NaN frame with row stride ld"""
    v = torch.randint(-amp, amp + 1, (rows, cols), generator=gen, device=gen.device).float()
    return framed_in(v, ld, byte_off)


def assert_rows_untouched(view, rows_idx, what="output"):
    """the listed rows of a guarded view (rows of a packed placement that no kernel row maps to) still hold the sentinel"""
    if len(rows_idx) == 0:
        return
    it = torch.int16 if view.element_size() == 2 else torch.int32
    sub = view[rows_idx]
    bad = (sub.contiguous().view(it) != -1)
    if bad.any():
        i, j = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} elements stored in rows no kernel row maps to; first (row, column): ({int(rows_idx[i])}, {j})")


def assert_exact_rows(got, ref, what="vector"):
    """assert_exact for a 1-d tensor: reported as (row, column) = (0, index)"""
    assert_exact(got.reshape(1, -1), ref.reshape(1, -1), what)


def assert_close_rows(got, ref, tol, what="vector"):
    assert_close_elementwise(got.reshape(1, -1), ref.reshape(1, -1), tol.reshape(1, -1), what)


WORST = {}          # output name -> largest |got - ref| / bound seen so far (where the bound is not 0): the figures of docs/parity.md


def close(got, ref, tol, what, key):
    """assert_close_elementwise that also keeps the largest error / bound ratio under `key`"""
    if got.dim() == 1:
        got, ref, tol = got.reshape(1, -1), ref.reshape(1, -1), tol.reshape(1, -1)
    assert_close_elementwise(got, ref, tol, what)
    pos = tol > 0
    if pos.any():          # (a check that passed: the ratio is at most 1)
        WORST[key] = max(WORST.get(key, 0.0), float(((got.double() - ref.double()).abs()[pos] / tol.double()[pos]).max()))


# ------------------------------------------------------------------------------------------------ LayerNorm forward
def ln_input(rows, cols, ld, gen, mask=None, byte_off=0):
    """x = 2 randn + 0.5 in a NaN frame; a row whose |mean| exceeds four standard deviations is re-centred (a few rows of very few
    columns: there the variance would lose the digits the rstd bound counts on).  Masked rows NaN.  cols == 1: std is 0 by
    definition and x - mean is exactly 0 in any arithmetic, so the condition says nothing and the draw stays."""
    x = torch.randn(rows, cols, generator=gen, device=gen.device) * 2 + 0.5
    if cols > 1:
        xd = x.double()
        far = xd.mean(1).abs() > 3.5 * xd.std(1, unbiased=False)
        x[far] = (xd[far] - xd[far].mean(1, keepdim=True)).float()
        xd = x.double()
        assert (xd.mean(1).abs() <= 4 * xd.std(1, unbiased=False)).all(), "each row's |mean| is at most four times its standard deviation"
    return nan_rows_(framed_in(x, ld, byte_off), mask)


def _live(mask, rows, device):
    return torch.ones(rows, dtype=torch.bool, device=device) if mask is None else ~mask.bool()


def ln_fwd_stats_ref(x, mask=None):
    """(mean, mean bound, rstd, rstd bound) in float64 from the fp32 x; masked rows: 0 with bound 0"""
    live = _live(mask, x.shape[0], x.device)
    xd = torch.where(live[:, None], x.double(), torch.zeros((), dtype=torch.float64, device=x.device))
    mean = xd.mean(1)
    rstd = 1.0 / torch.sqrt(xd.var(1, unbiased=False) + EPS)
    z = torch.zeros_like(mean)
    return (torch.where(live, mean, z), torch.where(live, MEAN_REL * xd.abs().mean(1), z),
            torch.where(live, rstd, z), torch.where(live, RSTD_REL * rstd, z))


def ln_fwd_y_ref(x, gamma, beta, add_rows, mask, mean_k, rstd_k):
    """(y reference, y bound, y_bf16 reference, y_bf16 bound) in float64 from the fp32 inputs and the KERNEL's (already checked)
    mean and rstd.  add_rows: the [rows, cols] rows of the add table each row receives, or None.  Masked rows: exactly 0 (+ add)."""
    live = _live(mask, x.shape[0], x.device)[:, None]
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    xd = torch.where(live, x.double(), zero)
    mu, rs, ga = mean_k.double()[:, None], rstd_k.double()[:, None], gamma.double()[None, :]
    be = beta.double()[None, :] if beta is not None else zero
    core = torch.where(live, (xd - mu) * rs * ga + be, zero)
    tol_core = torch.where(live, LN_REL * ((xd.abs() + mu.abs()) * rs * ga.abs() + be.abs()), zero)
    if add_rows is not None:
        ad = add_rows.double()
        y, tol_y = core + ad, torch.where(live, tol_core + LN_REL * ad.abs(), zero)
    else:
        y, tol_y = core, tol_core
    return y, tol_y, core, tol_core + BF16_STEP * core.abs()


def ln_fwd_emulate32(x, gamma, beta, add_rows, mask, eps=EPS):
    """the forward kernels' formula in fp32 torch, rounded where they round: (mean, rstd, y fp32, y_bf16)"""
    live = _live(mask, x.shape[0], x.device)
    xz = torch.where(live[:, None], x, torch.zeros((), device=x.device))
    cols = torch.tensor(float(x.shape[1]), dtype=F32, device=x.device)
    mean = xz.sum(1) / cols
    d = xz - mean[:, None]
    rstd = torch.rsqrt((d * d).sum(1) / cols + torch.tensor(eps, dtype=F32, device=x.device))
    t = d * rstd[:, None] * gamma[None, :]
    if beta is not None:
        t = t + beta[None, :]
    t = torch.where(live[:, None], t, torch.zeros((), device=x.device))
    y = t + add_rows if add_rows is not None else t
    z = torch.zeros_like(mean)
    return torch.where(live, mean, z), torch.where(live, rstd, z), y, t.to(BF)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def ln_bwd_stats(x, mask=None):
    """ln_stats32 of the unmasked rows, 0 for the masked ones: what the kernel AND the reference receive"""
    live = _live(mask, x.shape[0], x.device)
    mean, rstd = ln_stats32(torch.where(live[:, None], x, torch.zeros((), device=x.device)))
    z = torch.zeros_like(mean)
    return torch.where(live, mean, z), torch.where(live, rstd, z)


def ln_bwd_ref(dy, x, gamma, mean32, rstd32, mask, init):
    """float64 references and bounds of every backward output.  init: dict of the accumulated outputs' initial values (dgamma,
    dbeta, dxsum: [cols] or None).  Every rounding of a column sum is relative to a partial sum of at most |init| + sum_r |term|, and
    there are at most rows + 8 of them (the adds inside a workgroup, three through LDS, one atomic or slot add per workgroup, the
    term's own product and xhat's two roundings)."""
    rows, cols = x.shape
    live = _live(mask, rows, x.device)[:, None]
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    xd, dyd = torch.where(live, x.double(), zero), torch.where(live, dy.double(), zero)
    mu, rs = mean32.double()[:, None], rstd32.double()[:, None]
    xh = torch.where(live, (xd - mu) * rs, zero)
    g = dyd * gamma.double()[None, :]
    s1, s2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    dx = rs * (g - s1 - xh * s2)
    tol_dx = rs * (2.0 ** -20 * (g.abs() + s1.abs() + (xh * s2).abs())
                   + 2.0 ** -19 * (g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True)))
    dx, tol_dx = torch.where(live, dx, zero), torch.where(live, tol_dx, zero)
    n = (rows + 8) * SUM_ULP
    i0 = {k: (v.double() if v is not None else None) for k, v in init.items()}
    out = dict(dx=(dx, tol_dx), dx_bf16=(dx, tol_dx + BF16_STEP * dx.abs()))
    if i0.get("dbeta") is not None:
        out["dbeta"] = (i0["dbeta"] + dyd.sum(0), torch.zeros(cols, dtype=torch.float64, device=x.device))
    if i0.get("dgamma") is not None:
        t = dyd * xh
        out["dgamma"] = (i0["dgamma"] + t.sum(0), n * (t.abs().sum(0) + i0["dgamma"].abs()))
    if i0.get("dxsum") is not None:
        out["dxsum"] = (i0["dxsum"] + dx.sum(0), n * (dx.abs().sum(0) + i0["dxsum"].abs()) + tol_dx.sum(0))
    return out


def ln_bwd_emulate32(dy, x, gamma, mean32, rstd32, mask, init):
    """the backward kernels' formula in fp32 torch: dict of dx, dx_bf16, dgamma, dbeta, dxsum"""
    live = _live(mask, x.shape[0], x.device)[:, None]
    z = torch.zeros((), device=x.device)
    xz, dz = torch.where(live, x, z), torch.where(live, dy, z)
    xh = torch.where(live, (xz - mean32[:, None]) * rstd32[:, None], z)
    g = dz * gamma[None, :]
    cols = torch.tensor(float(x.shape[1]), dtype=F32, device=x.device)
    s1, s2 = g.sum(1, keepdim=True) / cols, (g * xh).sum(1, keepdim=True) / cols
    dx = torch.where(live, rstd32[:, None] * (g - s1 - xh * s2), z)
    out = dict(dx=dx, dx_bf16=dx.to(BF))
    for k, t in (("dgamma", dz * xh), ("dbeta", dz), ("dxsum", dx)):
        if init.get(k) is not None:
            out[k] = init[k] + t.sum(0)
    return out


# ------------------------------------------------------------------------------------------------ tabular value encoder
def tab_value_fwd_ref(x, w1, b1, max_value, padding_value):
    """(h1 reference, bound, padmask) : relu(min(x, max_value) w1 + b1)"""
    xc = torch.minimum(x.double(), torch.tensor(float(max_value), dtype=torch.float64, device=x.device))[:, None]
    pre = xc * w1.double()[None, :] + b1.double()[None, :]
    ref = pre.clamp_min(0)
    tol = BF16_STEP * ref.abs() + 2.0 ** -22 * ((xc * w1.double()[None, :]).abs() + b1.double().abs()[None, :])
    return ref, tol, (x == padding_value).to(torch.uint8)


def tab_value_bwd_ref(dh1, h1, x, max_value, init_w, init_b):
    """((dw1 reference, bound), (db1 reference, exact)) with the ReLU gate taken from the STORED h1"""
    rows = x.shape[0]
    gsel = torch.where(h1.float() > 0, dh1.double(), torch.zeros((), dtype=torch.float64, device=x.device))
    xc = torch.minimum(x.double(), torch.tensor(float(max_value), dtype=torch.float64, device=x.device))[:, None]
    term = gsel * xc
    tol = (rows + 8) * SUM_ULP * (term.abs().sum(0) + init_w.double().abs())
    return (init_w.double() + term.sum(0), tol), init_b.double() + gsel.sum(0)


# ------------------------------------------------------------------------------------------------ AdamW
def f32(v):
    """a Python float rounded to fp32, as a Python float: what a kernel receives for a `float` argument"""
    return float(torch.tensor(v, dtype=F32))


def adamw_ref(p, g, m, v, sq_word, lr, b1, b2, eps, wd, bc1, bc2, max_norm, use_norm=True):
    """One step in float64 per element from the fp32 state and the fp32 hyper-parameters the kernel receives; 1 - beta and
    1 - lr wd are formed in fp32 as the kernel forms them (1 - 0.999 alone differs by 6e-5 otherwise), and so is the clip
    coefficient, the third per-launch scalar.  sq_word: the kernel's own (checked) sum g^2.  -> dict of (reference, bound) for p, m, v."""
    t32 = lambda a: torch.tensor(a, dtype=F32)
    lr, b1, b2, eps, wd, bc1, bc2, max_norm = (f32(a) for a in (lr, b1, b2, eps, wd, bc1, bc2, max_norm))
    omb1, omb2 = float(t32(1.0) - t32(b1)), float(t32(1.0) - t32(b2))
    decay = float(t32(1.0) - t32(lr) * t32(wd))
    clip = 1.0          # one scalar per launch, formed in fp32 as the kernel forms it (sqrtf, + 1e-6f, a division), like 1 - beta
    if max_norm > 0 and use_norm:
        c = float(t32(max_norm) / (torch.sqrt(t32(float(sq_word))) + t32(1e-6)))
        clip = c if c < 1.0 else 1.0
    pd, gd, md, vd = p.double(), g.double() * clip, m.double(), v.double()
    m1, v1 = b1 * md + omb1 * gd, b2 * vd + omb2 * gd * gd
    upd = (lr / bc1) * (m1 / (v1.sqrt() / bc2 ** 0.5 + eps))
    p1 = pd * decay - upd
    return dict(m=(m1, 2.0 ** -22 * ((b1 * md).abs() + (omb1 * gd).abs())),
                v=(v1, 2.0 ** -22 * ((b2 * vd).abs() + (omb2 * gd * gd).abs())),
                p=(p1, 2.0 ** -22 * pd.abs() + 2.0 ** -19 * upd.abs()))


def adamw_emulate32(p, g, m, v, sq_word, lr, b1, b2, eps, wd, bc1, bc2, max_norm, use_norm=True):
    """adamw_kernel's statements in fp32 torch -> (p, m, v)"""
    t = lambda a: torch.tensor(a, dtype=F32, device=p.device)
    lr, b1, b2, eps, wd, bc1, bc2, max_norm = (t(a) for a in (lr, b1, b2, eps, wd, bc1, bc2, max_norm))
    clip = t(1.0)
    if float(max_norm) > 0 and use_norm:
        c = max_norm / (torch.sqrt(t(float(sq_word))) + t(1e-6))
        clip = c if float(c) < 1.0 else t(1.0)
    step, rbc2 = lr / bc1, t(1.0) / torch.sqrt(bc2)
    gi = g * clip
    pi = p * (t(1.0) - lr * wd)
    mi = b1 * m + (t(1.0) - b1) * gi
    vi = b2 * v + (t(1.0) - b2) * gi * gi
    pi = pi - step * (mi / (torch.sqrt(vi) * rbc2 + eps))
    return pi, mi, vi


# ================================================================================================ LayerNorm case drivers
# One driver builds a case's framed operands and outputs, one checks every output; the launch between them is the library on the
# GPU (tests/test_row_edges_gpu.py) or the fp32 restatement on the CPU (tests/test_row_edges_cpu.py: every bound is satisfiable,
# and the drivers themselves are exercised without a GPU).
def row_mask(rows, gen, on):
    """uint8 [rows]: about a third of the rows masked, the last one always (more than one row), or None"""
    if not on:
        return None
    m = torch.rand(rows, generator=gen, device=gen.device) < 0.3
    if rows > 1:
        m[rows - 1] = True
        m[0] = False
    else:
        m[0] = False
    return m.to(torch.uint8)


def vec_framed(v, byte_off=0, pad=3):
    """a 1-d tensor inside a NaN frame, its base byte_off bytes past a 16-byte boundary"""
    return framed_in(v.reshape(1, -1), v.numel() + pad, byte_off)[0]


def packed_rows(rows, period, row0, extra):
    """destination row of every kernel row in a packed placement: sample r / period of (period + extra) rows, from row0 on"""
    r = torch.arange(rows)
    return ((r // period) * (period + extra) + row0 + r % period).tolist()


def ln_fwd_setup(case, gen, extra=5):
    rows, cols, dev = case["rows"], case["cols"], gen.device
    T = dict(mask=row_mask(rows, gen, case["mask"]))
    T["x"] = ln_input(rows, cols, case["ldx"], gen, T["mask"], case["x_off"])
    T["gamma"] = vec_framed(torch.randn(cols, generator=gen, device=dev), case["gamma_off"])
    T["beta"] = vec_framed(torch.randn(cols, generator=gen, device=dev)) if case["beta"] else None
    period = case["period"]
    T["add"] = None
    if case["add"]:
        n_add = period if period else rows
        T["add"] = framed_in(torch.randn(n_add, cols, generator=gen, device=dev), cols, case["add_off"])          # the table's row stride IS cols
    T["dest"] = packed_rows(rows, period, case["y_row0"], extra) if period else list(range(rows))
    T["y_rows"] = cdiv(rows, period) * (period + extra) if period else rows
    T["y_bstride"] = (period + extra) * case["ldy"] if period else 0
    return T


def cdiv(a, b):
    return (a + b - 1) // b


def ln_fwd_outputs(case, T, stats, device):
    rows, cols = case["rows"], case["cols"]
    O = dict(y=None, ybf=None, mean=None, rstd=None)
    if case["y"]:
        O["y"] = guarded_out(T["y_rows"], cols, case["ldy"], F32, device=device)
    if case["ybf"]:
        O["ybf"] = guarded_out(rows, max(cols, case["cols_pad"]), case["ld_bf16"], BF, byte_off=case["ybf_off"], device=device)
    if stats:
        O["mean"], O["rstd"] = guarded_out(1, rows, rows + 3, F32, device=device), guarded_out(1, rows, rows + 3, F32, device=device)
    return O


def ln_fwd_args(case, T, O):
    """mca_layernorm_fwd's arguments up to the stream"""
    p = lambda t: None if t is None else t.data_ptr()
    y_ptr = None if O["y"] is None else O["y"].data_ptr() + (case["y_row0"] * case["ldy"] * 4 if case["period"] else 0)
    return (p(T["x"]), case["ldx"], p(T["gamma"]), p(T["beta"]), p(T["mask"]), p(T["add"]), case["period"], y_ptr, case["ldy"] if case["y"] else 0,
            T["y_bstride"], p(O["ybf"]), case["ld_bf16"] if case["ybf"] else 0, case["cols_pad"], p(O["mean"]), p(O["rstd"]), case["rows"], case["cols"], EPS)


def ln_fwd_emulate_into(case, T, O):
    """the CPU stand-in of the launch: the fp32 restatement stored where the kernel stores"""
    rows, cols = case["rows"], case["cols"]
    add_rows = None
    if T["add"] is not None and O["y"] is not None:
        add_rows = T["add"][torch.arange(rows) % case["period"]] if case["period"] else T["add"]
    mean, rstd, y, yb = ln_fwd_emulate32(T["x"], T["gamma"], T["beta"], add_rows, T["mask"])
    if O["mean"] is not None:
        O["mean"].t[0].copy_(mean)
        O["rstd"].t[0].copy_(rstd)
    if O["y"] is not None:
        O["y"].t[T["dest"]] = y
    if O["ybf"] is not None:
        O["ybf"].t[:, :cols] = yb
        O["ybf"].t[:, cols:case["cols_pad"]] = 0


def ln_fwd_check(case, T, O, stats_k=None, what=""):
    """every output of one forward launch, in order: a wrong statistic cannot hide in y.  stats_k: the (checked) kernel statistics
    of an earlier launch of the same call form, for a launch that was asked for none.  -> (mean, rstd) of the kernel"""
    rows, cols = case["rows"], case["cols"]
    what = what or case["name"]
    if O["mean"] is not None:
        mean, tol_m, rstd, tol_r = ln_fwd_stats_ref(T["x"], T["mask"])
        close(O["mean"].t[0], mean, tol_m, f"{what}: mean (row = 0, column = the row)", "ln_fwd mean")
        close(O["rstd"].t[0], rstd, tol_r, f"{what}: rstd (row = 0, column = the row)", "ln_fwd rstd")
        stats_k = (O["mean"].t[0].clone(), O["rstd"].t[0].clone())
    add_rows = None
    if T["add"] is not None:
        add_rows = T["add"][torch.arange(rows, device=T["add"].device) % case["period"]] if case["period"] else T["add"]
    y, tol_y, yb, tol_yb = ln_fwd_y_ref(T["x"], T["gamma"], T["beta"], add_rows, T["mask"], *stats_k)
    if O["y"] is not None:
        close(O["y"].t[T["dest"]], y, tol_y, f"{what}: y", "ln_fwd y")
        hit = set(T["dest"])
        assert_rows_untouched(O["y"].t, [r for r in range(T["y_rows"]) if r not in hit], f"{what}: y")
    if O["ybf"] is not None:
        close(O["ybf"].t[:, :cols], yb, tol_yb, f"{what}: y_bf16", "ln_fwd y_bf16")
        if case["cols_pad"] > cols:
            pad = O["ybf"].t[:, cols:]
            assert_exact(pad, torch.zeros_like(pad), f"{what}: y_bf16 columns [cols, cols_pad)")
    for k in ("mean", "rstd", "y", "ybf"):
        if O[k] is not None:
            assert_guard_intact(O[k], f"{what}: {k}")
    return stats_k


def ln_bwd_setup(case, gen, extra=5):
    rows, cols, dev, period = case["rows"], case["cols"], gen.device, case["period"]
    T = dict(mask=row_mask(rows, gen, case["mask"]))
    T["x"] = ln_input(rows, cols, case["ldx"], gen, T["mask"], case["x_off"])
    T["mean"], T["rstd"] = ln_bwd_stats(T["x"], T["mask"])
    T["gamma"] = vec_framed(torch.randn(cols, generator=gen, device=dev), case["gamma_off"])
    dy = torch.randint(-4, 5, (rows, cols), generator=gen, device=dev).float()
    nan_rows_(dy, T["mask"])
    T["src"] = packed_rows(rows, period, case["y_row0"], extra) if period else list(range(rows))
    n_dy = cdiv(rows, period) * (period + extra) if period else rows
    full = framed_in(torch.full((n_dy, cols), float("nan"), device=dev), case["ldy"])
    full[T["src"]] = dy
    T["dy_full"], T["dy"] = full, dy
    T["dy_ptr"] = full.data_ptr() + (case["y_row0"] * case["ldy"] * 4 if period else 0)
    T["y_bstride"] = (period + extra) * case["ldy"] if period else 0
    T["init"] = {k: (torch.randint(-3, 4, (cols,), generator=gen, device=dev).float() if case[k] else None) for k in ("dgamma", "dbeta", "dxsum")}
    return T


def ln_bwd_outputs(case, T, device, scratch_floats=0):
    rows, cols = case["rows"], case["cols"]
    O = dict(dx=guarded_out(rows, cols, case["lddx"], F32, device=device) if case["dx"] else None,
             dxb=guarded_out(rows, cols, case["ld_bf16"], BF, byte_off=case["dxb_off"], device=device) if case["dxb"] else None,
             scratch=guarded_out(1, scratch_floats, scratch_floats + 3, F32, device=device) if scratch_floats else None)
    for k in ("dgamma", "dbeta", "dxsum"):
        O[k] = None
        if case[k]:
            O[k] = guarded_out(1, cols, cols + 3, F32, device=device)
            O[k].t[0].copy_(T["init"][k])
    return O


def ln_bwd_args(case, T, O):
    """mca_layernorm_bwd's arguments up to the stream (the _det form appends scratch, scratch_floats)"""
    p = lambda t: None if t is None else t.data_ptr()
    return (T["dy_ptr"], case["ldy"], T["y_bstride"], case["period"], p(T["x"]), case["ldx"], p(T["gamma"]), p(T["mean"]), p(T["rstd"]), p(T["mask"]),
            p(O["dx"]), case["lddx"] if case["dx"] else 0, p(O["dxb"]), case["ld_bf16"] if case["dxb"] else 0, p(O["dgamma"]), p(O["dbeta"]), p(O["dxsum"]),
            case["rows"], case["cols"])


def ln_bwd_emulate_into(case, T, O):
    e = ln_bwd_emulate32(T["dy"], T["x"], T["gamma"], T["mean"], T["rstd"], T["mask"], T["init"])
    if O["dx"] is not None:
        O["dx"].t.copy_(e["dx"])
    if O["dxb"] is not None:
        O["dxb"].t.copy_(e["dx_bf16"])
    for k in ("dgamma", "dbeta", "dxsum"):
        if O[k] is not None:
            O[k].t[0].copy_(e[k])


def ln_bwd_check(case, T, O, what=""):
    what = what or case["name"]
    ref = ln_bwd_ref(T["dy"], T["x"], T["gamma"], T["mean"], T["rstd"], T["mask"], T["init"])
    if O["dbeta"] is not None:
        assert_exact_rows(O["dbeta"].t[0], ref["dbeta"][0].float(), f"{what}: dbeta (row = 0)")
    if O["dx"] is not None:
        close(O["dx"].t, *ref["dx"], f"{what}: dx", "ln_bwd dx")
    if O["dxb"] is not None:
        close(O["dxb"].t, *ref["dx_bf16"], f"{what}: dx_bf16", "ln_bwd dx_bf16")
    for k in ("dgamma", "dxsum"):
        if O[k] is not None:
            close(O[k].t[0], *ref[k], f"{what}: {k} (row = 0)", f"ln_bwd {k}")
    for k in ("dx", "dxb", "dgamma", "dbeta", "dxsum", "scratch"):
        if O[k] is not None:
            assert_guard_intact(O[k], f"{what}: {k}")
