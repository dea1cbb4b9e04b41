"""Helpers of the evaluation-kernel edge tests (tests/test_eval_edges_gpu.py; checked themselves by tests/test_eval_edges_cpu.py): the
operands of a case inside frames, float64 / integer references of csrc/evaluate.hip's entry points as their header comments state
them, the bounds derived in docs/parity.md ("Evaluation kernels: every element, at the edges"), and fp32 restatements of the
kernels whose results are not exact.  Plain functions on any device.

Integer-valued operands make every tile_core product and sum exact in any order (|sum| < 2^24), so most outputs are compared
with assert_exact; what is left (a normalisation, expf / log1pf, one product by a scale that is no power of two) has a bound."""
import math

import numpy as np
import torch

import eval_cases as EC
from gemm_edge_util import _framed, assert_exact, assert_guard_intact, guarded_out          # noqa: F401
from row_edge_util import WORST, close, framed_in          # noqa: F401

F32, F64, I32 = torch.float32, torch.float64, torch.int32
U = 2.0 ** -24
EXPF_ULP = LOG1PF_ULP = 2          # twice the 1 ulp the HIP math documentation lists; 1 ulp <= 2 U relative
TINY = 2.0 ** -126
PAD = EC.PAD
SEED, STEP = 0x1234567, 7


def _mask_ref(seed, step, rows, units, p):
    """the kernel's dropout mask (csrc/evaluate.hip dropout_keep), restated: keep where a hash of (seed, step, row, unit) >= p"""
    u64 = np.uint64

    def fmix(k):
        k = k ^ (k >> u64(33)); k = k * u64(0xff51afd7ed558ccd); k = k ^ (k >> u64(33))
        k = k * u64(0xc4ceb9fe1a85ec53); return k ^ (k >> u64(33))
    with np.errstate(over="ignore"):
        r = np.arange(rows, dtype=np.uint64)[:, None]
        u = np.arange(units, dtype=np.uint64)[None, :]
        h = fmix(u64(seed) ^ fmix(u64(step) ^ fmix((r << u64(32)) | u)))
    return torch.from_numpy((h >> u64(40)).astype(np.float32) * np.float32(2.0 ** -24) >= np.float32(p))


# ------------------------------------------------------------------------------------------------ operands
def gen(seed, dev):
    return torch.Generator(device=dev).manual_seed(seed)


def ints(shape, g, amp):
    return torch.randint(-amp, amp + 1, shape, generator=g, device=g.device).float()


def int_mat(rows, cols, g, amp=2):
    """[rows, cols] fp32 integers in {-amp .. amp} inside a NaN frame with row stride cols + PAD"""
    return framed_in(ints((rows, cols), g, amp), cols + PAD)


def framed_i32(t):
    """a 1-d int32 tensor inside a frame of 0xFF bytes: a stray index is -1"""
    _, _, view = _framed(1, t.numel(), t.numel() + PAD, I32, t.device, 0xFF, 0)
    view.copy_(t.reshape(1, -1).to(I32))
    return view[0]


def gather_index(n, rows):
    """n indices into `rows` rows, out of order (descending from the last row, wrapping) and, for n > 2, with a repeat"""
    idx = (rows - 1 - torch.arange(n)) % rows
    if n > 2:
        idx[n - 1] = idx[0]
    return idx


def out(rows, cols, dev, dtype=F32, ld=None):
    return guarded_out(rows, cols, cols + PAD if ld is None else ld, dtype, device=dev)


def untouched(g, what):
    it = {8: torch.int64, 4: I32, 2: torch.int16}[g.es]
    assert (g.t.contiguous().view(it) == -1).all(), f"{what}: stored to by a refused or empty call"
    assert_guard_intact(g, what)


def _tree64(part):
    """[..., 64] lane partials -> wave_sum's xor butterfly"""
    lane = torch.arange(64, device=part.device)
    v = part
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]


def _lanes(x, width=64):
    """[rows, d] -> [rows, trips, width]: element k goes to lane k % width, trip k // width (zero padded)"""
    rows, d = x.shape
    trips = EC.cdiv(d, width)
    p = torch.zeros(rows, trips * width, dtype=x.dtype, device=x.device)
    p[:, :d] = x
    return p.reshape(rows, trips, width)


# ------------------------------------------------------------------------------------------------ mca_rows_normalize_f32
def normalize_setup(c, dev):
    n, d = c["n"], c["d"]
    x = torch.randn(n, d, generator=gen(41, dev), device=dev)
    if n >= 3:
        x[1] = 0.0                      # a zero row: 0 / 1e-8 = 0
    if n >= 4:
        x[2] = 0.0
        x[2, d - 1] = 1e-9              # a row of norm 1e-9: divided by 1e-8
    return dict(x=framed_in(x, d + PAD)), dict(y=out(n, d, dev))


def normalize_ref(c, T):
    """y = x / max(||x||, 1e-8f).  Bound: the squares' sum meets cdiv(d, 64) fmaf steps and 6 tree levels (+ 1: a product rounded on its own),
    all addends positive, and enters under a square root (half its relative error); sqrtf 1 ulp, the division one rounding"""
    xd = T["x"].double()
    nrm = xd.norm(dim=1, keepdim=True).clamp_min(float(np.float32(1e-8)))
    ref = xd / nrm
    return ref, ((EC.cdiv(c["d"], 64) + 7) / 2 + 3) * U * ref.abs()


def normalize_emulate(c, T, O):
    x = T["x"]
    part = _lanes(x * x)
    s = torch.zeros(x.shape[0], 64, device=x.device)
    for k in range(part.shape[1]):
        s = s + part[:, k]
    nrm = torch.sqrt(_tree64(s)).clamp_min(torch.tensor(1e-8, dtype=F32, device=x.device))
    O["y"].t.copy_(x / nrm[:, None])


def normalize_check(c, T, O):
    ref, tol = normalize_ref(c, T)
    close(O["y"].t, ref, tol, c["name"], "eval normalize")
    if c["n"] >= 3:
        assert (O["y"].t[1] == 0).all(), "a zero row gives zeros"
    if c["n"] >= 4:
        assert abs(float(O["y"].t[2, c["d"] - 1]) - 0.1) < 1e-7, "a row of norm 1e-9 is divided by 1e-8"
    assert_guard_intact(O["y"], c["name"])


# ------------------------------------------------------------------------------------------------ mca_cosine_rank_f32
def rank_setup(c, dev):
    nq, nt, d = c["nq"], c["nt"], c["d"]
    g = gen(42, dev)
    t = ints((nt, d), g, 2)
    q_rows = nt if c["gather"] else nq          # with a gather, query row i is paired with target i
    q = ints((q_rows, d), g, 2)
    if nt >= 3:
        t[nt - 1] = t[0]                # a duplicate of target 0: a tie for the query whose target it is, never counted
        q[min(1, q_rows - 1)] = t[min(1, q_rows - 1)]          # a query equal to its own target
    idx = gather_index(nq, nt).to(dev) if c["gather"] else None
    T = dict(q=framed_in(q, d + PAD), t=framed_in(t, d + PAD), qidx=framed_i32(idx) if idx is not None else None)
    return T, dict(s_true=out(1, nq, dev), rank=out(1, nq, dev, I32))


def rank_ref(c, T):
    """(s_true, rank) as int64: the integer scores are exact, the rank is the count of STRICTLY greater scores"""
    q, t = T["q"].to(torch.int64), T["t"].to(torch.int64)
    idx = T["qidx"].long() if T["qidx"] is not None else torch.arange(c["nq"], device=q.device)
    S = (q[idx].double() @ t.double().t()).to(torch.int64)
    st = (q[idx] * t[idx]).sum(1)
    return st, (S > st[:, None]).sum(1)


def rank_emulate(c, T, O):
    st, rk = rank_ref(c, T)
    O["s_true"].t[0].copy_(st.float())
    O["rank"].t[0].copy_(rk.to(I32))


def rank_check(c, T, O):
    st, rk = rank_ref(c, T)
    assert int(st.abs().max()) < 2 ** 24
    assert_exact(O["s_true"].t, st.float().reshape(1, -1), f"{c['name']}: s_true (row = 0, column = the query)")
    assert_exact(O["rank"].t, rk.to(I32).reshape(1, -1), f"{c['name']}: rank (row = 0, column = the query)")
    assert_guard_intact(O["s_true"], c["name"]), assert_guard_intact(O["rank"], c["name"])


# ------------------------------------------------------------------------------------------------ mca_pair_gauss_sum_f32
PAIR_T = 0.125          # a power of two: -t * d2 is exact


def pair_tiles(n):
    return EC.cdiv(n, EC.TILE) if n > 0 else 1


def pair_setup(c, dev, short=0):
    n, d = c["n"], c["d"]
    x = int_mat(max(n, 1), d, gen(43, dev)) if n > 0 else None
    np_ = pair_tiles(n) ** 2 - short
    O = dict(partials=out(1, np_, dev, F64) if np_ > 0 else None, sum=out(1, 1, dev, F64), value=out(1, 1, dev))
    return dict(x=x), O


def pair_ref(c, T, dev="cpu"):
    """(per-tile sums [tiles, tiles], their bounds, total, bound): sum over i < j of exp(-t d2_ij), d2 exact; only expf rounds before the
    fp64 sums (whose own roundings, 2^-53 each, are covered by 1e-13 relative)"""
    n, tiles = c["n"], pair_tiles(c["n"])
    dev = T["x"].device if T["x"] is not None else dev
    if n <= 1:
        z = torch.zeros(tiles, tiles, dtype=F64, device=dev)
        return z, z, z.sum(), z.sum()
    x = T["x"][:n].double()
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(2)
    e = torch.exp(-PAIR_T * d2) * torch.triu(torch.ones(n, n, dtype=F64, device=dev), 1)
    pad = torch.zeros(tiles * EC.TILE, tiles * EC.TILE, dtype=F64, device=dev)
    pad[:n, :n] = e
    per = pad.reshape(tiles, EC.TILE, tiles, EC.TILE).sum((1, 3))
    rel = 2 * EXPF_ULP * U + 1e-13
    return per, rel * per, per.sum(), rel * per.sum()


def pair_emulate(c, T, O):
    n, tiles = c["n"], pair_tiles(c["n"])
    if n > 1:
        x = T["x"][:n]
        d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(2)          # integers: exact in fp32
        e = torch.exp(-PAIR_T * d2).double() * torch.triu(torch.ones(n, n, dtype=F64, device=x.device), 1)
        pad = torch.zeros(tiles * EC.TILE, tiles * EC.TILE, dtype=F64, device=x.device)
        pad[:n, :n] = e
        per = pad.reshape(tiles, EC.TILE, tiles, EC.TILE).sum((1, 3))
        O["partials"].t[0].copy_(per.reshape(-1))
        tot = per.sum()
    else:
        tot = torch.zeros((), dtype=F64, device=O["sum"].t.device)
    O["sum"].t[0, 0] = tot
    pairs = 0.5 * n * (n - 1)
    O["value"].t[0, 0] = float(torch.log(tot / pairs)) if pairs > 0 else float("nan")


def pair_check(c, T, O):
    n, tiles, name = c["n"], pair_tiles(c["n"]), c["name"]
    per, per_tol, tot, tot_tol = pair_ref(c, T, O["sum"].t.device)
    if n > 1:
        got = O["partials"].t[0].reshape(tiles, tiles)
        low = torch.tril(torch.ones(tiles, tiles, dtype=torch.bool, device=got.device), -1)
        assert (got[low] == 0).all(), f"{name}: a partial below the diagonal is not exactly 0"
        close(got, per, per_tol, f"{name}: partials (row, column = tile)", "eval pair partials")
    else:
        untouched(O["partials"], f"{name}: partials")
    close(O["sum"].t, tot.reshape(1, 1), tot_tol.reshape(1, 1), f"{name}: sum_out", "eval pair sum")
    if n <= 1:
        assert float(O["sum"].t[0, 0]) == 0.0 and math.isnan(float(O["value"].t[0, 0])), f"{name}: value_out is NaN for n <= 1"
    else:
        v = torch.log(tot / (0.5 * n * (n - 1)))
        close(O["value"].t, v.reshape(1, 1), (tot_tol / tot + U * v.abs() + 1e-13).reshape(1, 1), f"{name}: value_out", "eval pair value")
    for k in ("partials", "sum", "value"):
        assert_guard_intact(O[k], f"{name}: {k}")


# ------------------------------------------------------------------------------------------------ mca_probe_nt_f32
BIAS_UP = 500.0          # with dropout the bias lifts every pre-activation above 0 (|x . w| <= 4 * 96), so y > 0 exactly where the mask keeps


def nt_setup(c, dev):
    M, N, K = c["M"], c["N"], c["K"]
    g = gen(44, dev)
    x_rows = M + 5 if c["gather"] else M
    T = dict(x=int_mat(x_rows, K, g), w=int_mat(N, K, g), bias=None, xidx=None)
    if c["bias"]:
        b = ints((N,), g, 3) + (BIAS_UP if c["act"] == 2 else 0.0)
        T["bias"] = framed_in(b.reshape(1, -1), N + PAD)[0]
    if c["gather"]:
        T["xidx"] = framed_i32(gather_index(M, x_rows).to(dev))
    return T, dict(y=out(M, N, dev))


def nt_ref(c, T):
    """(reference, bound, keep mask or None).  Exact but for p = 0.25: z * fl(1 / 0.75f) is one rounding of the float64 product"""
    M, N = c["M"], c["N"]
    x = T["x"][T["xidx"].long()] if T["xidx"] is not None else T["x"]
    z = x.double() @ T["w"].double().t() + (T["bias"].double()[None, :] if T["bias"] is not None else 0.0)
    tol = torch.zeros_like(z)
    keep = None
    if c["act"] == 2:
        p = np.float32(c["p"])
        scale = float(np.float32(1) / (np.float32(1) - p)) if p < 1 else 0.0
        keep = _mask_ref(SEED, STEP, M, N, float(p)).to(z.device)
        z = torch.where(keep, z * scale, torch.zeros_like(z))
        if scale > 0 and math.log2(scale) != int(math.log2(scale)):          # no power of two: the product rounds
            tol = U * z.abs()
    if c["act"] >= 1:
        z = z.clamp_min(0)
    return z, tol, keep


def nt_emulate(c, T, O):
    x = T["x"][T["xidx"].long()] if T["xidx"] is not None else T["x"]
    z = x @ T["w"].t()
    if T["bias"] is not None:
        z = z + T["bias"][None, :]
    if c["act"] == 2:
        p = torch.tensor(c["p"], dtype=F32)
        scale = (1.0 / (1.0 - p)).to(z.device) if c["p"] < 1 else torch.zeros((), device=z.device)
        keep = _mask_ref(SEED, STEP, c["M"], c["N"], c["p"]).to(z.device)
        z = torch.where(keep, z * scale, torch.zeros_like(z))
    if c["act"] >= 1:
        z = z.clamp_min(0)
    O["y"].t.copy_(z)


def nt_check(c, T, O):
    ref, tol, keep = nt_ref(c, T)
    y = O["y"].t
    if keep is not None:          # the mask, at every (row, unit): the lifted pre-activations are positive
        want = keep if c["p"] < 1 else torch.zeros_like(keep)
        assert_exact((y > 0), want, f"{c['name']}: kept units (the dropout mask)")
    if bool((tol > 0).any()):
        close(y, ref, tol, c["name"], "eval probe_nt p=0.25")
    else:
        assert_exact(y, ref.float(), c["name"])
    assert_guard_intact(O["y"], c["name"])


# ------------------------------------------------------------------------------------------------ mca_probe_head_f32
DACT = 2.0
PLANT_Z = [0.0, 50.0, -50.0, 100.0, -100.0, 3.0, -2.0]


def head_setup(c, dev):
    K, L, B = c["K"], c["L"], c["B"]
    g = gen(45, dev)
    a_rows, y_rows = (B + 3 if c["aidx"] else B), (B + 2 if c["yidx"] else B)
    a = ints((a_rows, K), g, 2)
    w = ints((L, K), g, 1)
    aidx = gather_index(B, a_rows) if c["aidx"] else torch.arange(B)
    yidx = gather_index(B, y_rows) if c["yidx"] else torch.arange(B)
    a[aidx[0]] = 0.0          # batch row 0: a == 0, so z = bias and da is exactly 0
    if c["loss"] == EC.BCE:
        bias = torch.tensor([PLANT_Z[l % len(PLANT_Z)] for l in range(L)], device=dev)
        labels = torch.randint(0, 2, (y_rows, L), generator=g, device=dev).float()
    else:
        bias = ints((L,), g, 3)
        labels = ints((y_rows, L), g, 4)
        z = a[aidx.to(dev)] @ w.t() + bias[None, :]
        labels[yidx[B - 1]] = z[B - 1]          # the last batch row: e == 0 at every label
    T = dict(a=framed_in(a, K + PAD), w=framed_in(w, K), bias=framed_in(bias.reshape(1, -1), L + PAD)[0], labels=framed_in(labels, L),
             aidx=framed_i32(aidx.to(dev)) if c["aidx"] else None, yidx=framed_i32(yidx.to(dev)) if c["yidx"] else None)
    blocks = EC.cdiv(B, 4)
    O = dict(pred=out(B, L, dev, ld=L), dz=out(B, L, dev, ld=L) if c["dz"] else None, da=out(B, K, dev, ld=K) if c["da"] else None,
             loss_part=out(1, blocks, dev))
    return T, O


def head_ref(c, T):
    """dict of (reference, bound or None = exact) for pred, dz, da, loss_part.  z, |e|, e^2 are exact integers; inv_count = fl(1 / (B L))
    and the L1 / MSE gradients are single correctly rounded fp32 products, restated in numpy float32.  BCE: expf and log1pf (2 ulp each)."""
    K, L, B = c["K"], c["L"], c["B"]
    dev = T["a"].device
    a = T["a"][T["aidx"].long()] if T["aidx"] is not None else T["a"]
    y = T["labels"][T["yidx"].long()] if T["yidx"] is not None else T["labels"]
    w = T["w"].double()
    z = a.double() @ w.t() + T["bias"].double()[None, :]
    e = z - y.double()
    inv = np.float32(1) / np.float32(B * L)
    ref = dict(pred=(z, None))
    zero = torch.zeros_like(z)
    if c["loss"] == EC.L1:
        le, le_tol = e.abs(), None
        g, g_tol = torch.sign(e) * float(inv), None
    elif c["loss"] == EC.MSE:
        le, le_tol = e * e, None
        g = torch.from_numpy((np.float32(2) * e.cpu().numpy().astype(np.float32)) * inv).double().to(dev)
        g_tol = None
    else:
        sp = torch.log1p(torch.exp(-z.abs()))
        lin = z.clamp_min(0) - z * y.double()
        le = lin + sp
        le_tol = 2 * (EXPF_ULP + LOG1PF_ULP) * U * sp + 3 * U * (lin.abs() + sp) + TINY
        s = torch.sigmoid(z)
        g = (s - y.double()) * float(inv)
        g_tol = float(inv) * (2 * EXPF_ULP * U * s * (1 - s) + 3 * U * s + U * (s - y.double()).abs() + TINY) + U * g.abs()
    ref["dz"] = (g, g_tol)
    gt = g_tol if g_tol is not None else zero
    da = (g @ w) * DACT
    da_tol = DACT * (gt @ w.abs() + (L + 2) * U * (g.abs() @ w.abs()))
    live = a > 0
    ref["da"] = (torch.where(live, da, torch.zeros_like(da)), torch.where(live, da_tol, torch.zeros_like(da_tol)))
    blocks = EC.cdiv(B, 4)
    pad = torch.zeros(blocks * 4, L, dtype=F64, device=dev)
    pad[:B] = le
    part = pad.reshape(blocks, 4 * L).sum(1)
    if le_tol is None:
        ref["loss_part"] = (part, None)
    else:
        padt = torch.zeros(blocks * 4, L, dtype=F64, device=dev)
        padt[:B] = le_tol
        ref["loss_part"] = (part, padt.reshape(blocks, 4 * L).sum(1) + 8 * U * part.abs())          # 6 tree levels and two adds
    return ref


def head_emulate(c, T, O, gate=lambda a: a > 0):
    K, L, B = c["K"], c["L"], c["B"]
    a = T["a"][T["aidx"].long()] if T["aidx"] is not None else T["a"]
    y = T["labels"][T["yidx"].long()] if T["yidx"] is not None else T["labels"]
    w, dev = T["w"], a.device
    z = a @ w.t() + T["bias"][None, :]          # integers: exact
    e = z - y
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(B * L), dtype=F32)
    inv = inv.to(dev)
    if c["loss"] == EC.L1:
        le, g = e.abs(), torch.sign(e)
    elif c["loss"] == EC.MSE:
        le, g = e * e, 2.0 * e
    else:
        le = z.clamp_min(0) - z * y + torch.log1p(torch.exp(-z.abs()))
        g = 1.0 / (1.0 + torch.exp(-z)) - y
    g = g * inv
    O["pred"].t.copy_(z)
    if O["dz"] is not None:
        O["dz"].t.copy_(g)
    if O["da"] is not None:
        s = torch.zeros(B, K, device=dev)
        for l in range(L):
            s = s + g[:, l, None] * w[l][None, :]
        O["da"].t.copy_(torch.where(gate(a), s * DACT, torch.zeros_like(s)))
    blocks = EC.cdiv(B, 4)
    lanes = torch.zeros(blocks * 4, 64, device=dev)
    lanes[:B, :L] = le
    r = _tree64(lanes).reshape(blocks, 4)
    O["loss_part"].t[0].copy_((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3]))


def head_check(c, T, O):
    ref, name = head_ref(c, T), c["name"]
    for k, key in (("pred", None), ("dz", "eval head dz (BCE)"), ("da", "eval head da"), ("loss_part", "eval head loss_part (BCE)")):
        if O[k] is None:
            continue
        want, tol = ref[k]
        got = O[k].t if k != "loss_part" else O[k].t[0]
        assert torch.isfinite(got).all(), f"{name}: {k} is not finite"
        if tol is None:
            assert_exact(got.reshape(want.shape[0], -1), want.float().reshape(want.shape[0], -1), f"{name}: {k}")
        else:
            close(got, want, tol, f"{name}: {k}", key)
        assert_guard_intact(O[k], f"{name}: {k}")
    if O["da"] is not None:
        a = T["a"][T["aidx"].long()] if T["aidx"] is not None else T["a"]
        assert (O["da"].t[a <= 0] == 0).all(), f"{name}: da is exactly 0 where a <= 0"


# ------------------------------------------------------------------------------------------------ mca_probe_tn_f32
def tn_setup(c, dev, short=0):
    R, N, K = c["R"], c["N"], c["K"]
    g = gen(46, dev)
    b_rows = R + 4 if c["gather"] else R
    T = dict(a=int_mat(R, N, g), b=int_mat(b_rows, K, g), bidx=framed_i32(gather_index(R, b_rows).to(dev)) if c["gather"] else None)
    need = EC.cdiv(R, EC.PROBE_ROWS_PER_CHUNK) * N * (K + 1)
    return T, dict(partials=out(1, need - short, dev), gw=out(N, K, dev, ld=K), gb=out(1, N, dev), need=need)


def tn_ref(c, T):
    b = T["b"][T["bidx"].long()] if T["bidx"] is not None else T["b"]
    a = T["a"].double()
    return a.t() @ b.double(), a.sum(0)


def tn_emulate(c, T, O, ones=1.0):
    gw, gb = tn_ref(c, T)
    O["gw"].t.copy_(gw.float())
    O["gb"].t[0].copy_((gb * ones).float())
    O["partials"].t.fill_(0.0)


def tn_check(c, T, O):
    gw, gb = tn_ref(c, T)
    name = c["name"]
    assert_exact(O["gw"].t, gw.float(), f"{name}: gw")
    assert_exact(O["gb"].t, gb.float().reshape(1, -1), f"{name}: gb (row = 0, column = the output unit)")
    assert (O["partials"].t.view(I32) != -1).all(), f"{name}: every word of a workspace of exactly the reported size is written"
    for k in ("partials", "gw", "gb"):
        assert_guard_intact(O[k], f"{name}: {k}")
