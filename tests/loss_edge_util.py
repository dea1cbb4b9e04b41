"""Helpers of the contrastive-loss edge tests (tests/test_loss_edges_gpu.py; checked themselves by tests/test_loss_edges_cpu.py):
the data of a case, the float64 restatement of csrc/loss.hip's header formulas, the element-wise bounds derived in docs/parity.md
("Contrastive loss: every element, at the edges"), the checker of one launch's outputs, and an fp32 restatement of the five kernels
in their own summation grouping that shows every bound satisfiable without a GPU.  Everything here runs on the CPU: the GPU test
copies the kernels' outputs back."""
import importlib
import math

import numpy as np
import torch

import loss_cases as LC
from row_edge_util import WORST          # noqa: F401  (one table of worst ratios for every edge test of a process)

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24                 # fp32 unit roundoff: one rounding, relative to the value it rounds
EXPF_ULP = 2                   # expf / logf: twice the 1 ulp the HIP math documentation lists for either; 1 ulp <= 2 U relative
LOGF_ULP = 2
TINY = 2.0 ** -126             # an expf result below the smallest normal number may be flushed: an absolute error of at most this
QNAN = 0x7FC00000              # the NaN reduce_terms_kernel stores for a term with no valid row
SHOW = 6
S_OF = {"exact": 0.0, "prod3": math.log(1 / 0.07), "prod4": math.log(100.0)}
TARGET = {"prod3": 1e3, "prod4": 1e4}


# ------------------------------------------------------------------------------------------------ cases -> data
def schedule_terms(variant):
    """(terms, R) of structure.loss_terms for a small configuration, as tests/test_kernels_gpu.py::test_contrastive_loss builds them"""
    from util_small import small_config
    S = importlib.import_module("mca-paper_amd.structure")
    cfg = small_config(variant)
    st = S.FusionStructure([70, 45, 30], 8, (3, 2), fcl=cfg["fcl"], zorro=cfg["zorro"])
    terms = S.loss_terms(list(cfg["encoder_configs"].keys()), st, cfg["bimodal_contrastive"], cfg["non_fusion_fcl"])
    return [(t.slot_a, t.slot_b, t.and_bits, t.or_bits) for t in terms], st.n_return, [t.name for t in terms]


def term_valid(terms, present):
    """[T, B] bool: ((present & and_bits) == and_bits) and (or_bits == 0 or (present & or_bits) != 0)"""
    a = torch.tensor([t[2] for t in terms], dtype=torch.int64)[:, None]
    o = torch.tensor([t[3] for t in terms], dtype=torch.int64)[:, None]
    p = present.to(torch.int64)[None, :]
    return ((p & a) == a) & ((o == 0) | ((p & o) != 0))


def make_data(case, seed=0):
    """dict(pooled [B, R, D] fp32, present [B] int32, terms, s fp32 scalar tensor, B, R, D, T, b_local, W, exact)"""
    terms, R = case["terms"], case["R"]
    if isinstance(terms, str):
        terms, R, _ = schedule_terms(terms.split(":")[1])
    B, D, b = case["B"], case["D"], case["b_local"]
    g = torch.Generator().manual_seed(1000 + seed)
    present = torch.tensor([case["present"].get(i, LC.present_word(i)) for i in range(B)], dtype=torch.int32)
    s = torch.tensor(S_OF[case["kind"]], dtype=F32)
    if case["kind"] == "exact":
        pooled = torch.randint(-3, 4, (B, R, D), generator=g).float()
        pooled[0] = 3.0
        pooled[B - 1] = 3.0
    else:
        pooled = torch.randn(B, R, D, generator=g)
        P = pooled.double()
        gmax = max(float((P[:, sa] @ P[:, sb].t()).abs().max()) for sa, sb, _, _ in terms)
        pooled = (P * math.sqrt(TARGET[case["kind"]] / (math.exp(float(s)) * gmax))).float()
    return dict(pooled=pooled, present=present, terms=terms, s=s, B=B, R=R, D=D, T=len(terms), b_local=b, W=B // b, exact=case["kind"] == "exact",
                name=case["name"])


# ------------------------------------------------------------------------------------------------ float64 reference and bounds
def reference(d):
    """Every quantity of csrc/loss.hip's header comments in float64 from the fp32 inputs, each with its bound (docs/parity.md):
    rank-independent w, stats, dG, and per rank term_loss, loss, d_logit_scale, d_pooled."""
    B, R, D, T, b, W, terms = d["B"], d["R"], d["D"], d["T"], d["b_local"], d["W"], d["terms"]
    P = d["pooled"].double()
    s = float(d["s"])
    Tm = math.exp(s)
    A = torch.stack([P[:, t[0]] for t in terms])          # [T, B, D]
    Bm = torch.stack([P[:, t[1]] for t in terms])
    G = A @ Bm.transpose(1, 2)                            # G_t[i][j] = sum_d A_t[i][d] B_t[j][d]
    l = Tm * G
    if d["exact"]:
        # integers of at most 9 D < 2^24: exact in fp32 in any order; expf(0) = 1 and 1 * G are exact
        assert s == 0.0 and float(G.abs().max()) < 2 ** 24 and torch.equal(G, G.round())
        dl = torch.zeros_like(l)
    else:
        # one chain of D products and D adds: an addend meets at most D + 1 roundings (+ 1 for the second order); then T = expf(s)
        # (EXPF_ULP ulps) and the product T * G (one rounding)
        dl = Tm * (D + 2) * U * (A.abs() @ Bm.abs().transpose(1, 2)) + l.abs() * (1 + 2 * EXPF_ULP) * U
    NR = LC.cdiv(B, LC.ROWSTATS_BLOCK) + 6 + 4          # roundings an addend of a block sum meets: its thread's adds, 6 shuffle levels, 4 waves
    eye = torch.eye(B, dtype=F64)[None]
    out = dict(dl=dl, l=l)
    side = {}
    for name, L, DL in (("row", l, dl), ("col", l.transpose(1, 2), dl.transpose(1, 2))):          # L[t][i][j]: entry j of row / column i
        m = L.max(2).values
        lse = torch.logsumexp(L, 2)
        Pm = torch.exp(L - lse[:, :, None])
        # lse is 1-Lipschitz in the largest logit error; the subtraction l - m, expf, the block sum, logf of a value in [1, B], the add
        dlse = DL.max(2).values + U * (Pm * (L - m[:, :, None]).abs()).sum(2) + (2 * EXPF_ULP + NR) * U + B * TINY \
            + 2 * LOGF_ULP * U * math.log(B) + U * lse.abs()
        E = (Pm * L).sum(2)
        e = torch.expm1(DL + U * (L - m[:, :, None]).abs() + 2 * EXPF_ULP * U)          # relative error of p_j up to a common factor
        den = 1 - (Pm * e).sum(2)
        assert (den > 0.5).all()
        dE = ((Pm * e * (L - E[:, :, None]).abs()).sum(2) + (Pm * (1 + e) * DL).sum(2) + (2 * NR + 2) * U * (Pm * (1 + e) * L.abs()).sum(2)
              + B * TINY * L.abs().max(2).values) / den
        side[name] = dict(m=m, lse=lse, P=Pm, dlse=dlse, E=E, dE=dE)
    r_, c_ = side["row"], side["col"]
    diag, ddiag = torch.diagonal(l, dim1=1, dim2=2), torch.diagonal(dl, dim1=1, dim2=2)
    ce = (r_["lse"] - diag) + (c_["lse"] - diag)
    dce = r_["dlse"] + c_["dlse"] + 2 * ddiag + U * ((r_["lse"] - diag).abs() + (c_["lse"] - diag).abs() + ce.abs())
    dsum = (r_["E"] - diag) + (c_["E"] - diag)
    ddsum = r_["dE"] + c_["dE"] + 2 * ddiag + U * ((r_["E"] - diag).abs() + (c_["E"] - diag).abs() + dsum.abs())
    out["stats"] = torch.stack([r_["lse"], c_["lse"], ce, dsum], 2)
    out["stats_tol"] = torch.stack([r_["dlse"], c_["dlse"], dce, ddsum], 2)
    assert torch.isfinite(out["stats"]).all() and torch.isfinite(out["stats_tol"]).all(), "the float64 reference stays finite"
    # ---- reduce_terms
    valid = term_valid(terms, d["present"])
    n = valid.reshape(T, W, b).sum(2)                     # [T, W]
    nl = (n > 0).sum(0)                                   # [W]
    n32, nl32 = n.numpy().astype(np.float32), np.maximum(nl.numpy(), 1).astype(np.float32)
    with np.errstate(divide="ignore"):
        w32 = np.where(n32 > 0, np.float32(1) / (np.float32(2) * n32 * nl32[None, :]), np.float32(0)).astype(np.float32)
    out["w32"] = torch.from_numpy(w32)
    w = torch.where(n > 0, 1.0 / (2.0 * n.double() * nl.clamp_min(1).double()[None, :]), torch.zeros((), dtype=F64))
    out.update(valid=valid, n=n, nl=nl)
    z = torch.zeros((), dtype=F64)
    ranks = []
    for r in range(W):
        rows = slice(r * b, (r + 1) * b)
        v = valid[:, rows]
        cnt = n[:, r].double()
        live = cnt > 0
        two_n = (2 * cnt).clamp_min(1)

        def mean_terms(x, dx):
            """(per-term value, bound, total over the live terms / nl, bound): b - 1 adds and a division per term, then T adds and a division"""
            xs, axs, dxs = torch.where(v, x[:, rows], z).sum(1), torch.where(v, x[:, rows].abs(), z).sum(1), torch.where(v, dx[:, rows], z).sum(1)
            per, dper = xs / two_n, (dxs + (b + 1) * U * axs) / two_n
            k = max(int(nl[r]), 1)
            tot = torch.where(live, per, z).sum() / k
            dtot = (torch.where(live, dper, z).sum() + (T + 2) * U * torch.where(live, per.abs(), z).sum()) / k
            return per, dper, tot, dtot

        tl, dtl, loss, dloss = mean_terms(ce, dce)
        _, _, dls, ddls = mean_terms(dsum, ddsum)
        ranks.append(dict(term_loss=tl, term_tol=dtl, live=live, loss=loss, loss_tol=dloss, dls=dls, dls_tol=ddls))
    # ---- dgram: dG_t[i][j] = T (w_i (softmax_row_i[j] - [i == j]) + w_j (softmax_col_j[i] - [i == j])), w of an invalid row 0
    wrow = torch.where(valid, w[:, torch.arange(B) // b], z)          # [T, B]
    Pr, Pc = r_["P"], c_["P"].transpose(1, 2)                         # Pc[t][i][j] = exp(l[i][j] - lse_col[j])
    K = 5 + 2 * EXPF_ULP          # the subtraction, w's own rounding, the product by w, the add, the product by T, T = expf(s)
    er = torch.expm1(dl + r_["dlse"][:, :, None] + U * (l - r_["lse"][:, :, None]).abs() + 2 * EXPF_ULP * U)
    ec = torch.expm1(dl + c_["dlse"][:, None, :] + U * (l - c_["lse"][:, None, :]).abs() + 2 * EXPF_ULP * U)
    out["dG"] = Tm * (wrow[:, :, None] * (Pr - eye) + wrow[:, None, :] * (Pc - eye))
    out["dG_tol"] = Tm * (wrow[:, :, None] * (Pr * er + K * U * (Pr - eye).abs() + TINY) + wrow[:, None, :] * (Pc * ec + K * U * (Pc - eye).abs() + TINY))
    # ---- dpooled, per rank
    for r in range(W):
        ranks[r]["d_pooled"], ranks[r]["d_pooled_tol"] = dpooled64(d, out["dG"], out["dG_tol"], r)
    out["ranks"] = ranks
    out["used"] = sorted({t[0] for t in terms} | {t[1] for t in terms})
    return out


def dpooled64(d, dG, dG_tol, r):
    """d_pooled[il][slot] = sum over terms with slot_a == slot of sum_j dG[i][j] b_j + over terms with slot_b == slot of sum_i' dG[i'][i] a_i'
    for the rows of rank r, in float64 from a given dG, with |error| <= sum dG_tol |pooled| + U N sum |dG| |pooled|, N the number of addends
    (an addend meets its product's rounding, its slice's adds and the three adds of the four slices: at most N of them, docs/parity.md)
    + N TINY (a product below the smallest normal number keeps no relative precision).  dG_tol None: dG is taken as given."""
    B, R, D, b, terms = d["B"], d["R"], d["D"], d["b_local"], d["terms"]
    P = d["pooled"].double()
    rows = slice(r * b, (r + 1) * b)
    ref, mag, tol = (torch.zeros(b, R, D, dtype=F64) for _ in range(3))
    N = torch.zeros(R)
    for t, (sa, sb, _, _) in enumerate(terms):
        for slot, g, other in ((sa, dG[t, rows, :], P[:, sb]), (sb, dG[t, :, rows].t(), P[:, sa])):
            ref[:, slot] += g @ other
            mag[:, slot] += g.abs() @ other.abs()
            N[slot] += B
        if dG_tol is not None:
            tol[:, sa] += dG_tol[t, rows, :] @ P[:, sb].abs()
            tol[:, sb] += dG_tol[t, :, rows].t() @ P[:, sa].abs()
    return ref, tol + N[None, :, None].double() * (U * mag + TINY)


# ------------------------------------------------------------------------------------------------ the checker
def _fail(what, bad, got, ref, tol, axes):
    idx = bad.nonzero()[:SHOW].tolist()
    rows = []
    for ix in idx:
        t = tuple(ix)
        rows.append(", ".join(f"{a} {i}" for a, i in zip(axes, ix)) + f": got {float(got[t])!r}, want {float(ref[t])!r}" + (f", bound {float(tol[t]):.3e}" if tol is not None else ""))
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong; first: " + "; ".join(rows))


def close(got, ref, tol, what, key, axes):
    """|got - ref| <= tol at every element (NaN fails), the failure names the element by `axes`; keeps the worst ratio under `key`"""
    assert got.shape == ref.shape == tol.shape, (what, got.shape, ref.shape, tol.shape)
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    if bad.any():
        _fail(what, bad, got, ref, tol, axes)
    pos = tol > 0
    if key is not None and pos.any():
        WORST[key] = max(WORST.get(key, 0.0), float((err[pos] / tol[pos]).max()))


def exact(got, ref, what, axes):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = ~(got == ref)
    if bad.any():
        _fail(what, bad, got, ref, None, axes)


def check(d, ref, r, o, common=True):
    """One launch (rank r, row0 = r b_local) against the reference, in the order of the chain so that a wrong link is named and not
    what it feeds.  o: CPU tensors w [T, W], stats [T, B, 4], dG [T, B, B], term_loss [T], loss [], dls [], d_pooled [b, R, D].
    common False: w, stats and dG, which do not depend on the rank, are bitwise those of a launch that was checked."""
    name, R = f"{d['name']} rank {r}", ref["ranks"][r]
    if common:
        check_common(d, ref, name, o)
    check_rank(d, ref, r, name, R, o)


def check_common(d, ref, name, o):
    exact(o["w"], ref["w32"], f"{name}: w", ("term", "rank"))
    close(o["stats"], ref["stats"], ref["stats_tol"], f"{name}: stats", None, ("term", "row", "column"))
    for k, key in enumerate(("lse_row", "lse_col", "ce", "dsum")):          # (passed: only the ratios, per column of stats)
        close(o["stats"][:, :, k], ref["stats"][:, :, k], ref["stats_tol"][:, :, k], f"{name}: stats[{k}]", f"loss {key}", ("term", "row"))
    close(o["dG"], ref["dG"], ref["dG_tol"], f"{name}: dG", "loss dG", ("term", "row", "column"))


def check_rank(d, ref, r, name, R, o):
    tl = o["term_loss"]
    exact(torch.isnan(tl), ~R["live"], f"{name}: term_loss is NaN", ("term",))
    dead = ~R["live"]
    if dead.any():
        bits = tl.view(torch.int32)[dead]
        assert (bits == QNAN).all(), f"{name}: term_loss of a term with no valid row is not the kernel's quiet NaN: {[hex(int(x) & 0xFFFFFFFF) for x in bits[:SHOW]]}"
    live = R["live"]
    close(tl[live], R["term_loss"][live], R["term_tol"][live], f"{name}: term_loss (live terms)", "loss term_loss", ("live term",))
    close(o["loss"].reshape(1), R["loss"].reshape(1), R["loss_tol"].reshape(1), f"{name}: loss", "loss loss", ("element",))
    close(o["dls"].reshape(1), R["dls"].reshape(1), R["dls_tol"].reshape(1), f"{name}: d_logit_scale", "loss d_logit_scale", ("element",))
    if not live.any():
        assert float(o["loss"]) == 0.0 and float(o["dls"]) == 0.0, f"{name}: no live term: loss and d_logit_scale are exactly 0"
    dp = o["d_pooled"]
    unused = [sl for sl in range(d["R"]) if sl not in ref["used"]]
    for sl in unused:
        exact(dp[:, sl], torch.zeros_like(dp[:, sl]), f"{name}: d_pooled of slot {sl}, which no term names", ("row", "column"))
    close(dp, R["d_pooled"], R["d_pooled_tol"], f"{name}: d_pooled", "loss d_pooled", ("row", "slot", "column"))
    iso, iso_tol = dpooled64(d, o["dG"].double(), None, r)
    close(dp, iso, iso_tol, f"{name}: d_pooled against the kernel's own dG", "loss d_pooled | dG", ("row", "slot", "column"))


# ------------------------------------------------------------------------------------------------ fp32 restatement of the kernels
def _block_sum(part):
    """part [..., 256] per-thread partial sums -> wave_sum (xor butterfly over 64 lanes) then ((0 + w0) + w1) + w2) + w3"""
    v = part.reshape(*part.shape[:-1], 4, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    t = torch.zeros(part.shape[:-1], dtype=F32)
    for k in range(4):
        t = t + v[..., k, 0]
    return t


def _strided(x, fill):
    """[T, B, B] -> [T, B, trips, 256]: entry j of a row goes to thread j % 256, trip j // 256"""
    T, B, _ = x.shape
    trips = LC.cdiv(B, 256)
    p = torch.full((T, B, trips * 256), fill, dtype=F32)
    p[:, :, :B] = x
    return p.reshape(T, B, trips, 256)


def emulate(d, r, common=None, **faults):
    """one launch at rank r -> the dict check() takes.  common: emulate_common(d) of an earlier rank of the same case"""
    c = common or emulate_common(d, **faults)
    T, b, cnt, s, ds = d["T"], d["b_local"], c["cnt"], c["s"], c["ds"]
    term_loss = torch.empty(T, dtype=F32)
    tot, dtot, k_live = torch.zeros(()), torch.zeros(()), 0
    for t in range(T):
        n = cnt[t, r]
        if n > 0:
            term_loss[t] = s[t, r] / (2.0 * n)
            tot, dtot, k_live = tot + term_loss[t], dtot + ds[t, r] / (2.0 * n), k_live + 1
        else:
            term_loss.view(torch.int32)[t] = QNAN
    k_live = torch.tensor(float(max(k_live, 1)))
    return dict(w=c["w"], stats=c["stats"], dG=c["dG"], term_loss=term_loss, loss=tot / k_live, dls=dtot / k_live,
                d_pooled=c["d_pooled"][r * b:(r + 1) * b].clone())


def emulate_common(d, slices=4, n_from_rank0=False, ignore_or=False, max_subtract=True):
    """The five kernels' statements in fp32 torch with their summation grouping: the Gram chain over d (products rounded: no fma, the
    worse case), 256-strided partials then the wave and block tree, sequential sums in reduce_terms, four slices in dpooled.  The
    keyword arguments plant the faults the checker must find.  -> the dict check() takes"""
    B, R, D, T, b, W, terms = d["B"], d["R"], d["D"], d["T"], d["b_local"], d["W"], d["terms"]
    P = d["pooled"]
    Tm = torch.exp(d["s"])
    A = torch.stack([P[:, t[0]] for t in terms])
    Bm = torch.stack([P[:, t[1]] for t in terms])
    G = torch.zeros(T, B, B, dtype=F32)
    for k in range(D):
        G = G + A[:, :, None, k] * Bm[:, None, :, k]
    l = Tm * G
    st = []
    for L in (l, l.transpose(1, 2)):
        m = L.max(2).values if max_subtract else torch.zeros(T, B)
        p = torch.exp(L - m[:, :, None])
        ps, pl = _strided(p, 0.0), _strided(p * L, 0.0)
        acc_s, acc_e = torch.zeros(T, B, 256), torch.zeros(T, B, 256)
        for k in range(ps.shape[2]):
            acc_s, acc_e = acc_s + ps[:, :, k], acc_e + pl[:, :, k]
        sr, er = _block_sum(acc_s), _block_sum(acc_e)
        st.append((m + torch.log(sr), er / sr))
    diag = torch.diagonal(l, dim1=1, dim2=2)
    (lse_r, e_r), (lse_c, e_c) = st
    stats = torch.stack([lse_r, lse_c, (lse_r - diag) + (lse_c - diag), (e_r - diag) + (e_c - diag)], 2)
    use = [(t[0], t[1], t[2], 0) for t in terms] if ignore_or else terms
    valid = term_valid(use, d["present"])
    zero = torch.zeros((), dtype=F32)
    cnt, s, ds = torch.zeros(T, W), torch.zeros(T, W), torch.zeros(T, W)
    for k in range(b):
        v = valid[:, k::b]          # row r' b + k of every rank r'
        cnt = cnt + v.float()
        s = torch.where(v, s + stats[:, k::b, 2], s)
        ds = torch.where(v, ds + stats[:, k::b, 3], ds)
    if n_from_rank0:
        cnt = cnt[:, :1].expand(T, W).contiguous()
    nl = (cnt > 0).float().sum(0)
    denom = torch.where(nl > 0, nl, torch.ones(()))
    w = torch.where(cnt > 0, 1.0 / (2.0 * cnt * denom[None, :]), zero)
    # dgram
    wrow = torch.where(valid, w[:, torch.arange(B) // b], zero)
    eye = torch.eye(B)[None]
    g = torch.zeros(T, B, B)
    g = g + wrow[:, :, None] * (torch.exp(l - lse_r[:, :, None]) - eye)
    g = g + wrow[:, None, :] * (torch.exp(l - lse_c[:, None, :]) - eye)
    dG = Tm * g
    # dpooled
    red = []
    for sl in range(4):
        acc = torch.zeros(B, R, D)          # every rank's rows at once: a launch computes those of its own rank
        for t, (sa, sb, _, _) in enumerate(terms):
            for j in range(sl, B, 4):
                acc[:, sa] = acc[:, sa] + dG[t, :, j, None] * P[j, sb][None, :]
            for j in range(sl, B, 4):
                acc[:, sb] = acc[:, sb] + dG[t, j, :, None] * P[j, sa][None, :]
        red.append(acc)
    dp = red[0]
    for sl in range(1, slices):
        dp = dp + red[sl]
    return dict(w=w, stats=stats, dG=dG, cnt=cnt, s=s, ds=ds, d_pooled=dp)
