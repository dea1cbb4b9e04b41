"""Helpers of the streaming contrastive-loss tests (tests/test_loss_stream_gpu.py; checked themselves by
tests/test_loss_stream_cpu.py): the element-wise bounds of mca_contrastive_stream_fwd_bwd derived in docs/parity.md ("Streaming
contrastive loss: every element"), the checker of one launch, and an fp32 restatement of the three kernels of csrc/loss_stream.hip
in their own summation grouping.  The float64 values are those of tests/loss_edge_util.py's reference(), which restates
csrc/loss.hip's header formulas; only the bounds are this kernel's own.  Everything here runs on the CPU."""
import math

import torch

import loss_edge_util as U
import loss_stream_cases as SC
from loss_edge_util import EXPF_ULP, F32, F64, LOGF_ULP, QNAN, TINY, WORST, close, exact, make_data, term_valid          # noqa: F401

UR = U.U          # fp32 unit roundoff
NEG = -3.0e38     # ST_NEG: the running maximum of a lane that has seen no column yet


def roundings(B):
    """(NF, NR) of a row of B logits: NF exp factors an addend passes through (its own expf, the rescale of every later tile of its
    lane, the combine of the 8 lanes) and NR roundings of adds and products it meets (16 adds and one rescale product per tile,
    8 products and 8 adds in the combine)."""
    nt = SC.cdiv(B, SC.TJ)
    return nt + 1, 16 * nt + nt + 2 * SC.LANES


def reference(d):
    """loss_edge_util.reference(d) with every bound replaced by the streaming kernel's (docs/parity.md)."""
    ref = U.reference(d)
    B, T, b, W, terms = d["B"], d["T"], d["b_local"], d["W"], d["terms"]
    s = float(d["s"])
    Tm = math.exp(s)
    l, dl = ref["l"], ref["dl"]          # dl: a chain of D fused multiply-adds meets fewer roundings than the dense kernel's bound allows
    NF, NR = roundings(B)
    side = {}
    for name, L, DL in (("row", l, dl), ("col", l.transpose(1, 2), dl.transpose(1, 2))):
        m = L.max(2).values
        lse = torch.logsumexp(L, 2)
        Pm = torch.exp(L - lse[:, :, None])
        gap = (L - m[:, :, None]).abs()          # the arguments of an addend's exp factors are all <= 0 and sum to l - max
        dlse = DL.max(2).values + UR * (Pm * gap).sum(2) + (2 * EXPF_ULP * NF + NR) * UR + B * NF * TINY \
            + 2 * LOGF_ULP * UR * math.log(B) + UR * lse.abs()
        E = (Pm * L).sum(2)
        e = torch.expm1(DL + UR * gap + 2 * EXPF_ULP * NF * UR)
        den = 1 - (Pm * e).sum(2)
        assert (den > 0.5).all()
        dE = ((Pm * e * (L - E[:, :, None]).abs()).sum(2) + (Pm * (1 + e) * DL).sum(2) + (2 * NR + 2) * UR * (Pm * (1 + e) * L.abs()).sum(2)
              + B * NF * TINY * L.abs().max(2).values) / den
        side[name] = dict(lse=lse, P=Pm, dlse=dlse, E=E, dE=dE)
    r_, c_ = side["row"], side["col"]
    diag, ddiag = torch.diagonal(l, dim1=1, dim2=2), torch.diagonal(dl, dim1=1, dim2=2)
    ce = (r_["lse"] - diag) + (c_["lse"] - diag)
    dce = r_["dlse"] + c_["dlse"] + 2 * ddiag + UR * ((r_["lse"] - diag).abs() + (c_["lse"] - diag).abs() + ce.abs())
    dsum = (r_["E"] - diag) + (c_["E"] - diag)
    ddsum = r_["dE"] + c_["dE"] + 2 * ddiag + UR * ((r_["E"] - diag).abs() + (c_["E"] - diag).abs() + dsum.abs())
    out = dict(ref)
    out["dense_ranks"] = ref["ranks"]          # the dense kernel's bounds, for the test that holds the two kernels against each other
    out["lse"] = torch.stack([r_["lse"], c_["lse"]])          # [2, T, B]
    out["lse_tol"] = torch.stack([r_["dlse"], c_["dlse"]])
    out["erat"] = torch.stack([r_["E"], c_["E"]])
    out["erat_tol"] = torch.stack([r_["dE"], c_["dE"]])
    out["diag"], out["diag_tol"] = diag, ddiag
    assert torch.isfinite(out["lse_tol"]).all() and torch.isfinite(out["erat_tol"]).all()
    valid, n, nl = ref["valid"], ref["n"], ref["nl"]
    z = torch.zeros((), dtype=F64)
    ranks = []
    for r in range(W):
        rows = slice(r * b, (r + 1) * b)
        v = valid[:, rows]
        cnt = n[:, r].double()
        live = cnt > 0
        two_n = (2 * cnt).clamp_min(1)

        def mean_terms(x, dx):
            """stream_reduce_kernel sums as reduce_terms_kernel does: b - 1 adds and a division per term, then T adds and a division"""
            xs, axs, dxs = torch.where(v, x[:, rows], z).sum(1), torch.where(v, x[:, rows].abs(), z).sum(1), torch.where(v, dx[:, rows], z).sum(1)
            per, dper = xs / two_n, (dxs + (b + 1) * UR * axs) / two_n
            k = max(int(nl[r]), 1)
            tot = torch.where(live, per, z).sum() / k
            dtot = (torch.where(live, dper, z).sum() + (T + 2) * UR * torch.where(live, per.abs(), z).sum()) / k
            return per, dper, tot, dtot

        tl, dtl, loss, dloss = mean_terms(ce, dce)
        _, _, dls, ddls = mean_terms(dsum, ddsum)
        ranks.append(dict(term_loss=tl, term_tol=dtl, live=live, loss=loss, loss_tol=dloss, dls=dls, dls_tol=ddls))
    # dG is never stored; its bound feeds d_pooled's.  The statement per element is the dense kernel's (the subtraction, w's rounding,
    # the product by w, the add, the product by T, T = expf(s)), with this kernel's lse bounds
    w = torch.where(n > 0, 1.0 / (2.0 * n.double() * nl.clamp_min(1).double()[None, :]), z)
    wrow = torch.where(valid, w[:, torch.arange(B) // b], z)
    eye = torch.eye(B, dtype=F64)[None]
    Pr, Pc = r_["P"], c_["P"].transpose(1, 2)
    K = 5 + 2 * EXPF_ULP
    er = torch.expm1(dl + r_["dlse"][:, :, None] + UR * (l - r_["lse"][:, :, None]).abs() + 2 * EXPF_ULP * UR)
    ec = torch.expm1(dl + c_["dlse"][:, None, :] + UR * (l - c_["lse"][:, None, :]).abs() + 2 * EXPF_ULP * UR)
    dG_tol = Tm * (wrow[:, :, None] * (Pr * er + K * UR * (Pr - eye).abs() + TINY) + wrow[:, None, :] * (Pc * ec + K * UR * (Pc - eye).abs() + TINY))
    out["dG_tol"] = dG_tol
    # d_pooled: one chain of fused multiply-adds over the N addends of a slot, (term, direction, y) ascending: an addend meets at most
    # N roundings, which is what dpooled64 allows the dense kernel's slices
    for r in range(W):
        ranks[r]["d_pooled"], ranks[r]["d_pooled_tol"] = U.dpooled64(d, ref["dG"], dG_tol, r)
    out["ranks"] = ranks
    return out


def check(d, ref, r, o, common=True):
    """One launch (rank r) against the reference.  o: CPU tensors w [T, W], lse [2, T, B], erat [2, T, B], diag [T, B], term_loss [T],
    loss [], dls [], d_pooled [b, R, D]."""
    name, R = f"{d['name']} rank {r}", ref["ranks"][r]
    if common:
        exact(o["w"], ref["w32"], f"{name}: w", ("term", "rank"))
        close(o["diag"], ref["diag"], ref["diag_tol"], f"{name}: diag", "stream diag", ("term", "row"))
        close(o["lse"], ref["lse"], ref["lse_tol"], f"{name}: lse", "stream lse", ("direction", "term", "row"))
        close(o["erat"], ref["erat"], ref["erat_tol"], f"{name}: E / S", "stream erat", ("direction", "term", "row"))
    tl = o["term_loss"]
    exact(torch.isnan(tl), ~R["live"], f"{name}: term_loss is NaN", ("term",))
    dead, live = ~R["live"], R["live"]
    if dead.any():
        bits = tl.view(torch.int32)[dead]
        assert (bits == QNAN).all(), f"{name}: term_loss of a term with no valid row is not the kernel's quiet NaN: {[hex(int(x) & 0xFFFFFFFF) for x in bits[:6]]}"
    close(tl[live], R["term_loss"][live], R["term_tol"][live], f"{name}: term_loss (live terms)", "stream term_loss", ("live term",))
    close(o["loss"].reshape(1), R["loss"].reshape(1), R["loss_tol"].reshape(1), f"{name}: loss", "stream loss", ("element",))
    close(o["dls"].reshape(1), R["dls"].reshape(1), R["dls_tol"].reshape(1), f"{name}: d_logit_scale", "stream d_logit_scale", ("element",))
    if not live.any():
        assert float(o["loss"]) == 0.0 and float(o["dls"]) == 0.0, f"{name}: no live term: loss and d_logit_scale are exactly 0"
    dp = o["d_pooled"]
    for sl in range(d["R"]):
        if sl not in ref["used"]:
            exact(dp[:, sl], torch.zeros_like(dp[:, sl]), f"{name}: d_pooled of slot {sl}, which no term names", ("row", "column"))
    close(dp, R["d_pooled"], R["d_pooled_tol"], f"{name}: d_pooled", "stream d_pooled", ("row", "slot", "column"))


# ------------------------------------------------------------------------------------------------ fp32 restatement of the kernels
def _lane_order(x, fill):
    """[T, B, B] -> [T, B, 8, tiles, 16]: the logits of an owner row as its 8 lanes meet them (lane = 2 wave + half; column y of a
    tile is wave y // 32, q = y % 32 = (r & 3) + 4 half + 8 (r >> 2), register r)"""
    T, B, _ = x.shape
    nt = SC.cdiv(B, SC.TJ)
    p = torch.full((T, B, nt * SC.TJ), fill, dtype=x.dtype)
    p[:, :, :B] = x
    v = p.reshape(T, B, nt, 4, 4, 2, 4)          # tile, wave, r >> 2, half, r & 3
    return v.permute(0, 1, 3, 5, 2, 4, 6).reshape(T, B, 8, nt, 16)


def _online(L, drop_rescale=False):
    """stream_stats_kernel for owner rows L [T, B, B] -> (lse, E / S)"""
    T, B, _ = L.shape
    v, ok = _lane_order(L, 0.0), _lane_order(torch.ones_like(L, dtype=torch.bool), False)
    neg = torch.tensor(NEG, dtype=F32)
    m, s, e = torch.full((T, B, 8), NEG, dtype=F32), torch.zeros(T, B, 8), torch.zeros(T, B, 8)
    for jt in range(v.shape[3]):
        lv, mk = v[:, :, :, jt], ok[:, :, :, jt]
        mn = torch.maximum(m, torch.where(mk, lv, neg).max(3).values)
        if not drop_rescale:
            sc = torch.exp(m - mn)
            s, e = s * sc, e * sc
        for r in range(16):
            p = torch.exp(lv[..., r] - mn)
            s = torch.where(mk[..., r], s + p, s)
            e = torch.where(mk[..., r], e + p * lv[..., r], e)
        m = mn
    M = m.max(2).values
    S, E = torch.zeros(T, B), torch.zeros(T, B)
    for k in range(8):
        f = torch.exp(m[:, :, k] - M)
        S, E = S + s[:, :, k] * f, E + e[:, :, k] * f
    return M + torch.log(S), E / S


def emulate_common(d, drop_rescale=False, skip_dir1_of=None):
    """The three kernels in fp32 torch with their summation grouping: the Gram chain over d ascending (products rounded: the worse
    case of the fused chain), the per-lane online softmax and the fixed-order combine, sequential sums in the reduction, one chain per
    d_pooled element over (term, direction, y).  The keyword arguments plant the faults the checker must find."""
    B, R, D, T, b, W, terms = d["B"], d["R"], d["D"], d["T"], d["b_local"], d["W"], d["terms"]
    P = d["pooled"]
    Tm = torch.exp(d["s"])
    A = torch.stack([P[:, t[0]] for t in terms])
    Bm = torch.stack([P[:, t[1]] for t in terms])
    G = torch.zeros(T, B, B, dtype=F32)
    for k in range(D):
        G = G + A[:, :, None, k] * Bm[:, None, :, k]
    l = Tm * G
    (lse_r, e_r), (lse_c, e_c) = _online(l, drop_rescale), _online(l.transpose(1, 2).contiguous(), drop_rescale)
    diag = torch.diagonal(l, dim1=1, dim2=2)
    ce, dsum = (lse_r - diag) + (lse_c - diag), (e_r - diag) + (e_c - diag)
    valid = term_valid(terms, d["present"])
    zero = torch.zeros((), dtype=F32)
    cnt, s, ds = torch.zeros(T, W), torch.zeros(T, W), torch.zeros(T, W)
    for k in range(b):
        v = valid[:, k::b]
        cnt = cnt + v.float()
        s = torch.where(v, s + ce[:, k::b], s)
        ds = torch.where(v, ds + dsum[:, k::b], ds)
    nl = (cnt > 0).float().sum(0)
    denom = torch.where(nl > 0, nl, torch.ones(()))
    w = torch.where(cnt > 0, 1.0 / (2.0 * cnt * denom[None, :]), zero)
    wrow = torch.where(valid, w[:, torch.arange(B) // b], zero)
    eye = torch.eye(B)[None]
    g = torch.zeros(T, B, B)
    g = g + wrow[:, :, None] * (torch.exp(l - lse_r[:, :, None]) - eye)
    g = g + wrow[:, None, :] * (torch.exp(l - lse_c[:, None, :]) - eye)
    dG = Tm * g
    dp = torch.zeros(B, R, D)          # every rank's rows at once: a launch computes those of its own rank
    for t, (sa, sb, _, _) in enumerate(terms):
        for j in range(B):
            dp[:, sa] = dp[:, sa] + dG[t, :, j, None] * P[j, sb][None, :]
        if skip_dir1_of != t:
            for j in range(B):
                dp[:, sb] = dp[:, sb] + dG[t, j, :, None] * P[j, sa][None, :]
    return dict(w=w, lse=torch.stack([lse_r, lse_c]), erat=torch.stack([e_r, e_c]), diag=diag.contiguous(), cnt=cnt, s=s, ds=ds, d_pooled=dp)


def emulate(d, r, common=None, **faults):
    """one launch at rank r -> the dict check() takes"""
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
    return dict(w=c["w"], lse=c["lse"], erat=c["erat"], diag=c["diag"], term_loss=term_loss, loss=tot / k_live, dls=dtot / k_live,
                d_pooled=c["d_pooled"][r * b:(r + 1) * b].clone())
