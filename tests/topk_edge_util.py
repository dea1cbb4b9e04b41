"""Helpers of the top-k retrieval tests (tests/test_retrieval_gpu.py; checked themselves by tests/test_retrieval_cpu.py): the
reference of mca_cosine_topk_f32's semantics as include/mca_hip.h states them, the operands of a case inside frames, the checker,
and a torch restatement of the kernel's chunked selection that can carry a planted fault.  Plain functions on any device.

The reference: the candidates of a row (valid, not excluded, score not NaN) in a stable sort by (-score, index), +0 and -0 equal,
padded with index -1 / score -inf.  Integer-valued operands in {-2 .. 2} make every score exact in any order (|sum| < 2^24) and
ties abound, so index and score are compared exactly."""
import torch

import topk_cases as TC
from eval_edge_util import F32, F64, I32, PAD, framed_i32, gather_index, gen, ints, out, untouched          # noqa: F401
from gemm_edge_util import _framed, assert_exact, assert_guard_intact
from row_edge_util import framed_in

NEG_INF = float("-inf")


def topk_ref(S, k, tvalid=None, exclude=None, tie_high=False):
    """S [nq, nt] (any float dtype; NaN, +-inf and +-0 allowed) -> (score [nq, k] of S's dtype, index [nq, k] int64).
    tie_high: the planted fault, equal scores in DESCENDING index order."""
    nq, nt = S.shape
    dev = S.device
    cols = torch.arange(nt, device=dev)[None, :].expand(nq, nt)
    cand = ~torch.isnan(S)
    if tvalid is not None:
        cand = cand & (tvalid.reshape(1, -1).to(dev) != 0)
    if exclude is not None:
        cand = cand & (cols != exclude.reshape(-1, 1).to(dev))
    key = torch.where(cand, -S.double(), torch.zeros((), dtype=F64, device=dev)) + 0.0          # -0 + 0 = +0: the two zeros tie
    if tie_high:
        order = torch.argsort(key.flip(1), dim=1, stable=True)
        order = (nt - 1 - order) if nt else order
    else:
        order = torch.argsort(key, dim=1, stable=True)                      # by (-score, index) ...
    late = torch.argsort((~cand).gather(1, order).to(torch.int8), dim=1, stable=True)          # ... candidates first, order kept
    order = order.gather(1, late)
    count = cand.sum(1, keepdim=True)
    index = torch.full((nq, k), -1, dtype=torch.int64, device=dev)
    score = torch.full((nq, k), NEG_INF, dtype=S.dtype, device=dev)
    w = min(k, nt)
    have = torch.arange(w, device=dev)[None, :] < count
    index[:, :w] = torch.where(have, order[:, :w], index[:, :w])
    score[:, :w] = torch.where(have, S.gather(1, order[:, :w]), score[:, :w])
    return score, index


def brute_force(S, k, tvalid=None, exclude=None):
    """the same semantics with python loops and comparisons only (tiny matrices): lists of k (score, index) per row"""
    rows = []
    for r, row in enumerate(S.tolist()):
        c = [(s, j) for j, s in enumerate(row) if s == s and (tvalid is None or tvalid[j]) and (exclude is None or j != int(exclude[r]))]
        picked = []
        while c and len(picked) < k:
            best = c[0]
            for x in c[1:]:
                if x[0] > best[0] or (x[0] == best[0] and x[1] < best[1]):
                    best = x
            picked.append(best)
            c.remove(best)
        rows.append(picked + [(NEG_INF, -1)] * (k - len(picked)))
    return rows


# ------------------------------------------------------------------------------------------------ operands of a listed case
def valid_pattern(nt, dev):
    """two of three targets valid; the last target invalid (the tail of the last tile) when there is more than one"""
    v = (torch.arange(nt, device=dev) % 3 != 1)
    if nt > 1:
        v[nt - 1] = False
    return v


def exclude_pattern(nq, nt, dev):
    """query r may not return target r % nt; every fifth query excludes nothing (-1)"""
    r = torch.arange(nq, device=dev)
    return torch.where(r % 5 == 4, torch.full_like(r, -1), r % nt)


def framed_u8(t):
    """a 1-d uint8 tensor inside a frame of 0xFF bytes: a stray read is 'valid'"""
    _, _, view = _framed(1, t.numel(), t.numel() + PAD, torch.uint8, t.device, 0xFF, 0)
    view.copy_(t.reshape(1, -1).to(torch.uint8))
    return view[0]


def operands(c, q, t, dev):
    """q [q_rows, d] and t [nt, d] of a case into NaN frames, with the case's optional arguments"""
    nq, nt, d = c["nq"], c["nt"], c["d"]
    return dict(q=framed_in(q, d + PAD), t=framed_in(t, d + PAD),
                qidx=framed_i32(gather_index(nq, q.shape[0]).to(dev)) if c["qidx"] else None,
                tvalid=framed_u8(valid_pattern(nt, dev)) if c["tvalid"] else None,
                exclude=framed_i32(exclude_pattern(nq, nt, dev)) if c["exclude"] else None)


def outputs(c, dev, short=0):
    nq, k = c["nq"], c["k"]
    need = TC.workspace_bytes(nq, c["nt"], k)
    return dict(score=out(nq, k, dev), index=out(nq, k, dev, I32), ws=out(1, need // 4 - short, dev, I32), need=need)


def topk_setup(c, dev, seed=48):
    g = gen(seed, dev)
    t = ints((c["nt"], c["d"]), g, 2)
    q = ints((c["nq"] + 5 if c["qidx"] else c["nq"], c["d"]), g, 2)
    return operands(c, q, t, dev), outputs(c, dev)


def scores64(c, T):
    """the [nq, nt] float64 score matrix of a case's operands (exact for integer operands)"""
    q = T["q"][T["qidx"].long()] if T["qidx"] is not None else T["q"]
    return q.double() @ T["t"].double().t()


def case_ref(c, T, S=None, **kw):
    S = scores64(c, T) if S is None else S
    return topk_ref(S, c["k"], T["tvalid"], T["exclude"].long() if T["exclude"] is not None else None, **kw)


def topk_check(c, T, O, S=None):
    """index, then score, at every element; then the frames.  S: the score matrix when it is not the exact product"""
    score, index = case_ref(c, T, S)
    name = c["name"]
    assert_exact(O["index"].t, index.to(I32), f"{name}: index (row = the query, column = the place)")
    assert_exact(O["score"].t, score.float(), f"{name}: score (row = the query, column = the place)")
    inside = (O["index"].t >= -1) & (O["index"].t < c["nt"])
    assert bool(inside.all()), f"{name}: an index outside -1 .. nt - 1"
    for key in ("score", "index", "ws"):
        assert_guard_intact(O[key], f"{name}: {key}")


# ------------------------------------------------------------------------------------------------ torch restatement of the kernel
FAULTS = ("tie_high", "merge_drop", "tail", "exclude_ignored", "pad_sentinel")


def topk_emulate(c, T, O, fault=None):
    """The kernel's plan restated: the best k of every 1024-target chunk, then the chunks' lists merged under the same order;
    stored where the kernel stores.  fault: one of FAULTS, planted."""
    k, nt, nq = c["k"], c["nt"], c["nq"]
    S = scores64(c, T)
    dev = S.device
    tv = T["tvalid"].clone() if T["tvalid"] is not None else torch.ones(nt, dtype=torch.uint8, device=dev)
    ex = T["exclude"].long() if (T["exclude"] is not None and fault != "exclude_ignored") else None
    if fault == "tail":          # the zero-filled columns of the last tile taken for targets
        pad = TC.cdiv(nt, TC.TILE) * TC.TILE - nt
        S = torch.cat([S, torch.zeros(nq, pad, dtype=F64, device=dev)], 1)
        tv = torch.cat([tv, torch.ones(pad, dtype=torch.uint8, device=dev)])
    part_s, part_i = [], []
    for c0 in range(0, S.shape[1], TC.CHUNK):
        s, i = topk_ref(S[:, c0:c0 + TC.CHUNK], k, tv[c0:c0 + TC.CHUNK], ex - c0 if ex is not None else None, tie_high=fault == "tie_high")
        if fault == "merge_drop":
            s[:, k - 1], i[:, k - 1] = NEG_INF, -1
        part_s.append(s)
        part_i.append(torch.where(i >= 0, i + c0, i))
    if part_s:
        ps, pi = torch.cat(part_s, 1), torch.cat(part_i, 1)
        # merge: the entries in ascending target index (padding last, as NaN: no candidate), so that a place in this row stands
        # for the index in the tie rule; then the same selection over the entries
        by_index = torch.argsort(torch.where(pi >= 0, pi, torch.full_like(pi, 2 ** 40)), dim=1, stable=True)
        ps, pi = ps.gather(1, by_index), pi.gather(1, by_index)
        ps = torch.where(pi >= 0, ps, torch.full_like(ps, float("nan")))
        s, j = topk_ref(ps, k, tie_high=fault == "tie_high")
        idx = torch.where(j >= 0, pi.gather(1, j.clamp_min(0)), j)
    else:
        s, idx = torch.full((nq, k), NEG_INF, dtype=F64, device=dev), torch.full((nq, k), -1, dtype=torch.int64, device=dev)
    if fault == "pad_sentinel":
        keep = idx >= 0
        O["score"].t[keep] = s.float()[keep]
        O["index"].t[keep] = idx.to(I32)[keep]
        return
    O["score"].t.copy_(s.float())
    O["index"].t.copy_(idx.to(I32))
