"""Helpers of the token-table edge tests (tests/test_token_edges_gpu.py; checked themselves by tests/test_token_edges_cpu.py): the
framing of tests/gemm_edge_util.py and tests/row_edge_util.py around every operand of csrc/embedding.hip, the float64 and int64
references of the lookup and of the table gradient, the bounds derived in docs/parity.md ("Token tables: every element, at the
edges"), and fp32 restatements of the kernels' arithmetic, stored where the kernels store, that show every bound satisfiable
without a GPU.  Values are drawn on the CPU from seeded generators and references are computed there; `device` is where the framed
operands live and where the launch (the library, or the restatement) stores."""
import torch

import token_cases as TC
from gemm_edge_util import assert_close_elementwise, assert_exact, assert_guard_intact, framed_copy, guarded_out
from row_edge_util import assert_rows_untouched, framed_in

F32, I32, I64 = torch.float32, torch.int32, torch.int64
RENORM_REL = 2.0 ** -20        # 15.5 fp32 roundings of 2^-24 (docs/parity.md), rounded up to a power of two
NEAR = 2.0 ** -10              # relative distance of the near-threshold rows from max_norm
SUM_ULP = 2.0 ** -24
NORM_CLASSES = ("3x", "0.5x", "near above", "near below", "exactly at")
INT_MIN = {4: -2 ** 31, 8: -2 ** 63}
WORST = {}                     # output name -> largest |got - ref| / bound seen so far (where the bound is not 0)


def close(got, ref, tol, what, key):
    """assert_close_elementwise that also keeps the largest error / bound ratio under `key`"""
    assert_close_elementwise(got, ref, tol, what)
    pos = tol > 0
    if pos.any():
        WORST[key] = max(WORST.get(key, 0.0), float(((got.double() - ref.double()).abs()[pos] / tol.double()[pos]).max()))


def assert_bits(got, ref, what):
    """the same bits at every element of two fp32 [rows, cols] tensors (an int32 compare: -0 is not +0, a NaN equals itself)"""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bad = got.contiguous().view(I32) != ref.contiguous().view(I32)
    if bad.any():
        idx = bad.nonzero()[:8].tolist()
        rows = [(i, j, float(got[i, j]), float(ref[i, j])) for i, j in idx]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits; first (row, column, got, want): {rows}")


def _framed_at(make, offsets, mod, want):
    """make(byte_off) until the view's address is `want` modulo `mod` (the allocator's own alignment decides which offset does it)"""
    for bo in offsets:
        v = make(bo)
        if v.data_ptr() % mod == want:
            return v
    raise AssertionError(f"no offset of {offsets} puts the operand at {want} modulo {mod}")


def framed16(src, ld):
    """an fp32 input in a NaN frame, 16 but not 32 bytes aligned"""
    return _framed_at(lambda bo: framed_in(src, ld, bo), (16, 32, 48, 64), 32, 16)


def guarded16(rows, cols, ld, device):
    """an fp32 output in a sentinel frame, 16 but not 32 bytes aligned"""
    return _framed_at(lambda bo: guarded_out(rows, cols, ld, F32, byte_off=bo, device=device), (16, 32, 48, 64), 32, 16)


def framed_idx(idx, idx_bytes, device):
    """`tokens` indices of idx_bytes each inside a frame of -1 (0xFF..: out of range, so a read one element outside raises the flag or
    skips a token); int32 indices 4 but not 8 bytes aligned"""
    v = idx.clamp(INT_MIN[idx_bytes], 2 ** 31 - 1 if idx_bytes == 4 else 2 ** 63 - 1).to(I32 if idx_bytes == 4 else I64).reshape(1, -1).to(device)
    out = framed_copy(v, v.shape[1] + 3, 4 if idx_bytes == 4 else 0)[0]
    assert out.data_ptr() % idx_bytes == 0 and (idx_bytes == 8 or out.data_ptr() % 8 == 4)
    whole = torch.as_strided(out, (out.numel() + 6,), (1,), out.storage_offset() - 3)
    assert (whole[:3] == -1).all() and (whole[-3:] == -1).all()
    return out


def filled(g, value):
    g.t.copy_(value) if torch.is_tensor(value) else g.t.fill_(value)
    return g


def flat_of(g, n):
    """the n elements from a guarded view's element (0, 0) on, as the kernel addresses them"""
    return torch.as_strided(g.t, (n,), (1,), g.t.storage_offset())


def gen(seed):
    return torch.Generator().manual_seed(seed)


def packed_rows(tokens, period):
    """row of a packed placement each token maps to: sample i / period of (period + EXTRA) rows"""
    i = torch.arange(tokens)
    return (i // period) * (period + TC.EXTRA) + i % period


def n_packed(tokens, period):
    return TC.cdiv(tokens, period) * (period + TC.EXTRA)


# ================================================================================================ lookup: data
def norm_class(vocab, cls0):
    return (torch.arange(vocab) + cls0) % 5


def make_table(vocab, cols, max_norm, cls0, g):
    """fp32 [vocab, cols]; the row's norm class by row number: 3x, 0.5x, (1 + 2^-10)x, (1 - 2^-10)x max_norm, and exactly max_norm
    (one non-zero element of either sign, at column row % cols)"""
    w = torch.randn(vocab, cols, generator=g).double()
    w = torch.where(w == 0, torch.ones_like(w), w)
    cls = norm_class(vocab, cls0)
    target = max_norm * torch.tensor([3.0, 0.5, 1 + NEAR, 1 - NEAR, 1.0], dtype=torch.float64)[cls]
    w = (w / w.norm(dim=1, keepdim=True) * target[:, None]).float()
    eq = (cls == 4).nonzero().flatten()
    w[eq] = 0
    w[eq, eq % cols] = torch.where(eq % 2 == 0, max_norm, -max_norm).float()
    return w.contiguous()


def assert_table_classes(w, max_norm, cls0):
    """the near rows keep their 2^-10 distance (a thousand times the fp32 norm's error: fp32 and float64 decide alike), the
    exactly-at rows have an fp32 norm EQUAL to max_norm, whichever way it is summed"""
    cls = norm_class(w.shape[0], cls0)
    rel = w.double().norm(dim=1) / max_norm - 1
    for k, want in ((2, NEAR), (3, -NEAR)):
        assert ((rel[cls == k] - want).abs() <= 2.0 ** -20).all(), f"near rows ({NORM_CLASSES[k]}) are {NEAR} from max_norm"
    assert (rel[cls == 0] > 1).all() and (rel[cls == 1] < -0.4).all()
    at = w[cls == 4]
    assert (rel[cls == 4] == 0).all() and ((at != 0).sum(1) == 1).all()
    assert (torch.sqrt((at * at).sum(1)) == torch.tensor(max_norm, dtype=F32)).all(), "max_norm squared is exact in fp32"


def lookup_indices(case, which="pattern"):
    """int64 [tokens]; values an int32 operand cannot hold are clamped into it by framed_idx (INT64_MIN becomes INT32_MIN)"""
    vocab, n, cls0 = case["vocab"], case["tokens"], case["cls0"]
    pattern = case["pattern"] if which == "pattern" else which
    i = torch.arange(n)
    g = gen(1000 + n + vocab)
    big = next((r for r in range(vocab) if (r + cls0) % 5 == 0), 0)          # a row at 3x max_norm where there is one
    if pattern == "same":
        return torch.full((n,), big, dtype=I64)
    if pattern == "distinct":
        return (vocab - 1 - i) % vocab          # tokens <= vocab: every token another row
    if pattern == "ends":
        return torch.where(i % 2 == 0, 0, vocab - 1)
    if pattern == "straddle":          # rows on both sides of the renormalisation's first pass, two of them at 3x max_norm
        b = TC.GRID_CAP * TC.WAVES * TC.RENORM_CHUNK
        lo, hi = next(r for r in range(b - 1, 0, -1) if (r + cls0) % 5 == 0), next(r for r in range(b, vocab) if (r + cls0) % 5 == 0)
        return torch.tensor(([vocab - 1, 0, lo, b - 1, b, b + 1, hi, vocab - 1, 5, b] * TC.cdiv(n, 10))[:n], dtype=I64)
    if pattern == "oob-tail":          # out of range only among the last 5: behind the mark kernel's first pass
        idx = i % vocab
        idx[-4] = vocab
        return idx
    idx = torch.randint(0, vocab, (n,), generator=g)
    idx[0] = idx[-1]
    if pattern == "second":          # the second of two lookups: other rows than the first, and none the first one rescaled twice-ambiguously
        first = lookup_indices(case)
        named = torch.zeros(vocab, dtype=torch.bool)
        named[first] = True
        fresh = (~named).nonzero().flatten()
        kept = (named & (norm_class(vocab, cls0) != 0) & (norm_class(vocab, cls0) != 2)).nonzero().flatten()          # named before, never rescaled
        return torch.where(i % 2 == 0, kept[(i // 2) % len(kept)], fresh[torch.randint(0, len(fresh), (n,), generator=g)])
    if pattern == "oob":          # -1, vocab and the most negative value among valid ones; the first and the last token out of range
        bad = torch.tensor([-1, vocab, INT_MIN[8]], dtype=I64)
        sel = (i % 3 == 0) | (i == n - 1)
        idx = torch.where(sel, bad[(i // 3) % 3], idx)
    return idx.to(I64)


def lookup_setup(case, device, second=False):
    """every operand of one lookup, framed.  second: the case's second lookup (its own indices, add and destination) on the table
    and marker of the first: pass them in with T['table'], T['marker'], T['flag'] afterwards"""
    vocab, cols, n, period, ldd = case["vocab"], case["cols"], case["tokens"], case["period"], case["ldd"]
    g = gen(7 + (100 if second else 0))
    T = dict(w0=make_table(vocab, cols, case["max_norm"], case["cls0"], g), idx=lookup_indices(case, case["second"] if second else "pattern"))
    assert_table_classes(T["w0"], case["max_norm"], case["cls0"])
    T["valid"] = (T["idx"] >= 0) & (T["idx"] < vocab)
    T["add0"] = torch.randn(period, cols, generator=g) if case["add"] else None
    T["dst0"] = torch.randn(n, cols, generator=g) if case["acc"] else None
    T["dest"], T["dst_rows"] = packed_rows(n, period), n_packed(n, period)
    T["bstride"] = (period + TC.EXTRA) * ldd
    assert T["bstride"] > period * ldd
    T["table"] = filled(guarded_out(vocab, cols, cols, F32, device=device), T["w0"].to(device))          # the table is packed: ld == cols
    T["marker"] = filled(guarded_out(1, vocab, vocab + 3, I32, device=device), 0)
    T["flag"] = filled(guarded_out(1, 1, 4, I32, device=device), TC.FLAG_PRESET)
    T["add"] = framed16(T["add0"].to(device), cols) if case["add"] else None          # add's row stride IS cols
    T["idx_dev"] = framed_idx(T["idx"], case["idx_bytes"], device)
    T["dst"] = guarded16(T["dst_rows"], cols, ldd, device)
    if case["acc"]:
        T["dst"].t[T["dest"].to(device)] = T["dst0"].to(device)
    return T


def lookup_args(case, T):
    """mca_embedding_lookup's arguments up to the stream"""
    return (T["table"].data_ptr(), case["vocab"], case["cols"], case["max_norm"], T["idx_dev"].data_ptr(), case["idx_bytes"], case["tokens"], case["period"],
            None if T["add"] is None else T["add"].data_ptr(), T["dst"].data_ptr(), case["ldd"], T["bstride"], case["acc"], T["marker"].data_ptr(),
            T["flag"].data_ptr() if case["flag"] else None, TC.OOB_BIT)


# ================================================================================================ lookup: fp32 restatement
def renorm32(w, named, max_norm, twice=None):
    """embedding_renorm_marked_kernel's arithmetic on the named rows, in fp32 torch, in place.  twice: a row two wavefronts took,
    both from the norm they read before either stored (the planted fault)"""
    mn = torch.tensor(max_norm, dtype=F32)
    rows = named.nonzero().flatten()
    sub = w[rows]
    nrm = torch.sqrt((sub * sub).sum(1))
    sc = torch.where(nrm > mn, mn / (nrm + torch.tensor(1e-7, dtype=F32)), torch.ones((), dtype=F32))
    if twice is not None:
        sc = torch.where(rows == twice, sc * sc, sc)
    w[rows] = torch.where((sc != 1)[:, None], sub * sc[:, None], sub)


def lookup_emulate_into(case, T, fault=None):
    """the CPU stand-in of the three launches: marks, renormalises and gathers through the kernels' own address arithmetic on the
    flat destination.  fault: 'twice' (one row rescaled twice), 'idx+1' (one token's row taken from idx + 1), 'last-group' (the
    partial last group skipped), 'ldd' (ldd taken for cols)"""
    vocab, cols, n, period, ldd = case["vocab"], case["cols"], case["tokens"], case["period"], case["ldd"]
    idx, valid = T["idx"], T["valid"]
    if case["flag"] and not valid.all():
        T["flag"].t[0, 0] |= TC.OOB_BIT
    named = torch.zeros(vocab, dtype=torch.bool)
    named[idx[valid]] = True
    w = T["table"].t.clone()
    big = (named & (w.double().norm(dim=1) > 2 * case["max_norm"])).nonzero().flatten()
    renorm32(w, named, case["max_norm"], twice=int(big[0]) if fault == "twice" else None)
    T["table"].t.copy_(w)
    src = idx.clone()
    if fault == "idx+1":
        t = int(valid.nonzero()[-1])
        src[t] = (src[t] + 1) % vocab
    i = torch.arange(n)
    live = valid | bool(case["add"]) | (not case["acc"])          # (v < 0 && !add && accumulate) continue
    if fault == "last-group" and n % period:
        live = live & (i < n - n % period)
    val = torch.where(valid[:, None], w[src.clamp(0, vocab - 1)], torch.zeros((), dtype=F32))
    if case["add"]:
        val = val + T["add"][i % period]
    flat = flat_of(T["dst"], T["dst_rows"] * ldd)
    stride = cols if fault == "ldd" else ldd
    addr = ((i // period) * T["bstride"] + (i % period) * stride)[:, None] + torch.arange(cols)[None, :]
    if case["acc"]:
        val = val + flat[addr]
    flat[addr[live]] = val[live]


# ================================================================================================ lookup: the check
def lookup_check(case, T, what="", w_before=None, flag_before=TC.FLAG_PRESET):
    """marker and flag, then the table, then the destination composed from the table the launch left, then every guard.
    w_before: the table this lookup started from when it is not T['w0'] (a second lookup)"""
    what = what or case["name"]
    vocab, cols, n, period = case["vocab"], case["cols"], case["tokens"], case["period"]
    idx, valid, mn = T["idx"], T["valid"], case["max_norm"]
    w0 = T["w0"] if w_before is None else w_before
    # 1. marker, flag
    assert_exact(T["marker"].t.cpu(), torch.zeros(1, vocab, dtype=I32), f"{what}: marker (row = 0, column = the table row)")
    assert_guard_intact(T["marker"], f"{what}: marker")
    want_flag = flag_before | (TC.OOB_BIT if (case["flag"] and not valid.all()) else 0)
    assert int(T["flag"].t[0, 0]) == want_flag, f"{what}: flag word {int(T['flag'].t[0, 0])}, want {want_flag}"
    assert bool((~valid).any()) == bool(case["oob"]), "the case's pattern has an index out of range exactly when it says so"
    # 2. table
    named = torch.zeros(vocab, dtype=torch.bool)
    named[idx[valid]] = True
    norm = w0.double().norm(dim=1)
    resc = named & (norm > mn)
    got_w = T["table"].t.cpu()
    ref = torch.where(resc[:, None], w0.double() * mn / (norm[:, None] + 1e-7), w0.double())
    close(got_w, ref, torch.where(resc[:, None], RENORM_REL * ref.abs(), torch.zeros((), dtype=torch.float64)), f"{what}: table", "lookup table")
    assert_bits(got_w[~resc], w0[~resc], f"{what}: table rows no token names or at or below max_norm (row = its rank among them)")
    # 3. destination, bitwise, from the table as it was left
    i = torch.arange(n)
    val = torch.where(valid[:, None], got_w[idx.clamp(0, vocab - 1)], torch.zeros((), dtype=F32))
    if case["add"]:
        val = val + T["add0"][i % period]
    if case["acc"]:
        val = val + T["dst0"]
        if not case["add"]:
            val = torch.where(valid[:, None], val, T["dst0"])          # nothing to add: the old bits (val is the same value; -0 would not be)
    got = T["dst"].t.cpu()
    assert_bits(got[T["dest"]], val, f"{what}: destination (row = the token)")
    hit = set(T["dest"].tolist())
    if T["dst_rows"] - len(hit) <= 4096:
        assert_rows_untouched(got, [r for r in range(T["dst_rows"]) if r not in hit], f"{what}: destination")
    else:
        gap = torch.ones(T["dst_rows"], dtype=torch.bool)
        gap[T["dest"]] = False
        assert (got[gap].view(I32) == -1).all(), f"{what}: destination rows no token maps to"
    for k in ("table", "dst", "flag"):
        assert_guard_intact(T[k], f"{what}: {k}")
    return got_w


def lookup_snapshot(T):
    return {k: T[k].buf.clone() for k in ("table", "dst", "marker", "flag")}


# ================================================================================================ table gradient: data
def grad_indices(case):
    vocab, n, pattern = case["vocab"], case["tokens"], case["pattern"]
    i = torch.arange(n)
    g = gen(2000 + n + vocab)
    pad = case["padding_idx"] + (vocab if case["padding_idx"] < 0 else 0)
    if pattern == "one":          # a run as long as the token count; not the padding row where there is another
        return torch.full((n,), (vocab - 2) % vocab if pad == vocab - 1 else vocab - 1, dtype=I64)
    if pattern == "cyclic":
        return i % vocab
    if pattern == "distinct":
        return (i * 7) % vocab          # 7 and vocab = 300 are coprime
    if pattern == "descending":
        return ((n - 1 - i) * vocab) // n
    if pattern == "strict-descending":
        return vocab - 1 - i
    if pattern == "allpad":
        return torch.full((n,), pad if pad < vocab else 0, dtype=I64)          # (padding_idx = vocab: there is no padding row, all of row 0)
    if pattern == "alloob":
        return torch.tensor([-1, vocab, INT_MIN[8], vocab + 5], dtype=I64)[i % 4]
    if pattern == "three-rows":
        return torch.tensor([2, vocab - 1, 7])[torch.randint(0, 3, (n,), generator=g)]
    idx = torch.randint(0, vocab, (n,), generator=g)          # mixed: valid rows, the padding row, out of range
    idx = torch.where(i % 5 == 1, torch.tensor([-1, vocab, INT_MIN[8]], dtype=I64)[(i // 5) % 3], idx)
    idx = torch.where(i % 7 == 2, torch.full((), pad if pad < vocab else 0, dtype=I64), idx)
    idx[n - 1] = idx[0]
    return idx.to(I64)


def grad_setup(case, device, real):
    """dy inside NaN: columns [cols, ldy), the rows between samples AND the rows of tokens that are padding or out of range.
    real: randn, else integers in {-4 .. 4}; the initial dtable small non-zero integers (randn for real)"""
    vocab, cols, n, period, ldy = case["vocab"], case["cols"], case["tokens"], case["period"], case["ldy"]
    g = gen(11 + int(real))
    T = dict(idx=grad_indices(case), real=real)
    pad = case["padding_idx"] + (vocab if case["padding_idx"] < 0 else 0)
    valid = (T["idx"] >= 0) & (T["idx"] < vocab)
    T["key"] = torch.where(valid & (T["idx"] != pad), T["idx"], torch.full((), vocab, dtype=I64))
    live = T["key"] < vocab
    T["g"] = torch.randn(n, cols, generator=g) if real else torch.randint(-4, 5, (n, cols), generator=g).float()
    T["g"][~live] = float("nan")
    if real:
        T["init"] = torch.randn(vocab, cols, generator=g)
    else:
        T["init"] = (torch.randint(1, 5, (vocab, cols), generator=g) * (2 * torch.randint(0, 2, (vocab, cols), generator=g) - 1)).float()
    T["src"], rows = packed_rows(n, period), n_packed(n, period)
    T["bstride"] = (period + TC.EXTRA) * ldy
    full = framed_in(torch.full((rows, cols), float("nan"), device=device), ldy, 4)
    full[T["src"].to(device)] = T["g"].to(device)
    T["dy"] = full
    T["idx_dev"] = {ib: framed_idx(T["idx"], ib, device) for ib in (8, 4)}
    return T


def grad_outputs(case, T, device, det, scratch_floats=None):
    O = dict(dtable=filled(guarded_out(case["vocab"], case["cols"], case["cols"], F32, device=device), T["init"].to(device)), scratch=None)
    if det:
        need = 2 * case["tokens"] if scratch_floats is None else scratch_floats
        O["scratch"] = guarded_out(1, need, need + 3, F32, device=device)
    return O


def grad_args(case, T, O, idx_bytes):
    """mca_embedding_scatter_add's arguments up to the stream (the _det form appends scratch, scratch_floats)"""
    return (T["dy"].data_ptr(), case["ldy"], T["bstride"], case["period"], T["idx_dev"][idx_bytes].data_ptr(), idx_bytes, case["tokens"],
            O["dtable"].data_ptr(), case["vocab"], case["cols"], case["padding_idx"])


# ================================================================================================ table gradient: references
def sorted_tokens(key, reverse_ties=False):
    """the tokens in (key, position) order, and their keys: a stable sort.  reverse_ties: the planted fault"""
    n = key.numel()
    pos = torch.arange(n)
    order = torch.argsort(key * n + (n - 1 - pos if reverse_ties else pos))          # (key <= vocab, n < 2^31: no overflow in int64)
    return order, key[order]


def seq_sum32(init, key, g, vocab, order=None, direct=False):
    """fp32, one correctly rounded add at a time, as a plain sequential loop over each row's tokens in `order` (default: position):
    acc = 0; acc += g_k; dtable + acc  -  the header's order.  direct: dtable += g_k, what one atomic after another does"""
    if order is None:
        order = sorted_tokens(key)[0]
    sk = key[order]
    n = key.numel()
    first = torch.searchsorted(sk, sk)          # place of the first token of each token's row
    rank = torch.arange(n) - first
    out = init.clone()
    acc = out if direct else torch.zeros_like(init)
    live = sk < vocab
    by_rank = torch.argsort(rank, stable=True)
    counts = torch.bincount(rank).tolist()
    at = 0
    for cnt in counts:          # every row's rank-th token at once: the rows are distinct, each add is one fp32 add
        sel = by_rank[at:at + cnt]
        at += cnt
        sel = sel[live[sel]]
        if sel.numel():
            acc[sk[sel]] = acc[sk[sel]] + g[order[sel]]
    if not direct:
        touched = torch.zeros(vocab, dtype=torch.bool)
        touched[sk[live]] = True
        out[touched] = init[touched] + acc[touched]
    return out


def grad_ref64(T, vocab):
    """(float64 sum, per-row token count, sum of magnitudes with abs(init) inside)"""
    live = T["key"] < vocab
    k, gl = T["key"][live], T["g"][live].double()
    ref = T["init"].double().index_add_(0, k, gl)
    mag = T["init"].double().abs().index_add_(0, k, gl.abs())
    cnt = torch.zeros(vocab, dtype=torch.float64).index_add_(0, k, torch.ones(k.numel(), dtype=torch.float64))
    return ref, cnt, mag


def grad_emulate_into(case, T, O, det, fault=None):
    """the CPU stand-in: the det form's two launches (sort into the scratch, sum in the header's order), or the atomic form as
    sequential direct adds in REVERSED position order (an order atomics may take).  fault: 'pad' (the padding row summed),
    'ties' (equal keys sorted in reverse)"""
    vocab = case["vocab"]
    key, g = T["key"], T["g"]
    if fault == "pad":
        pad = case["padding_idx"] + (vocab if case["padding_idx"] < 0 else 0)
        key = torch.where(T["idx"] == pad, T["idx"], key)
    if det:
        order, sk = sorted_tokens(key, reverse_ties=fault == "ties")
        O["scratch"].t[0].view(I32)[:2 * case["tokens"]] = torch.cat([order, sk]).to(I32)
        O["dtable"].t.copy_(seq_sum32(T["init"], key, g, vocab, order=order))
    else:
        O["dtable"].t.copy_(seq_sum32(T["init"], key, g, vocab, order=sorted_tokens(key, reverse_ties=True)[0], direct=True))


def grad_check(case, T, O, det, what=""):
    """values at every element (exact for integer data; real data: the det form bitwise against the header's order, the atomic
    form within its bound), then the scratch, then the rows that must keep their bits, then the guards.  -> dtable on the CPU"""
    what = what or case["name"]
    vocab, n = case["vocab"], case["tokens"]
    got = O["dtable"].t.cpu()
    ref, cnt, mag = grad_ref64(T, vocab)
    if not T["real"]:
        assert float(mag.max()) < 2 ** 24
        assert_exact(got, ref.float(), f"{what}: dtable (integers)")
    elif det:
        if "seq" not in T:
            T["seq"] = seq_sum32(T["init"], T["key"], T["g"], vocab)
        assert_bits(got, T["seq"], f"{what}: dtable against (((g_0 + g_1) + g_2) + ...) in position order")
        close(got, ref, cnt[:, None] * SUM_ULP * mag, f"{what}: dtable", "dtable det")
    else:
        close(got, ref, cnt[:, None] * SUM_ULP * mag, f"{what}: dtable", "dtable atomic")
    if det:
        order, sk = sorted_tokens(T["key"])
        words = O["scratch"].t[0].view(I32).cpu()
        assert words.numel() == 2 * n
        assert_exact(words[:n].reshape(1, -1), order.to(I32).reshape(1, -1), f"{what}: scratch, tokens by (key, position) (row = 0, column = the place)")
        assert_exact(words[n:].reshape(1, -1), sk.to(I32).reshape(1, -1), f"{what}: scratch, keys (row = 0, column = the place)")
        assert_guard_intact(O["scratch"], f"{what}: scratch")
    assert_bits(got[cnt == 0], T["init"][cnt == 0], f"{what}: rows no contributing token names, the padding row among them (row = its rank among them)")
    assert_guard_intact(O["dtable"], f"{what}: dtable")
    return got


# ================================================================================================ refusals
BADARG, ALIGN = -1, -2


def lookup_refusals(L, case, T, stream=None):
    """every refused argument of mca_embedding_lookup, and rows == 0: (what, return code, wanted)"""
    a = list(lookup_args(case, T))
    TABLE, VOCAB, COLS, IDX, IB, ROWS, PERIOD, ADD, DST, LDD, BSTRIDE, MARKER, FLAG, BIT = 0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15
    calls = [("table NULL", {TABLE: None}, BADARG), ("idx NULL", {IDX: None}, BADARG), ("dst NULL", {DST: None}, BADARG), ("marker NULL", {MARKER: None}, BADARG),
             ("vocab 0", {VOCAB: 0}, BADARG), ("cols 0", {COLS: 0}, BADARG), ("rows -1", {ROWS: -1}, BADARG), ("period 0", {PERIOD: 0}, BADARG),
             ("idx_bytes 2", {IB: 2}, BADARG), ("flag with oob_bit 0", {FLAG: T["flag"].data_ptr(), BIT: 0}, BADARG),
             ("cols % 4", {COLS: case["cols"] - 2}, ALIGN), ("ldd % 4", {LDD: case["ldd"] + 2}, ALIGN), ("dst_bstride % 4", {BSTRIDE: T["bstride"] + 2}, ALIGN),
             ("table + 4", {TABLE: a[TABLE] + 4}, ALIGN), ("dst + 8", {DST: a[DST] + 8}, ALIGN), ("idx + 4 (int64)", {IDX: T["idx_dev"].data_ptr() + 4, IB: 8}, ALIGN),
             ("rows 0", {ROWS: 0}, 0)]
    if T["add"] is not None:
        calls.append(("add + 4", {ADD: a[ADD] + 4}, ALIGN))
    out = []
    for name, change, want in calls:
        b = list(a)
        for k, v in change.items():
            b[k] = v
        out.append((name, L.mca_embedding_lookup(*b, stream), want))
    return out


def grad_refusals(L, case, T, O, stream=None):
    """every refused argument of both table-gradient entry points, a scratch one float short, rows == 0"""
    a = list(grad_args(case, T, O, 8))
    DY, PERIOD, IDX, IB, ROWS, DTABLE, VOCAB, COLS = 0, 3, 4, 5, 6, 7, 8, 9
    need = 2 * case["tokens"]
    calls = [("dy NULL", {DY: None}, BADARG), ("idx NULL", {IDX: None}, BADARG), ("dtable NULL", {DTABLE: None}, BADARG), ("vocab 0", {VOCAB: 0}, BADARG),
             ("cols 0", {COLS: 0}, BADARG), ("rows -1", {ROWS: -1}, BADARG), ("period 0", {PERIOD: 0}, BADARG), ("idx_bytes 2", {IB: 2}, BADARG),
             ("idx + 4 (int64)", {IDX: a[IDX] + 4}, ALIGN), ("dy + 2", {DY: a[DY] + 2}, ALIGN), ("dtable + 2", {DTABLE: a[DTABLE] + 2}, ALIGN), ("rows 0", {ROWS: 0}, 0)]
    out = []
    for name, change, want in calls:
        b = list(a)
        for k, v in change.items():
            b[k] = v
        out.append((f"atomic: {name}", L.mca_embedding_scatter_add(*b, stream), want))
        out.append((f"det: {name}", L.mca_embedding_scatter_add_det(*b, O["scratch"].data_ptr(), need, stream), want))
    out.append(("det: scratch one float short", L.mca_embedding_scatter_add_det(*a, O["scratch"].data_ptr(), need - 1, stream), BADARG))
    out.append(("det: scratch NULL", L.mca_embedding_scatter_add_det(*a, None, need, stream), BADARG))
    return out


# ================================================================================================ case drivers
# One flow for both files: `launch` is the library on the GPU (tests/test_token_edges_gpu.py) or the fp32 restatement on the CPU
# (tests/test_token_edges_cpu.py: every bound is satisfiable, and the drivers themselves are exercised without a GPU).
def lookup_case(case, device, launch):
    """launch(case, T).  The case's lookup, its second lookup on the same table and marker if it has one, and, where an index is
    out of range, the same call with flag = NULL: nothing else changes"""
    T = lookup_setup(case, device)
    launch(case, T)
    got_w = lookup_check(case, T)
    if case["second"]:
        T2 = lookup_setup(case, device, second=True)
        T2.update(table=T["table"], marker=T["marker"], flag=T["flag"])
        launch(case, T2)
        lookup_check(case, T2, case["name"] + " (second lookup)", w_before=got_w)
    if case["oob"] and case["flag"] and case["tokens"] < 100000:
        quiet = dict(case, flag=0)
        N = lookup_setup(quiet, device)
        launch(quiet, N)
        lookup_check(quiet, N, case["name"] + " (flag NULL)")
        for k in ("table", "dst"):
            assert_bits(N[k].t.cpu(), T[k].t.cpu(), f"{case['name']}: {k} with flag NULL against {k} with a flag")


def grad_case(case, device, launch):
    """launch(case, T, O, det, idx_bytes).  Integer data, then randn; the atomic and the fixed-order form; int64 and int32 indices"""
    for real in (False, True):
        T = grad_setup(case, device, real)
        res = {}
        for det in (False, True):
            for ib in (8, 4):
                O = grad_outputs(case, T, device, det)
                launch(case, T, O, det, ib)
                res[det, ib] = grad_check(case, T, O, det, f"{case['name']} ({'det' if det else 'atomic'}, int{8 * ib}, {'randn' if real else 'integers'})")
        if real:
            O = grad_outputs(case, T, device, True)
            launch(case, T, O, True, 8)
            assert_bits(O["dtable"].t.cpu(), res[True, 8], f"{case['name']}: dtable of a second det run against the first")
            assert_bits(res[True, 4], res[True, 8], f"{case['name']}: det dtable with int32 indices against int64 indices")
