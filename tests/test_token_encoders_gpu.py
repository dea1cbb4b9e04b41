"""SequenceEncoder and SparseTabularEncoder on the GPU: the lookup and table-gradient kernels through the C ABI against torch's own
nn.Embedding(max_norm = 1) arithmetic on the CPU and the reference's fixture (tests/golden/token_encoders_tiny.pt), the
out-of-range guard, and the whole step - eager, replayed, deterministic, EAO - against plain torch restatements of the two
encoders registered under other type names (they run through ForeignStep, the way such a modality ran before)."""
import copy
import importlib
import math
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from util_small import GOLDEN, small_config, rel_err, to_device

pytestmark = pytest.mark.gpu
CASES = [(37, 64, 3, 5), (300, 512, 2, 70)]          # (V, D, b, n)
PATTERNS = ("same", "once", "pad", "last", "mixed")
OOB_BIT = 4


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("mca-paper_amd")


@pytest.fixture(scope="module")
def H(P):
    return importlib.import_module("mca-paper_amd.hip")


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(GOLDEN, "token_encoders_tiny.pt"), weights_only=False)


def stream():
    return torch.cuda.current_stream().cuda_stream


def make_table(V, D, seed):
    """rows at L2 norm 3 (r % 3 == 0), 0.5 (r % 3 == 1) and 0.999 / 1.001 (r % 3 == 2, either side of max_norm); row 0 (padding) zero"""
    w = torch.randn(V, D, generator=torch.Generator().manual_seed(seed))
    r = torch.arange(V)
    want = torch.where(r % 3 == 0, 3.0, torch.where(r % 3 == 1, 0.5, torch.where(r % 2 == 0, 0.999, 1.001)))
    w = w * (want / w.norm(dim=1))[:, None]
    w[0] = 0.0
    return w.contiguous()


def make_indices(pattern, V, b, n, seed):
    g = torch.Generator().manual_seed(seed)
    if pattern == "same":
        return torch.full((b, n), 3, dtype=torch.int64)
    if pattern == "once":
        return torch.randperm(V, generator=g)[: b * n].reshape(b, n).to(torch.int64)          # b * n <= V: every token another row
    if pattern == "pad":
        return torch.zeros(b, n, dtype=torch.int64)
    if pattern == "last":
        return torch.full((b, n), V - 1, dtype=torch.int64)
    idx = torch.randint(0, V, (b, n), generator=g)
    idx[0, :2] = idx[-1, -1]          # repeats across samples
    idx[-1, 0], idx[0, -1] = 0, V - 1
    return idx


def lookup(H, table, V, D, idx, n, add, dst, bstride, accumulate, marker, flag=None):
    H.call("mca_embedding_lookup", table.data_ptr(), V, D, 1.0, idx.data_ptr(), idx.element_size(), idx.numel(), n, H.ptr(add),
           dst.data_ptr(), D, bstride, int(accumulate), marker.data_ptr(), H.ptr(flag), OOB_BIT, stream())
    torch.cuda.synchronize()


def scatter(H, det, dy, bstride, n, idx, dtable, V, D, pad, scratch_floats=None):
    """-> return code (the plain form raises through H.call on an error)"""
    L = H.lib()
    args = (dy.data_ptr(), D, bstride, n, idx.data_ptr(), idx.element_size(), idx.numel(), dtable.data_ptr(), V, D, pad)
    if not det:
        H.call("mca_embedding_scatter_add", *args, stream())
        rc = 0
    else:
        need = L.mca_embedding_scatter_add_det_scratch(idx.numel()) if scratch_floats is None else scratch_floats
        s = torch.full((max(need, 1),), float("nan"), device="cuda")          # (the scratch needs no zeroing)
        rc = L.mca_embedding_scatter_add_det(*args, s.data_ptr(), need, stream())
    torch.cuda.synchronize()
    return rc


def rescale_tol(D):
    """the only difference to torch's renormalisation is the summation order of D squares under a square root"""
    return (D + 8) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ lookup forward
@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("idt", [torch.int64, torch.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("V,D,b,n", CASES)
def test_lookup_forward(H, V, D, b, n, idt, with_add, accumulate):
    tol = rescale_tol(D)
    add = torch.randn(n, D, generator=torch.Generator().manual_seed(5)) if with_add else None
    marker = torch.zeros(V, dtype=torch.int32, device="cuda")
    for pi, pattern in enumerate(PATTERNS):
        w0 = make_table(V, D, 100 + pi)
        idx = make_indices(pattern, V, b, n, 200 + pi)
        dst0 = torch.randn(b, n + 3, D, generator=torch.Generator().manual_seed(300 + pi))          # rows n .. n + 2 of a sample: sentinels
        # torch's own arithmetic on the CPU: the rows after the in-place renormalisation, and the table it leaves
        w_want = w0.clone()
        e_want = F.embedding(idx, w_want, padding_idx=0, max_norm=1.0)
        table, dst = w0.cuda(), dst0.cuda()
        lookup(H, table, V, D, idx.to(idt).cuda(), n, add.cuda() if with_add else None, dst, (n + 3) * D, accumulate, marker)
        got_w, got = table.cpu(), dst.cpu()
        assert int(marker.abs().sum()) == 0, pattern
        touched = torch.zeros(V, dtype=torch.bool); touched[idx.reshape(-1)] = True
        rescaled = touched & (w0.norm(dim=1) > 1.0)
        assert bool(rescaled.any()) or pattern == "pad"
        # the table: untouched rows and rows within max_norm keep their bits; rescaled rows within the bound, each once
        assert torch.equal(got_w[~rescaled], w0[~rescaled]), pattern
        assert torch.equal(w_want[~rescaled], w0[~rescaled])
        assert bool(((got_w[rescaled] - w_want[rescaled]).abs() <= tol * w_want[rescaled].abs()).all()), pattern
        assert bool((got_w[rescaled].norm(dim=1) <= 1.0 + 1e-6).all()) and bool((got_w[rescaled].norm(dim=1) > 0.999).all())
        # the output: exactly dst (=|+=) (row + add) of the table the kernels left, every fp32 add correctly rounded on both sides
        def compose(e):
            t = e + add[None] if with_add else e
            return dst0[:, :n] + t if accumulate else t
        assert torch.equal(got[:, :n], compose(got_w[idx])), pattern
        assert torch.equal(got[:, n:], dst0[:, n:]), f"{pattern}: sentinel rows written"
        # ... and against torch: bit-equal where no row was rescaled, within the bound (+ the roundings of the adds) where one was
        want = compose(e_want)
        tok_rescaled = rescaled[idx]
        assert torch.equal(got[:, :n][~tok_rescaled], want[~tok_rescaled]), pattern
        t_want = e_want + add[None] if with_add else e_want
        bound = tol * e_want.abs() + (2.0 ** -23 * (t_want.abs() + want.abs()) if (with_add or accumulate) else 0.0)
        assert bool(((got[:, :n] - want).abs() <= bound)[tok_rescaled].all()), pattern


def test_lookup_forward_reference_fixture(H, gold):
    """the reference's SequenceEncoder output and the table it leaves (V = 37, D = 128, b = 3, n = 9)"""
    rec = gold["SequenceEncoder"]
    V, D = rec["table_in"].shape
    idx, (b, n) = rec["batch"]["tokens"], rec["batch"]["tokens"].shape
    table, dst = rec["table_in"].cuda(), torch.zeros(b, n, D, device="cuda")
    marker = torch.zeros(V, dtype=torch.int32, device="cuda")
    lookup(H, table, V, D, idx.cuda(), n, rec["init"]["positional_encoder.pe"].cuda(), dst, n * D, False, marker)
    tol = rescale_tol(D)
    touched = torch.zeros(V, dtype=torch.bool); touched[idx.reshape(-1)] = True
    rescaled = touched & (rec["table_in"].norm(dim=1) > 1.0)
    assert int(rescaled.sum()) >= 3 and int((touched & ~rescaled).sum()) >= 3 and int(marker.abs().sum()) == 0
    got_w, got = table.cpu(), dst.cpu()
    assert torch.equal(got_w[~rescaled], rec["table_out"][~rescaled]) and torch.equal(got_w[~rescaled], rec["table_in"][~rescaled])
    assert bool(((got_w[rescaled] - rec["table_out"][rescaled]).abs() <= tol * rec["table_out"][rescaled].abs()).all())
    tok = rescaled[idx]
    assert torch.equal(got[~tok], rec["tokens"][~tok])
    e = rec["table_out"][idx]
    assert bool(((got - rec["tokens"]).abs() <= tol * e.abs() + 2.0 ** -23 * rec["tokens"].abs())[tok].all())
    assert torch.equal(rec["mask"], rec["batch"]["attention_mask"])          # the mask is handed through


def test_lookup_argument_checks(H):
    L = H.lib()
    t, d = torch.zeros(8, 64, device="cuda"), torch.zeros(4, 64, device="cuda")
    i, m = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    ok = lambda **k: L.mca_embedding_lookup(t.data_ptr(), 8, k.get("cols", 64), 1.0, i.data_ptr(), k.get("ib", 8), 4, k.get("period", 4), None,
                                            d.data_ptr() + k.get("off", 0), k.get("ldd", 64), 256, 0, k.get("marker", m.data_ptr()), None, 0, stream())
    assert ok() == 0
    assert ok(ib=2) == -1 and ok(period=0) == -1 and ok(marker=None) == -1
    assert ok(cols=62) == -2 and ok(ldd=66) == -2 and ok(off=4) == -2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ out-of-range guard
@pytest.mark.parametrize("idt", [torch.int64, torch.int32], ids=["i64", "i32"])
def test_out_of_range_indices_are_never_dereferenced(H, idt):
    """The table (and its gradient) sit in the middle of a larger allocation of the test's own, so that a kernel that did turn -1 or
    V into an address would still read and write the test's memory - and be seen in the guard rows."""
    V, D, b, n, G = 37, 64, 2, 6, 4
    big = torch.randn(G + V + G, D, generator=torch.Generator().manual_seed(1))
    big[G:] = big[G:] * (0.5 / big[G:].norm(dim=1))[:, None]          # table rows (and the guard behind) at norm 0.5; the guard in front random
    big[:G] *= 3.0
    idx = torch.tensor([[1, -1, 2, V, 3, 0], [V, 4, -1, 5, V - 1, 1]], dtype=torch.int64)
    bad = (idx < 0) | (idx >= V)
    add = torch.randn(n, D, generator=torch.Generator().manual_seed(2))
    dbig, flag = big.cuda(), torch.zeros(1, dtype=torch.int32, device="cuda")
    dst = torch.full((b, n, D), 7.5, device="cuda")
    marker = torch.zeros(V, dtype=torch.int32, device="cuda")
    didx = idx.to(idt).cuda()
    lookup(H, dbig[G:], V, D, didx, n, add.cuda(), dst, n * D, False, marker, flag)
    assert int(flag) == OOB_BIT and int(marker.abs().sum()) == 0
    assert torch.equal(dbig.cpu(), big)          # guards and table bit-unchanged (no row is above max_norm)
    got = dst.cpu()
    assert torch.equal(got[bad], add[None].expand(b, n, D)[bad])          # the add part alone
    assert torch.equal(got[~bad], (big[G:][idx.clamp(0, V - 1)] + add[None])[~bad])
    flag.zero_()
    lookup(H, dbig[G:], V, D, idx.clamp(0, V - 1).to(idt).cuda(), n, None, dst, n * D, True, marker, flag)
    assert int(flag) == 0          # in range: the bit stays clear
    # the table gradient: those tokens contribute nothing, in either form
    dy = torch.randn(b, n, D, generator=torch.Generator().manual_seed(3))
    g0 = torch.randn(G + V + G, D, generator=torch.Generator().manual_seed(4))
    keep = ~bad & (idx != 0)
    want = g0.double()
    want[G:].index_add_(0, idx[keep], dy[keep].double())
    cnt = torch.zeros(G + V + G).index_add_(0, idx[keep] + G, torch.ones(int(keep.sum())))
    mag = g0.abs().double()
    mag[G:].index_add_(0, idx[keep], dy[keep].abs().double())
    for det in (False, True):
        dg = g0.cuda()
        assert scatter(H, det, dy.cuda(), n * D, n, didx, dg[G:], V, D, 0) == 0
        got = dg.cpu()
        assert torch.equal(got[cnt == 0], g0[cnt == 0]), det          # guards, the padding row, rows no valid token names
        assert bool(((got.double() - want).abs() <= cnt[:, None] * 2.0 ** -24 * mag).all()), det


def token_config(variant="mca"):
    cfg = small_config(variant)
    enc = cfg["encoder_configs"]
    enc["text"] = {"type": "SequenceEncoder", "num_embeddings": 37, "max_tokens": 30, "embedding_dim": 128}
    if variant == "mca":
        enc["video"] = {"type": "SparseTabularEncoder", "num_embeddings": 23, "max_tokens": 45, "max_value": 100, "embedding_dim": 128}
    return cfg


def token_batch(P, cfg, values=True, seed=9):
    """b = 4; sample 1 has no text (all pad), sample 2 no video; values=False: the sparse encoder's data column is 0.0 everywhere"""
    batch = P.data.synthetic_batch(cfg, 4, seed=seed)
    t = batch["text"]
    t["tokens"][1] = 0
    t["tokens"][0, :3] = t["tokens"][3, 0]          # one row named by several tokens and samples
    t["attention_mask"] = (t["tokens"] == 0).to(torch.long)
    v = batch["video"]
    if "indices" in v:
        v["indices"][2] = 0
        v["data"][2] = 0.0
        v["data"][0, 0] = 250.0          # above max_value
        if not values:
            v["data"].zero_()
        v["attention_mask"] = (v["indices"] == 0).to(torch.long)
    return to_device(batch, "cuda")


def test_engine_raises_index_error_and_skips_the_update(P):
    optim = importlib.import_module("mca-paper_amd.optim")
    cfg = token_config()
    torch.manual_seed(3)
    model = P.build_model(copy.deepcopy(cfg)).cuda()
    batch = token_batch(P, cfg)
    model(batch)          # in range: nothing raised
    batch["text"]["tokens"][0, 4], batch["text"]["tokens"][3, 1] = 37, -1
    with pytest.raises(IndexError, match="outside"):
        model(batch)          # check_finite = True: raised inside the forward that saw it
    eng = model.engine
    assert int(eng.finite_flag) == 0
    eng.check_finite = "deferred"
    opt = optim.FusedAdamW(model, lr=1e-2)
    before = eng.flat.clone()
    table0 = model.encoders["text"].token_encoder.embedding.weight.detach().clone()
    out = model(batch); opt.zero_grad(); out["loss"].backward(); opt.step()
    torch.cuda.synchronize()
    after = eng.flat.clone()
    # (the forward may renormalise looked-up rows of the tables in place; AdamW itself moved nothing)
    table1 = model.encoders["text"].token_encoder.embedding.weight.detach()
    renormed = (table1 != table0).any(1)
    assert bool((table0[renormed].norm(dim=1) > 1.0).all())
    n_same = int((after == before).sum())
    assert n_same >= before.numel() - 128 * (37 + 23), "a flagged step reached the weights"
    assert bool(torch.isfinite(out["loss"]))
    with pytest.raises(IndexError, match="outside"):
        eng.assert_finite()
    eng.assert_finite()          # the flag was cleared by the raise


# ------------------------------------------------------------------------------------------------ scatter-add
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("idt", [torch.int64, torch.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("V,D,b,n", CASES + [(37, 64, 4, 150)])          # (600 tokens: the "mixed" pattern of this case names 3 rows)
def test_scatter_add(H, V, D, b, n, idt, det):
    for pi, pattern in enumerate(PATTERNS):
        if pattern == "once" and b * n > V:
            continue
        idx = make_indices(pattern, V, b, n, 400 + pi)
        if n == 150 and pattern == "mixed":
            idx = torch.tensor([2, V - 1, 7])[torch.randint(0, 3, (b, n), generator=torch.Generator().manual_seed(6))]
            assert idx.numel() == 600 and len(idx.unique()) == 3
        dy = torch.randn(b, n + 3, D, generator=torch.Generator().manual_seed(500 + pi))          # the packed layout: a sample is n + 3 rows
        g0 = torch.randn(V, D, generator=torch.Generator().manual_seed(600 + pi))
        keep = idx != 0
        contrib = dy[:, :n][keep]
        want = g0.double().index_add_(0, idx[keep], contrib.double())
        mag = g0.abs().double().index_add_(0, idx[keep], contrib.abs().double())
        k = torch.zeros(V).index_add_(0, idx[keep], torch.ones(int(keep.sum())))
        ddy, didx = dy.cuda(), idx.to(idt).cuda()
        runs = []
        for _ in range(2 if det else 1):
            dg = g0.cuda()
            assert scatter(H, det, ddy, (n + 3) * D, n, didx, dg, V, D, 0) == 0
            runs.append(dg.cpu())
        got = runs[0]
        assert torch.equal(got[0], g0[0]), f"{pattern}: the padding_idx row moved"
        assert torch.equal(got[k == 0], g0[k == 0]), pattern
        err = (got.double() - want).abs()
        assert bool((err <= k[:, None] * 2.0 ** -24 * mag).all()), (pattern, float((err / (mag * 2.0 ** -24)).max()))
        if pattern not in ("pad",):
            assert float((got - g0).abs().max()) > 0
        if det:
            assert torch.equal(runs[0], runs[1]), f"{pattern}: two launches differ"
            dg = g0.cuda()
            need = H.lib().mca_embedding_scatter_add_det_scratch(idx.numel())
            assert scatter(H, True, ddy, (n + 3) * D, n, didx, dg, V, D, 0, scratch_floats=need - 1) == -1          # MCA_E_BADARG
            assert torch.equal(dg.cpu(), g0), "a launch with too small a scratch wrote"


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("t", ["SequenceEncoder", "SparseTabularEncoder"])
def test_scatter_add_reference_fixture(H, gold, t, det):
    """the reference's table gradient for its stored upstream gradient; both sides are within k * 2^-24 * sum |g| of the exact sum"""
    rec = gold[t]
    idx = rec["batch"]["tokens" if t == "SequenceEncoder" else "indices"]
    V, D = rec["table_in"].shape
    n = idx.shape[1]
    want = rec["grads"]["token_encoder.embedding.weight"]
    dg = torch.zeros(V, D, device="cuda")
    assert scatter(H, det, rec["upstream"].cuda(), n * D, n, idx.cuda(), dg, V, D, 0) == 0
    keep = idx != 0
    k = torch.zeros(V).index_add_(0, idx[keep], torch.ones(int(keep.sum())))
    mag = torch.zeros(V, D, dtype=torch.float64).index_add_(0, idx[keep], rec["upstream"][keep].abs().double())
    got = dg.cpu()
    assert bool(((got.double() - want.double()).abs() <= 2 * k[:, None] * 2.0 ** -24 * mag).all())
    assert float(got[0].abs().sum()) == 0.0 and float(want[0].abs().sum()) == 0.0 and float(got.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ whole step against torch twins
def _holder(**mods):
    return nn.ModuleDict(mods)


class TwinSequenceEncoder(nn.Module):
    """encoders.py:145-166 restated: nn.Embedding(max_norm = 1) + the sinusoidal table; the mask handed through"""

    def __init__(self, num_embeddings=36602, embedding_dim=512, padding_idx=0, dropout=0.0, max_tokens=1024, **kwargs):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.token_encoder = _holder(embedding=nn.Embedding(num_embeddings, embedding_dim, padding_idx=padding_idx, max_norm=1.0))
        pos = torch.arange(max_tokens, dtype=torch.float32).unsqueeze(1)
        freq = torch.exp(torch.arange(0, embedding_dim, 2) * (-math.log(10000.0) / embedding_dim))
        pe = torch.zeros(max_tokens, embedding_dim)
        pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * freq), torch.cos(pos * freq)
        self.positional_encoder = nn.Module()
        self.positional_encoder.register_buffer("pe", pe)

    def forward(self, batch):
        x = self.token_encoder["embedding"](batch["tokens"].to(torch.int64))
        return x + self.positional_encoder.pe[: x.shape[1]], batch["attention_mask"]


class TwinSparseTabularEncoder(nn.Module):
    """encoders.py:40-72, 100-120 restated: nn.Embedding(max_norm = 1) + the value MLP, zero where data == padding_idx"""

    def __init__(self, num_embeddings=36602, embedding_dim=512, padding_idx=0, dropout=0.0, max_value=10000, **kwargs):
        super().__init__()
        self.embedding_dim, self.max_value, self.padding_value = embedding_dim, max_value, padding_idx
        self.token_encoder = _holder(embedding=nn.Embedding(num_embeddings, embedding_dim, padding_idx=padding_idx, max_norm=1.0))
        self.value_encoder = _holder(linear1=nn.Linear(1, embedding_dim), linear2=nn.Linear(embedding_dim, embedding_dim),
                                     norm=nn.LayerNorm(embedding_dim))

    def forward(self, batch):
        ve = self.value_encoder
        x = batch["data"].unsqueeze(-1)
        pad = x == self.padding_value
        x = ve["norm"](ve["linear2"](torch.relu(ve["linear1"](torch.clamp(x, max=self.max_value)))))
        x = x.masked_fill(pad, 0.0)
        return self.token_encoder["embedding"](batch["indices"].to(torch.int64)) + x, batch["attention_mask"]


TWINS = {"SequenceEncoder": ("TwinSequenceEncoder", TwinSequenceEncoder),
         "SparseTabularEncoder": ("TwinSparseTabularEncoder", TwinSparseTabularEncoder)}


@pytest.fixture()
def twins(P):
    for name, cls in TWINS.values():
        P.encoders_dict[name] = cls
    yield
    for name, _ in TWINS.values():
        P.encoders_dict.pop(name, None)


def twin_config(cfg):
    c = copy.deepcopy(cfg)
    for e in c["encoder_configs"].values():
        if e["type"] in TWINS:
            e["type"] = TWINS[e["type"]][0]
    return c


def initial_state(P, cfg, norm):
    """a seeded model's state with every table row at L2 norm `norm` (a float, or (lo, hi) for uniform in that range); the padding row zero"""
    torch.manual_seed(21)
    sd = {k: v.clone() for k, v in P.build_model(copy.deepcopy(cfg)).state_dict().items()}
    g = torch.Generator().manual_seed(22)
    for k, w in sd.items():
        if k.endswith("token_encoder.embedding.weight") and cfg["encoder_configs"][k.split(".")[1]]["type"] in TWINS:
            want = torch.full((w.shape[0],), float(norm)) if not isinstance(norm, tuple) else torch.rand(w.shape[0], generator=g) * (norm[1] - norm[0]) + norm[0]
            w.mul_((want / w.norm(dim=1).clamp(min=1e-12))[:, None])
            w[0] = 0.0
    return sd


def build(P, cfg, sd, deterministic=False, check_finite=True):
    model = P.build_model(copy.deepcopy(cfg))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not [k for k in missing if k.startswith("encoders.")] and not [k for k in unexpected if k.startswith("encoders.")]
    model = model.cuda()
    model.engine.check_finite = check_finite
    model.engine.set_deterministic(deterministic)
    return model


def one_step(model, batch):
    for p in model.parameters():
        p.grad = None
    out = model(batch)
    out["loss"].backward()
    torch.cuda.synchronize()
    ws = model.engine.workspace(4)
    return dict(loss=float(out["loss"]), x0=ws["x"][0].clone(), padding=ws["padding"].clone(),
                grads={n: p.grad.detach().clone() for n, p in model.named_parameters()})


def assert_same_step(nat, twin, grad_tol=5e-3, loss_tol=1e-6):
    """the project's bounds for one step run two ways from identical state (replayed-vs-eager): loss 1e-6 relative, every gradient
    tensor 5e-3 rel-L2 (the weight gradients are sums of fp32 atomics)"""
    assert abs(nat["loss"] - twin["loss"]) <= loss_tol * abs(twin["loss"]), (nat["loss"], twin["loss"])
    assert set(nat["grads"]) == set(twin["grads"])
    for n, g in twin["grads"].items():
        d = rel_err(nat["grads"][n], g)
        assert d <= grad_tol, (n, d)


@pytest.mark.parametrize("variant", ["mca", "eao"])
def test_step_matches_torch_twin(P, twins, variant):
    """audio = EmbeddedSequenceEncoder, text = SequenceEncoder, video = SparseTabularEncoder (MCA; EAO: text only), table rows at
    norm <= 0.9 so that nothing is rescaled.  The sparse encoder's data column is 0.0 here: its value part is then exactly zero on
    both sides and the two models are the same arithmetic (the value MLP with real values runs bf16 GEMM operands natively and
    fp32 in torch: test_sparse_value_chain_against_torch_twin holds that to the bounds of that difference)."""
    cfg = token_config(variant)
    sd = initial_state(P, cfg, (0.3, 0.9))
    batch = token_batch(P, cfg, values=False)
    nat = one_step(build(P, cfg, sd), batch)
    twin_model = build(P, twin_config(cfg), sd)
    assert not twin_model.engine.can_forward_backward()          # the twins run through ForeignStep
    twin = one_step(twin_model, batch)
    assert torch.equal(nat["x0"], twin["x0"]), "packed tokens differ"
    assert torch.equal(nat["padding"], twin["padding"])
    assert float(nat["grads"]["encoders.text.token_encoder.embedding.weight"].abs().max()) > 0
    assert_same_step(nat, twin)
    for n, g in nat["grads"].items():
        if n.endswith("token_encoder.embedding.weight"):
            assert float(g[0].abs().sum()) == 0.0, f"{n}: the padding row received a gradient"


def test_step_rescales_looked_up_rows_like_torch(P, twins):
    """every table row at norm 3: after one forward the rows the batch names are rescaled as the twin's nn.Embedding rescaled them,
    the others keep their bits"""
    cfg = token_config()
    sd = initial_state(P, cfg, 3.0)
    batch = token_batch(P, cfg, values=False)
    for mod, key, top in (("text", "tokens", 30), ("video", "indices", 15)):          # rows above `top` stay untouched
        t = batch[mod][key]
        batch[mod][key] = torch.where(t > top, t - 7, t)
    models = [build(P, c, sd) for c in (cfg, twin_config(cfg))]
    for m in models:
        with torch.no_grad():
            m(batch, no_loss=True)
    torch.cuda.synchronize()
    for mod, key in (("text", "tokens"), ("video", "indices")):
        k = f"encoders.{mod}.token_encoder.embedding.weight"
        nat, twin = (dict(m.named_parameters())[k].detach().cpu() for m in models)
        touched = torch.zeros(nat.shape[0], dtype=torch.bool); touched[batch[mod][key].reshape(-1).cpu()] = True
        touched[0] = False          # (the zero padding row is looked up and stays zero)
        assert 0 < int(touched.sum()) < nat.shape[0] - 1
        assert torch.equal(nat[~touched], sd[k][~touched]) and torch.equal(twin[~touched], sd[k][~touched]), k
        assert bool(((nat[touched] - twin[touched]).abs() <= rescale_tol(128) * twin[touched].abs()).all()), k
        assert bool(((nat[touched].norm(dim=1) - 1.0).abs() < 1e-5).all()), k


def test_sparse_value_chain_against_torch_twin(P, twins):
    """Real values in the sparse encoder's data column.  Natively the value MLP is TabularStep's chain (bf16 GEMM operands), in the
    twin it is fp32 torch, so only the table part of the video rows is the same arithmetic.  Bounds: every other row of the packed
    tokens and the padding bytes bit-equal; a video row = table row + LayerNorm output, the LayerNorm's input a 128-term product of
    operands rounded to bf16 (relative 2^-9 each, so 2^-8 per term): 2^-6 rel-L2 over the block leaves a factor 4 for the
    LayerNorm's division by the row's deviation; gradients at 8e-2 rel-L2, the bound test_engine_gpu holds a torch encoder against
    its native form to (bf16 operands against fp32 under the temperature-14 loss).  Measured on an MI355X: video rows 2.3e-3, gradients
    5e-3 to 5.1e-2 (the largest: the video table's)."""
    cfg = token_config()
    sd = initial_state(P, cfg, (0.3, 0.9))
    batch = token_batch(P, cfg, values=True)
    nat, twin = one_step(build(P, cfg, sd), batch), one_step(build(P, twin_config(cfg), sd), batch)
    x_n, x_t = nat["x0"].view(4, 153, 128), twin["x0"].view(4, 153, 128)
    video = slice(70, 115)
    other = torch.ones(153, dtype=torch.bool); other[video] = False
    assert torch.equal(x_n[:, other], x_t[:, other]) and torch.equal(nat["padding"], twin["padding"])
    zero_value = (batch["video"]["data"] == 0.0)
    assert torch.equal(x_n[:, video][zero_value], x_t[:, video][zero_value])          # value part masked: the table row alone
    d = rel_err(x_n[:, video], x_t[:, video])
    print(f"video rows rel-L2 {d:.3e}")
    assert 0 < d <= 2.0 ** -6, d
    for n, g in twin["grads"].items():
        e = rel_err(nat["grads"][n], g)
        print(f"{n}: rel-L2 {e:.3e}")
        assert e <= 8e-2, (n, e)
        if n.startswith("encoders.video."):
            assert float(nat["grads"][n].abs().max()) > 0, n


# ------------------------------------------------------------------------------------------------ graph replay, deterministic mode
def graphed(P, cfg, sd, batch, deterministic, eager):
    graph = importlib.import_module("mca-paper_amd.graph")
    optim = importlib.import_module("mca-paper_amd.optim")
    model = build(P, cfg, sd, deterministic=deterministic, check_finite="deferred")
    opt = optim.FusedAdamW(model, lr=1e-3)
    g = graph.GraphedStep(model, opt, batch, clip=2.0)
    assert g.direct          # native encoders: forward_backward, no autograd node
    g.step(batch, eager=eager)
    torch.cuda.synchronize()
    model.engine.assert_finite()
    eng = model.engine
    res = dict(loss=float(g.loss) if not eager else None, gflat=eng.gflat.clone(), flat=eng.flat.clone(), model=model,
               grads={n: eng.grad_of(p).clone() for n, p in model.named_parameters()})
    del g
    return res


def test_graph_replay_matches_eager_step(P):
    cfg = token_config()
    sd = initial_state(P, cfg, (0.3, 0.9))
    batch = token_batch(P, cfg, values=True)
    rep = graphed(P, cfg, sd, batch, deterministic=False, eager=False)
    eager = one_step(build(P, cfg, sd), batch)
    assert_same_step(dict(loss=rep["loss"], grads=rep["grads"]), eager)
    assert float(rep["grads"]["encoders.video.token_encoder.embedding.weight"].abs().max()) > 0


def test_deterministic_mode_is_bitwise_eager_and_replayed(P):
    """table rows at norm 3 (the rescale runs inside the step), real values: two eager steps and one replayed step from identical
    state leave the same bits in the flat gradient buffer (the table gradients are in it) and in the weights after FusedAdamW.step()"""
    cfg = token_config()
    sd = initial_state(P, cfg, 3.0)
    batch = token_batch(P, cfg, values=True)
    a, b, r = (graphed(P, cfg, sd, batch, deterministic=True, eager=e) for e in (True, True, False))
    eng = a["model"].engine
    for name, p in a["model"].named_parameters():
        if name.endswith("token_encoder.embedding.weight"):
            assert float(eng.grad_of(p).abs().max()) > 0, name
    for x, y, what in ((a, b, "eager / eager"), (a, r, "eager / replay")):
        assert torch.equal(x["gflat"], y["gflat"]), what
        assert torch.equal(x["flat"], y["flat"]), what
    assert not torch.equal(a["flat"], build(P, cfg, sd).engine.flat), "the step moved no weight"
