"""PatchEncoder on the GPU: `mca_patch_ln_fwd` through the C ABI, element by element inside NaN frames and sentinel guards
(tests/patch_cases.py: cases, data, float64 references and bounds); the whole step - eager, replayed, deterministic, EAO - against
the plain torch restatement of the encoder registered under another type name (tests/patch_twin.py: it runs through ForeignStep,
the way a matrix modality had to run before); and PatchStep against the reference's own recorded tokens and gradients
(tests/golden/patch_encoder_tiny.pt)."""
import copy
import importlib
import os

import pytest
import torch

import patch_cases as pc
from patch_twin import TWIN, TwinPatchEncoder, patch_config, twin_config
from row_edge_util import WORST
from util_small import GOLDEN, rel_err, small_config, to_device

pytestmark = pytest.mark.gpu
TOKENS_BOUND, GRAD_BOUND = 2.0 ** -6, 8e-2          # bf16 GEMM operands against fp32 torch: the bounds of test_sparse_value_chain_against_torch_twin


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
    return torch.load(os.path.join(GOLDEN, "patch_encoder_tiny.pt"), weights_only=False)


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ the kernel, per element
def launch(H, T, O):
    H.call("mca_patch_ln_fwd", *pc.args(T, O), stream())
    torch.cuda.synchronize()


@pytest.fixture()
def form(H, request):
    H.lib().mca_debug_set(13, pc.FORMS[request.param])
    yield request.param
    H.lib().mca_debug_set(13, 0)


@pytest.mark.parametrize("form", list(pc.FORMS), indirect=True)
@pytest.mark.parametrize("c", pc.CASES, ids=pc.case_id)
def test_kernel_plain_data(H, c, form):
    """statistics and xn_bf16 of every row (the plain data excludes none: cap MAX_EXCLUDED asserted), with xp and without, at a row
    stride of W + 3 (scalar accesses) and W + 4 (16-byte accesses where p2 % 4 == 0)"""
    gen = torch.Generator(device="cuda").manual_seed(5)
    rows = pc.plain_rows(c, gen)
    for extra, with_xp in ((3, True), (3, False), (4, True), (4, False)):
        T, O = pc.setup(c, rows, gen, ldv_extra=extra, with_xp=with_xp)
        launch(H, T, O)
        live, skipped = pc.check(T, O, f"{pc.case_id(c)} {form} plain ldv = W + {extra}{'' if with_xp else ', xp NULL'}", cap=pc.MAX_EXCLUDED)
        assert live > 0
    print({k: round(v, 3) for k, v in WORST.items() if k.startswith("patch_ln")})


@pytest.mark.parametrize("form", list(pc.FORMS), indirect=True)
@pytest.mark.parametrize("c", pc.CASES, ids=pc.case_id)
def test_kernel_special_patches(H, c, form):
    """every row of the case as every kind of patch_cases.KINDS: xp and padmask exact, all-pad rows exact, the rest within bounds"""
    gen = torch.Generator(device="cuda").manual_seed(6)
    for v in range(pc.N_KINDS):
        T, O = pc.setup(c, pc.special_rows(c, v, gen), gen, ldv_extra=3 + v % 2, with_xp=v % 4 < 2)
        launch(H, T, O)
        pc.check(T, O, f"{pc.case_id(c)} {form} special {v}")


def test_kernel_refusals_leave_the_outputs_untouched(H):
    """a host-side check that launches nothing: non-zero return, every sentinel intact"""
    c = (4, 4, 2, 2, 2)
    gen = torch.Generator(device="cuda").manual_seed(7)
    T, O = pc.setup(c, pc.plain_rows(c, gen), gen)
    L = H.lib()
    base = list(pc.args(T, O))
    IDX = dict(H=4, W=5, p1=6, p2=7, ld_bf16=14, cols_pad=15)

    def rc(**kw):
        a = list(base)
        for k, v in kw.items():
            a[IDX[k]] = v
        return L.mca_patch_ln_fwd(*a, stream())
    assert rc(H=9) != 0 and rc(W=9) != 0, "H % p1, W % p2"
    assert rc(H=66, W=64, p1=33, p2=32, cols_pad=1088, ld_bf16=1088) != 0, "P = 33 * 32"
    assert rc(cols_pad=15) != 0, "cols_pad < P"
    torch.cuda.synchronize()
    for k in ("xp", "xn", "mean", "rstd", "mask"):
        t = O[k].t
        it = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
        assert bool((t.contiguous().view(it) == (255 if it == torch.uint8 else -1)).all()), f"{k}: stored to by a refused call"
        pc.assert_guard_intact(O[k], k)
    assert rc() == 0          # the same arguments unchanged are accepted
    torch.cuda.synchronize()
    pc.check(T, O, "accepted call")


# ------------------------------------------------------------------------------------------------ the step against the torch twin
@pytest.fixture()
def twins(P):
    P.encoders_dict[TWIN] = TwinPatchEncoder
    yield
    P.encoders_dict.pop(TWIN, None)


def initial_state(P, cfg):
    """a seeded model's state; the patch encoder's LayerNorm gammas and betas moved off 1 and 0"""
    torch.manual_seed(21)
    sd = {k: v.clone() for k, v in P.build_model(copy.deepcopy(cfg)).state_dict().items()}
    g = torch.Generator().manual_seed(22)
    for k, w in sd.items():
        if k.startswith("encoders.audio.batch_to_tokens.") and (".1." in k or ".3." in k):
            w.add_(0.1 * torch.randn(w.shape, generator=g))
    return sd


def patch_batch(P, cfg, b=4, seed=16):          # (a seed that drops the patch modality of one sample)
    return to_device(P.data.synthetic_batch(cfg, b, seed=seed, p_drop=0.2, lengths="uniform"), "cuda")


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
    return dict(loss=float(out["loss"].detach()), x0=ws["x"][0].clone(), padding=ws["padding"].clone(), out=out,
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
    """audio = PatchEncoder over 40 x 35 matrices whose last rows are padded from a random row on, some samples dropped.  Natively
    the Linear runs bf16 operands, in the twin fp32: the audio rows with mask 0 at 2^-6 rel-L2 (and not bit-equal: two arithmetics),
    every gradient tensor at 8e-2; everything that does not depend on that arithmetic - the padding bytes, the presence bits, the
    packed rows of the other modalities and the fusion tokens - bit-equal.  Measured on an MI355X: docs/parity.md."""
    cfg = patch_config(small_config, variant)
    sd = initial_state(P, cfg)
    batch = patch_batch(P, cfg)
    nat_model, twin_model = build(P, cfg, sd), build(P, twin_config(cfg), sd)
    assert nat_model.engine.can_forward_backward() and not twin_model.engine.can_forward_backward()
    nat, twin = one_step(nat_model, batch), one_step(twin_model, batch)
    eng = nat_model.engine
    N, n, off = eng.N, 70, eng.offsets[0]
    assert torch.equal(nat["padding"], twin["padding"])
    x_n, x_t = nat["x0"].view(4, N, 128), twin["x0"].view(4, N, 128)
    pad = nat["padding"].view(4, N).bool()
    audio = torch.zeros(N, dtype=torch.bool, device="cuda")
    audio[off:off + n] = True
    if variant == "eao":          # (the modality's block is replicated into every combination segment that holds it)
        for src, dst, cnt in eng.st.copies:
            if bool(audio[src]):
                audio[dst:dst + cnt] = True
    assert torch.equal(x_n[:, ~audio], x_t[:, ~audio]), "rows of the other modalities / fusion tokens differ"
    live = ~pad[:, off:off + n]
    masked = int((~live).sum())
    assert 0 < masked < live.numel()
    a_n, a_t = x_n[:, off:off + n], x_t[:, off:off + n]
    assert bool(torch.isfinite(a_n).all()) and bool(torch.isfinite(a_t).all())          # masked rows: finite, not compared further
    d = rel_err(a_n[live], a_t[live])
    print(f"{variant}: audio rows (mask 0) rel-L2 {d:.3e}")
    assert 0 < d <= TOKENS_BOUND, d
    for k in ("audio", "video", "text"):
        assert torch.equal(nat["out"]["modality_sample_mask"][k], twin["out"]["modality_sample_mask"][k]), k
    dropped = (batch["audio"]["values"] == -10000).flatten(1).all(1)
    assert bool(dropped.any()) and torch.equal(nat["out"]["modality_sample_mask"]["audio"], ~dropped)          # presence bit clear
    for name, g in twin["grads"].items():
        e = rel_err(nat["grads"][name], g)
        print(f"{variant}: {name}: rel-L2 {e:.3e}")
        assert e <= GRAD_BOUND, (name, e)
        if name.startswith("encoders.audio."):
            assert float(nat["grads"][name].abs().max()) > 0, name
    assert float(nat["grads"]["encoders.audio.embedding.weight"].abs().max()) > 0


def test_wrong_shape_raises_before_any_launch(P):
    cfg = patch_config(small_config, "mca")
    model = build(P, cfg, initial_state(P, cfg))
    batch = patch_batch(P, cfg)
    hipmod = importlib.import_module("mca-paper_amd.hip")
    steps = importlib.import_module("mca-paper_amd.encoder_steps")
    engine = importlib.import_module("mca-paper_amd.engine")
    batch["audio"]["values"] = batch["audio"]["values"][:, :, :30].contiguous()
    seen, real = [], hipmod.call

    def recording(name, *a, **k):
        seen.append(name)
        return real(name, *a, **k)
    mods = (hipmod, steps, engine)
    try:
        for m in mods:
            m.call = recording
        with pytest.raises(AssertionError, match="60 - 70"), torch.no_grad():
            model(batch, no_loss=True)
    finally:
        for m in mods:
            m.call = real
    assert not {"mca_patch_ln_fwd", "mca_pack_masks", "mca_gemm_nt", "mca_layernorm_fwd"} & set(seen), seen


# ------------------------------------------------------------------------------------------------ the reference's fixture
@pytest.mark.parametrize("i", [0, 1])
def test_patch_step_against_the_reference_fixture(P, gold, i):
    """the reference's weights and batch through a model whose `audio` is the fixture's encoder; the tokens PatchStep.forward packs and
    the parameter gradients PatchStep.backward alone gives for the fixture's upstream gradient, against the REFERENCE's recorded
    values: mask equal, tokens with mask 0 at 2^-6 rel-L2, every gradient at 8e-2"""
    rec = gold["configs"][i]
    D, n, b = rec["config"]["embedding_dim"], rec["config"]["max_tokens"], rec["batch"]["values"].shape[0]
    cfg = small_config("mca")
    cfg.update(dim=D, heads=D // 64)
    for e in cfg["encoder_configs"].values():
        e["embedding_dim"] = D
    cfg["encoder_configs"]["audio"] = copy.deepcopy(rec["config"])
    torch.manual_seed(3)
    model = P.build_model(copy.deepcopy(cfg))
    model.encoders["audio"].load_state_dict(rec["weights"])
    model = model.cuda()
    batch = to_device(P.data.synthetic_batch(cfg, b, seed=4), "cuda")
    batch["audio"] = {"values": rec["batch"]["values"].cuda()}
    with torch.no_grad():
        model(batch, no_loss=True)
    torch.cuda.synchronize()
    eng = model.engine
    ws, step = eng.workspace(b), eng.enc_steps[0]
    assert type(step).__name__ == "PatchStep" and (step.off, step.n) == (eng.offsets[0], n)
    N, off = eng.N, step.off
    mask = ws["padding"].view(b, N)[:, off:off + n].cpu()
    assert torch.equal(mask.to(torch.int64), rec["mask"])
    live = rec["mask"] == 0
    tokens = ws["x"][0].view(b, N, D)[:, off:off + n].cpu()
    assert bool(torch.isfinite(tokens).all())
    d = rel_err(tokens[live], rec["tokens"][live])
    print(f"fixture {i}: tokens (mask 0) rel-L2 {d:.3e}")
    assert 0 < d <= TOKENS_BOUND, d
    eng.gflat.zero_()
    dx = torch.zeros(b * N, D, device="cuda")
    dx.view(b, N, D)[:, off:off + n] = rec["upstream"].cuda()
    step.backward(ws, dx, lambda fn: fn())
    torch.cuda.synchronize()
    params = dict(model.encoders["audio"].named_parameters())
    assert set(params) == set(rec["grads"])
    for k, want in rec["grads"].items():
        got = eng.grad_of(params[k]).cpu()
        e = rel_err(got, want)
        print(f"fixture {i}: {k}: rel-L2 {e:.3e}")
        assert float(got.abs().max()) > 0 and e <= GRAD_BOUND, (k, e)


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
    cfg = patch_config(small_config, "mca")
    sd = initial_state(P, cfg)
    batch = patch_batch(P, cfg)
    rep = graphed(P, cfg, sd, batch, deterministic=False, eager=False)
    eager = one_step(build(P, cfg, sd), batch)
    assert_same_step(dict(loss=rep["loss"], grads=rep["grads"]), eager)
    assert float(rep["grads"]["encoders.audio.embedding.weight"].abs().max()) > 0


def test_deterministic_mode_is_bitwise_eager_and_replayed(P):
    """two eager steps and one replayed step from identical state leave the same bits in the flat gradient buffer (the patch encoder's
    six gradients are in it) and in the weights after FusedAdamW.step()"""
    cfg = patch_config(small_config, "mca")
    sd = initial_state(P, cfg)
    batch = patch_batch(P, cfg)
    a, b, r = (graphed(P, cfg, sd, batch, deterministic=True, eager=e) for e in (True, True, False))
    eng = a["model"].engine
    for name, p in a["model"].named_parameters():
        if name.startswith("encoders.audio."):
            assert float(eng.grad_of(p).abs().max()) > 0, name
    for x, y, what in ((a, b, "eager / eager"), (a, r, "eager / replay")):
        assert torch.equal(x["gflat"], y["gflat"]), what
        assert torch.equal(x["flat"], y["flat"]), what
    assert not torch.equal(a["flat"], build(P, cfg, sd).engine.flat), "the step moved no weight"
