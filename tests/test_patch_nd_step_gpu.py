"""ImagePatchEncoder / VideoPatchEncoder in the fused step, on the GPU: the whole step - eager, replayed, deterministic, EAO - against
the plain torch restatement of the encoder registered under another type name (tests/patch_nd_twin.py: it runs through ForeignStep,
the way an image or video modality had to run before), and PatchNDStep against what the reference's own modules recorded
(tests/golden/patch_encoder_nd_tiny.pt).  The bounds are those of tests/test_patch_encoder_gpu.py: behind the front-end kernel
(tests/test_patch_nd_gpu.py) the arithmetic is the same launches."""
import copy
import importlib
import os

import pytest
import torch

from patch_nd_twin import ND_CFG, TWIN_CLASSES, nd_config, reference_tokens, twin_config
from util_small import GOLDEN, rel_err, small_config, to_device

pytestmark = pytest.mark.gpu
TOKENS_BOUND, GRAD_BOUND = 2.0 ** -6, 8e-2          # bf16 GEMM operands against fp32 torch: the bounds of test_patch_encoder_gpu.py::test_step_matches_torch_twin
MODES = {"image": "ImagePatchEncoder", "video": "VideoPatchEncoder"}


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("mca-paper_amd")


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(GOLDEN, "patch_encoder_nd_tiny.pt"), weights_only=False)


@pytest.fixture()
def twins(P):
    P.encoders_dict.update(TWIN_CLASSES)
    yield
    for k in TWIN_CLASSES:
        P.encoders_dict.pop(k, None)


def initial_state(P, cfg):
    """a seeded model's state; the patch encoder's LayerNorm gammas and betas moved off 1 and 0"""
    torch.manual_seed(21)
    sd = {k: v.clone() for k, v in P.build_model(copy.deepcopy(cfg)).state_dict().items()}
    g = torch.Generator().manual_seed(22)
    for k, w in sd.items():
        if k.startswith("encoders.audio.batch_to_tokens.") and (".1." in k or ".3." in k):
            w.add_(0.1 * torch.randn(w.shape, generator=g))
    return sd


def nd_batch(P, cfg, b=4, seed=16):          # (a seed that drops the patch modality of one sample)
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


@pytest.mark.parametrize("variant", ["mca", "eao"])
@pytest.mark.parametrize("mode", list(MODES))
def test_step_matches_torch_twin(P, twins, mode, variant):
    """audio = 3 x 8 x 15 images in (4, 5) patches / 2 x 4 x 8 x 10 clips in (2, 4, 5) patches, a random tail of rows / frames padded,
    one sample's modality dropped.  Natively the Linear runs bf16 operands, in the twin fp32: the audio rows with mask 0 at 2^-6 rel-L2
    (and not bit-equal: two arithmetics), every gradient tensor at 8e-2; everything that does not depend on that arithmetic - the
    padding bytes, the presence bits, the packed rows of the other modalities and the fusion tokens - bit-equal.  Measured on an
    MI355X: docs/parity.md."""
    cfg = nd_config(small_config, variant, mode)
    sd = initial_state(P, cfg)
    batch = nd_batch(P, cfg)
    nat_model, twin_model = build(P, cfg, sd), build(P, twin_config(cfg), sd)
    assert nat_model.engine.can_forward_backward() and not twin_model.engine.can_forward_backward()
    assert type(nat_model.engine.enc_steps[0]).__name__ == "PatchNDStep" and type(twin_model.engine.enc_steps[0]).__name__ == "ForeignStep"
    nat, twin = one_step(nat_model, batch), one_step(twin_model, batch)
    eng = nat_model.engine
    N, n, off = eng.N, ND_CFG[mode]["max_tokens"], eng.offsets[0]
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
    print(f"{mode} {variant}: audio rows (mask 0) rel-L2 {d:.3e}")
    assert 0 < d <= TOKENS_BOUND, d
    for k in ("audio", "video", "text"):
        assert torch.equal(nat["out"]["modality_sample_mask"][k], twin["out"]["modality_sample_mask"][k]), k
    dropped = (batch["audio"]["values"] == -10000).flatten(1).all(1)
    assert int(dropped.sum()) == 1 and torch.equal(nat["out"]["modality_sample_mask"]["audio"], ~dropped)          # presence bit clear
    worst = 0.0
    for name, g in twin["grads"].items():
        e = rel_err(nat["grads"][name], g)
        worst = max(worst, e)
        if name.startswith("encoders.audio."):
            print(f"{mode} {variant}: {name}: rel-L2 {e:.3e}")
            assert float(nat["grads"][name].abs().max()) > 0, name
        assert e <= GRAD_BOUND, (name, e)
    print(f"{mode} {variant}: largest gradient rel-L2 {worst:.3e}")
    assert float(nat["grads"]["encoders.audio.embedding.weight"].abs().max()) > 0


@pytest.mark.parametrize("mode", list(MODES))
def test_wrong_shape_raises_before_any_launch(P, mode):
    cfg = nd_config(small_config, "mca", mode)
    model = build(P, cfg, initial_state(P, cfg))
    batch = nd_batch(P, cfg)
    hipmod = importlib.import_module("mca-paper_amd.hip")
    steps = importlib.import_module("mca-paper_amd.encoder_steps")
    engine = importlib.import_module("mca-paper_amd.engine")
    batch["audio"]["values"] = batch["audio"]["values"][..., :10 if mode == "image" else 5].contiguous()          # one patch column fewer
    grid = {"image": 4, "video": 4}[mode]
    n = ND_CFG[mode]["max_tokens"]
    seen, real = [], hipmod.call

    def recording(name, *a, **k):
        seen.append(name)
        return real(name, *a, **k)
    mods = (hipmod, steps, engine)
    try:
        for m in mods:
            m.call = recording
        with pytest.raises(AssertionError, match=f"^{grid} - {n}$"), torch.no_grad():
            model(batch, no_loss=True)
    finally:
        for m in mods:
            m.call = real
    assert not {"mca_patch_nd_ln_fwd", "mca_patch_ln_fwd", "mca_pack_masks", "mca_gemm_nt", "mca_layernorm_fwd"} & set(seen), seen


# ------------------------------------------------------------------------------------------------ the reference's fixture
@pytest.mark.parametrize("mode", list(MODES))
def test_step_against_the_reference_fixture(P, gold, mode):
    """the fixture's weights and batch through a model whose `audio` is the fixture's encoder; the tokens the step packs and the
    parameter gradients PatchStep.backward alone gives for the fixture's upstream gradient, against what the REFERENCE's own modules
    recorded (batch_to_tokens + the position table, grid axes flattened): mask equal, tokens with mask 0 at 2^-6 rel-L2, every gradient
    at 8e-2"""
    rec = gold[mode]
    D, n, b = rec["config"]["embedding_dim"], rec["config"]["max_tokens"], rec["batch"]["values"].shape[0]
    weights = dict(rec["init"], **rec["ln"])
    want, upstream = reference_tokens(rec)
    cfg = small_config("mca")
    assert cfg["dim"] == D
    cfg["encoder_configs"]["audio"] = copy.deepcopy(rec["config"])
    torch.manual_seed(3)
    model = P.build_model(copy.deepcopy(cfg))
    model.encoders["audio"].load_state_dict(weights)
    model = model.cuda()
    batch = to_device(P.data.synthetic_batch(cfg, b, seed=4), "cuda")
    batch["audio"] = {"values": rec["batch"]["values"].cuda()}
    with torch.no_grad():
        model(batch, no_loss=True)
    torch.cuda.synchronize()
    eng = model.engine
    ws, step = eng.workspace(b), eng.enc_steps[0]
    assert type(step).__name__ == "PatchNDStep" and (step.off, step.n) == (eng.offsets[0], n)
    N, off = eng.N, step.off
    mask = ws["padding"].view(b, N)[:, off:off + n].cpu()
    assert torch.equal(mask.to(torch.int64), rec["mask"])
    live = rec["mask"] == 0
    tokens = ws["x"][0].view(b, N, D)[:, off:off + n].cpu()
    assert bool(torch.isfinite(tokens).all())
    d = rel_err(tokens[live], want[live])
    print(f"fixture {mode}: tokens (mask 0) rel-L2 {d:.3e}")
    assert 0 < d <= TOKENS_BOUND, d
    eng.gflat.zero_()
    dx = torch.zeros(b * N, D, device="cuda")
    dx.view(b, N, D)[:, off:off + n] = upstream.cuda()
    step.backward(ws, dx, lambda fn: fn())
    torch.cuda.synchronize()
    params = dict(model.encoders["audio"].named_parameters())
    assert set(params) == set(rec["grads"])
    for k, w in rec["grads"].items():
        got = eng.grad_of(params[k]).cpu()
        e = rel_err(got, w)
        print(f"fixture {mode}: {k}: rel-L2 {e:.3e}")
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


@pytest.mark.parametrize("mode", list(MODES))
def test_graph_replay_matches_eager_step(P, mode):
    """GraphedStep takes the direct path; its replay against the eager step from the same state: loss 1e-6 relative, every gradient
    tensor 5e-3 rel-L2 (the weight gradients are sums of fp32 atomics)"""
    cfg = nd_config(small_config, "mca", mode)
    sd = initial_state(P, cfg)
    batch = nd_batch(P, cfg)
    rep = graphed(P, cfg, sd, batch, deterministic=False, eager=False)
    eager = one_step(build(P, cfg, sd), batch)
    assert abs(rep["loss"] - eager["loss"]) <= 1e-6 * abs(eager["loss"]), (rep["loss"], eager["loss"])
    assert set(rep["grads"]) == set(eager["grads"])
    for name, g in eager["grads"].items():
        e = rel_err(rep["grads"][name], g)
        assert e <= 5e-3, (name, e)
    assert float(rep["grads"]["encoders.audio.embedding.weight"].abs().max()) > 0


@pytest.mark.parametrize("mode", list(MODES))
def test_deterministic_mode_is_bitwise_eager_and_replayed(P, mode):
    """two eager steps and one replayed step from identical state leave the same bits in the flat gradient buffer (the patch encoder's
    six gradients are in it) and in the weights after FusedAdamW.step()"""
    cfg = nd_config(small_config, "mca", mode)
    sd = initial_state(P, cfg)
    batch = nd_batch(P, cfg)
    a, b, r = (graphed(P, cfg, sd, batch, deterministic=True, eager=e) for e in (True, True, False))
    eng = a["model"].engine
    for name, p in a["model"].named_parameters():
        if name.startswith("encoders.audio."):
            assert float(eng.grad_of(p).abs().max()) > 0, name
    for x, y, what in ((a, b, "eager / eager"), (a, r, "eager / replay")):
        assert torch.equal(x["gflat"], y["gflat"]), what
        assert torch.equal(x["flat"], y["flat"]), what
    assert not torch.equal(a["flat"], build(P, cfg, sd).engine.flat), "the step moved no weight"
