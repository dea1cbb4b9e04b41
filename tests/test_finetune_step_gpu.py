"""GPU tests of the supervised fine-tune step (mca-paper_amd/finetune.py) on small_config, b = 6, 2 layers: the trunk gradients of a
task loss against the oracle's pooled tokens + a torch head and loss under autograd (the bounds of tests/test_step_gpu.py::
test_small_step_vs_oracle), the head gradients against a float64 head on the native pooled tokens (the kernel's bounds,
tests/task_head_util.py), the pure contrastive and the multi-task combinations, invalid rows, the first optimizer step with the joint
clip, the head warm-up, deterministic mode, a three-step loss trajectory against the oracle + torch AdamW, and the refusals."""
import copy
import importlib

import pytest
import torch

import task_head_cases as TC
import task_head_util as TU
from util_small import small_config, rel_err, to_device

pytestmark = pytest.mark.gpu
optim = importlib.import_module("mca-paper_amd.optim")
B, SEED, P_DROP = 6, 5, 0.3
U = TU.U


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("mca-paper_amd")


@pytest.fixture(scope="module")
def FT():
    return importlib.import_module("mca-paper_amd.finetune")


_cases = {}


def case(P, variant):
    """(cfg, state dict, host batch) of a variant, built once and never changed: at least one sample lacks audio, one has it"""
    if variant not in _cases:
        cfg = small_config(variant)
        batch = P.data.synthetic_batch(cfg, B, seed=SEED, p_drop=P_DROP)
        has_audio = ~batch["audio"]["attention_mask"].bool().all(1)
        assert has_audio.any() and not has_audio.all(), "the seed must give samples with and without audio"
        sd = P.params.init_state_dict(cfg, seed=3)
        for k in sd:
            if k.endswith("embedding.weight"):
                sd[k][::2] *= 0.05
        _cases[variant] = (cfg, sd, batch)
    return _cases[variant]


def labels_for(loss_type, cols=3):
    g = torch.Generator().manual_seed(17)
    return torch.randint(0, 2, (B, cols), generator=g).float() if loss_type == "BCE" else torch.randn(B, cols, generator=g)


def build(P, FT, cfg, sd, n_out, deterministic=False, lr=1e-3, **step_kw):
    torch.manual_seed(43)
    model = P.build_model(copy.deepcopy(cfg))
    model.load_state_dict(sd, strict=False)
    model = model.cuda()
    model.engine.check_finite = "deferred"
    model.engine.set_deterministic(deterministic)
    opt = optim.FusedAdamW(model, lr=lr)
    torch.manual_seed(44)
    head = FT.TaskHead(cfg["dim"], n_out)
    w0 = {k: v.detach().clone() for k, v in head.state_dict().items()}
    return model, opt, head, w0, FT.FineTuneStep(model, head, opt, **step_kw)


def spy(step):
    """record what the step's one kernel call read and wrote (clones): pooled, present, d_pooled_in, then pred, loss, d_pooled"""
    seen, inner = [], step._task_kernel

    def wrapped(pooled, present, b, y, y_off, ld, d_in, base):
        rec = dict(pooled=pooled.clone(), present=present.clone(), d_in=None if d_in is None else d_in.clone())
        pred, loss, d_pooled = inner(pooled, present, b, y, y_off, ld, d_in, base)
        rec.update(pred=pred.clone(), loss=loss.clone(), d_pooled=d_pooled.clone())
        seen.append(rec)
        return pred, loss, d_pooled

    step._task_kernel = wrapped
    return seen


def torch_task_loss(pooled, slot, valid, W, bias, y, loss_type):
    z = pooled[valid, slot] @ W.t() + bias
    if loss_type == "BCE":
        return torch.nn.functional.binary_cross_entropy_with_logits(z, y[valid])
    return torch.nn.functional.mse_loss(z, y[valid]) if loss_type == "MSE" else torch.nn.functional.l1_loss(z, y[valid])


def valid_of(sample_mask, names, any_bits):
    v = torch.zeros(B, dtype=torch.bool)
    for i, n in enumerate(names):
        if (any_bits >> i) & 1:
            v |= sample_mask[n].cpu()
    return v


_oracle_fwd = {}


def oracle_forward(P, variant, mode):
    """the oracle's pooled tokens with every parameter requiring grad, once per (variant, mode); the graph is kept"""
    key = (variant, mode)
    if key not in _oracle_fwd:
        from oracle import mca_oracle as O
        cfg, sd, batch = case(P, variant)
        sd = {k: v.clone() for k, v in sd.items()}
        params = {k: v for k, v in sd.items() if O.is_param(k)}
        for p in params.values():
            p.requires_grad_(True)
        out = O.mca_forward(O.Structure(copy.deepcopy(cfg)), sd, batch, mode, no_loss=True)
        _oracle_fwd[key] = (params, out["pooled"], out["modality_sample_mask"])
    return _oracle_fwd[key]


def oracle_grads(P, FT, variant, mode, slot, any_bits, head_w, y, loss_type):
    cfg = case(P, variant)[0]
    params, pooled, sm = oracle_forward(P, variant, mode)
    valid = valid_of(sm, list(cfg["encoder_configs"]), any_bits)
    loss = torch_task_loss(pooled, slot, valid, head_w["head.weight"], head_w["head.bias"], y, loss_type)
    gs = torch.autograd.grad(loss, list(params.values()), retain_graph=True, allow_unused=True)
    return float(loss.detach()), {k: (torch.zeros_like(p) if g is None else g.detach()) for (k, p), g in zip(params.items(), gs)}, valid


# ------------------------------------------------------------------------------------------------ a. gradients against the oracle
@pytest.mark.parametrize("variant,loss_type,readout,task", [("mca", "MSE", "fusion", -1), ("mca", "BCE", "audio", 1), ("tab", "BCE", "fusion", -1),
                                                           ("tab", "MSE", "audio", 2)])
def test_task_gradients_against_the_oracle(P, FT, variant, loss_type, readout, task):
    cfg, sd, batch = case(P, variant)
    y = labels_for(loss_type)
    L = 3 if task == -1 else 1
    model, opt, head, w0, step = build(P, FT, cfg, sd, L, readout=readout, loss_type=loss_type, task=task, clip=2.0)
    seen = spy(step)
    out = step.step(to_device(batch, "cuda"), y.cuda())
    model.engine.assert_finite()
    ycols = y if task == -1 else y[:, task:task + 1]
    l_ref, g_ref, valid = oracle_grads(P, FT, variant, "fp32", step.slot, step.any_bits, w0, ycols, loss_type)
    l_emu, g_emu, _ = oracle_grads(P, FT, variant, "bf16emu", step.slot, step.any_bits, w0, ycols, loss_type)
    has_audio = ~batch["audio"]["attention_mask"].bool().all(1)
    if readout == "audio":
        assert torch.equal(valid, has_audio) and not valid.all()
    assert int(out["n_valid"]) == int(valid.sum()) and out["pred"].shape == (B, L)
    assert abs(float(out["task_loss"]) - l_ref) <= max(4 * abs(l_emu - l_ref), 1e-3 * abs(l_ref)), (float(out["task_loss"]), l_ref, l_emu)
    grads = {n: p.grad.detach().cpu() for n, p in model.named_parameters()}
    errs, errs_emu = [], []
    for n, gref in g_ref.items():
        gn = grads[n]
        if gref.abs().max() == 0:
            assert gn.abs().max() < 1e-6, n
            continue
        e, e_emu = rel_err(gn, gref), rel_err(g_emu[n], gref)
        errs.append(e); errs_emu.append(e_emu)
        assert e < 4 * e_emu + 2e-2, (n, e, e_emu)
    med, med_emu = sorted(errs)[len(errs) // 2], sorted(errs_emu)[len(errs_emu) // 2]
    print(f"fine-tune {variant} {loss_type} {readout}: median gradient error {med:.2e} (bf16-emulating oracle {med_emu:.2e}) over {len(errs)} tensors")
    assert med < 1.3 * med_emu + 0.01, (med, med_emu)
    # the head: a float64 head on the NATIVE pooled tokens, within the kernel's bounds
    rec = seen[0]
    x = rec["pooled"][:, step.slot].cpu()
    nat_valid = ((rec["present"].cpu() & step.any_bits) != 0)
    assert torch.equal(nat_valid, valid)
    ref = TU.head_reference(x, w0["head.weight"], w0["head.bias"], ycols, valid, {"MSE": TC.MSE, "BCE": TC.BCE}[loss_type])
    got = dict(pred=rec["pred"].cpu(), loss=rec["loss"][0].cpu(), gw=step.params.gviews[0].cpu(), gb=step.params.gviews[1].cpu())
    for k, v in got.items():
        want, tol = ref[k]
        assert ((v.double() - want).abs() <= tol).all(), (k, float((v.double() - want).abs().max()), float(tol.max()))
    assert float(got["gw"].abs().max()) > 0
    # d_pooled: dz . w in the readout slot, exactly 0 elsewhere and in invalid rows
    dp = rec["d_pooled"].cpu()
    dz, dz_tol = ref["dz"]
    want = dz @ ref["w"]
    tol = dz_tol @ ref["w"].abs() + (L + 1) * TU.U1 * (dz.abs() @ ref["w"].abs())
    assert ((dp[:, step.slot].double() - want).abs() <= tol).all()
    other = torch.ones(dp.shape[1], dtype=torch.bool)
    other[step.slot] = False
    assert (dp[:, other] == 0).all() and (dp[~valid] == 0).all()


# ------------------------------------------------------------------------------------------------ b. pure contrastive
def test_pure_contrastive_is_forward_backward_bit_for_bit(P, FT):
    cfg, sd, batch = case(P, "mca")
    dbatch = to_device(batch, "cuda")
    a, _, _, _, _ = build(P, FT, cfg, sd, 1, deterministic=True)
    out = a.engine.forward_backward(dbatch)
    m, opt, head, w0, step = build(P, FT, cfg, sd, 1, deterministic=True, task_weight=0.0, contrastive_weight=1.0)
    got = step.step(dbatch, labels_for("MSE").cuda())
    torch.cuda.synchronize()
    assert torch.equal(a.engine.gflat, m.engine.gflat) and float(a.engine.gflat.abs().max()) > 0
    assert torch.equal(out["loss"], got["contrastive_loss"]) and torch.equal(got["loss"], got["contrastive_loss"])
    assert set(got["losses"]) == set(out["losses"])
    assert float(step.params.gflat.abs().max()) == 0.0          # task_weight 0: no head gradient


# ------------------------------------------------------------------------------------------------ c. multi-task
def test_multi_task_adds_the_task_gradient_onto_half_the_contrastive_one(P, FT):
    cfg, sd, batch = case(P, "mca")
    dbatch, y = to_device(batch, "cuda"), labels_for("MSE").cuda()
    a, _, _, _, _ = build(P, FT, cfg, sd, 1, deterministic=True)
    a.engine.forward_backward(dbatch)
    g_ls_plain = a.engine.grad_of(a.loss.loss_fn.logit_scale).clone()
    m, opt, head, w0, step = build(P, FT, cfg, sd, 1, deterministic=True, task_weight=1.0, contrastive_weight=0.5, clip=2.0)
    seen = spy(step)
    out = step.step(dbatch, y)
    rec = seen[0]
    # the task part alone, by the same kernel on the same operands (before the optimizer moved the head: its initial weights)
    m2, _, _, _, alone = build(P, FT, cfg, sd, 1, deterministic=True, task_weight=1.0, contrastive_weight=0.0)
    yw, y_off, ld = alone._label_window(y)
    _, _, task = alone._task_kernel(rec["pooled"], rec["present"], B, yw, y_off, ld, None, 0.0)
    torch.cuda.synchronize()
    want = 0.5 * rec["d_in"].double() + task.double()          # exact in float64; the kernel rounds it once
    assert ((rec["d_pooled"].double() - want).abs() <= U * want.abs()).all()
    assert float(task.abs().max()) > 0 and float(rec["d_in"].abs().max()) > 0
    assert torch.equal(m.engine.grad_of(m.loss.loss_fn.logit_scale), 0.5 * g_ls_plain) and float(g_ls_plain.abs()) > 0
    assert torch.equal(out["loss"], 1.0 * out["task_loss"] + 0.5 * out["contrastive_loss"])


# ------------------------------------------------------------------------------------------------ d. invalid rows
def test_labels_of_invalid_rows_change_no_bit(P, FT):
    cfg, sd, batch = case(P, "mca")
    dbatch = to_device(batch, "cuda")
    has_audio = ~batch["audio"]["attention_mask"].bool().all(1)
    y = labels_for("MSE")
    y2 = y.clone()
    y2[~has_audio] = 1e6
    res = []
    for lab in (y, y2):
        m, opt, head, w0, step = build(P, FT, cfg, sd, 3, deterministic=True, readout="audio", task=-1)
        out = step.step(dbatch, lab.cuda())
        m.engine.assert_finite()
        res.append([out["pred"].clone(), out["task_loss"].clone(), out["n_valid"].clone(), m.engine.gflat.clone(), step.params.gflat.clone(),
                    m.engine.flat.clone(), step.params.flat.clone(), step.gnorm.clone()])
    assert int(res[0][2]) == int(has_audio.sum()) < B
    for x, z in zip(*res):
        assert torch.equal(x, z)


# ------------------------------------------------------------------------------------------------ e. the first optimizer step
def test_first_step_is_adamw_on_the_native_gradients_with_the_joint_clip(P, FT):
    cfg, sd, batch = case(P, "mca")
    LR, HEAD_LR, CLIP = 1e-3, 5e-3, 0.05
    m, opt, head, w0, step = build(P, FT, cfg, sd, 3, lr=LR, task=-1, head_lr=HEAD_LR, clip=CLIP)
    step.step(to_device(batch, "cuda"), labels_for("MSE").cuda())
    m.engine.assert_finite()
    hip = importlib.import_module("mca-paper_amd.hip")
    sq_t, sq_h = (torch.zeros(optim.SQNORM_WORDS, device="cuda") for _ in range(2))
    hip.call("mca_grad_sqnorm", m.engine.gflat.data_ptr(), m.engine.n_params, sq_t.data_ptr(), hip.stream_ptr())
    hip.call("mca_grad_sqnorm", step.params.gflat.data_ptr(), step.params.numel, sq_h.data_ptr(), hip.stream_ptr())
    assert torch.equal(step.gnorm, torch.sqrt(sq_t[0] + sq_h[0])) and float(sq_t[0]) > 0 and float(sq_h[0]) > 0
    gnorm = float(step.gnorm)
    coef = min(1.0, CLIP / (gnorm + 1e-6))
    assert coef < 1.0, "the clip must be active"

    def want(g, w, lr):
        gc = g.double() * coef
        return -lr * (gc / ((gc * gc).sqrt() + 1e-8)) - lr * 0.01 * w.double()          # first step: the corrected moments are g and g^2

    for i, k in enumerate(("head.weight", "head.bias")):
        upd = step.params.views[i].cpu().double() - w0[k].double()
        d = (upd - want(step.params.gviews[i].cpu(), w0[k], HEAD_LR)).abs().max()
        assert d < 2e-6 * (HEAD_LR / LR), (k, float(d))
    assert torch.equal(head.state_dict()["head.weight"].cpu(), step.params.views[0].cpu())          # the module sees the trained weights
    moved = 0
    for n, p in m.named_parameters():
        if n.endswith("embedding.weight") or n not in sd:
            continue
        upd = p.detach().cpu().double() - sd[n].double()
        d = (upd - want(p.grad.cpu(), sd[n], LR)).abs().max()
        assert d < 2e-6, (n, float(d))
        moved += int(upd.abs().max() > 0)
    assert moved > 10


# ------------------------------------------------------------------------------------------------ f. head warm-up
def test_head_warmup_leaves_the_trunk_alone_for_two_steps(P, FT):
    cfg, sd, batch = case(P, "mca")
    dbatch, y = to_device(batch, "cuda"), labels_for("MSE").cuda()
    m, opt, head, w0, step = build(P, FT, cfg, sd, 1, head_warmup_steps=2)
    flat0, h0 = m.engine.flat.clone(), step.params.flat.clone()
    for s in range(2):
        step.step(dbatch, y)
        m.engine.assert_finite()
        assert torch.equal(m.engine.flat, flat0) and float(opt.exp_avg.abs().max()) == 0 and float(opt.exp_avg_sq.abs().max()) == 0
        assert opt.step_count == 0 and step.step_count == s + 1
        assert not torch.equal(step.params.flat, h0)
        h0 = step.params.flat.clone()
    step.step(dbatch, y)
    m.engine.assert_finite()
    assert not torch.equal(m.engine.flat, flat0) and float(opt.exp_avg.abs().max()) > 0 and opt.step_count == 1
    assert not torch.equal(step.params.flat, h0)


# ------------------------------------------------------------------------------------------------ g. deterministic mode
def test_deterministic_mode_repeats_three_steps_bit_for_bit(P, FT):
    cfg, sd, batch = case(P, "tab")
    dbatch, y = to_device(batch, "cuda"), labels_for("BCE").cuda()
    res = []
    for _ in range(2):
        m, opt, head, w0, step = build(P, FT, cfg, sd, 3, deterministic=True, loss_type="BCE", task=-1, contrastive_weight=0.5)
        losses = [step.step(dbatch, y)["loss"].clone() for _ in range(3)]
        m.engine.assert_finite()
        res.append([m.engine.flat.clone(), step.params.flat.clone()] + losses)
    for x, z in zip(*res):
        assert torch.equal(x, z)
    assert not torch.equal(res[0][2], res[0][4])


# ------------------------------------------------------------------------------------------------ h. the loss over three steps
def test_three_step_loss_trajectory_against_the_oracle_with_torch_adamw(P, FT):
    from oracle import mca_oracle as O
    cfg, sd, batch = case(P, "mca")
    y = labels_for("MSE")
    LR, CLIP = 1e-3, 2.0
    m, opt, head, w0, step = build(P, FT, cfg, sd, 3, lr=LR, task=-1, clip=CLIP)
    dbatch = to_device(batch, "cuda")
    nat = [float(step.step(dbatch, y.cuda())["task_loss"]) for _ in range(3)]
    m.engine.assert_finite()
    slot, any_bits = step.slot, step.any_bits

    def oracle_run(mode):
        S = O.Structure(copy.deepcopy(cfg))
        osd = {k: v.clone() for k, v in sd.items()}
        params = [v.requires_grad_(True) for k, v in osd.items() if O.is_param(k)]
        W, bias = w0["head.weight"].clone().requires_grad_(True), w0["head.bias"].clone().requires_grad_(True)
        adam = torch.optim.AdamW(params + [W, bias], lr=LR)
        losses = []
        for _ in range(3):
            adam.zero_grad()
            out = O.mca_forward(S, osd, batch, mode, no_loss=True)
            valid = valid_of(out["modality_sample_mask"], list(cfg["encoder_configs"]), any_bits)
            loss = torch_task_loss(out["pooled"], slot, valid, W, bias, y, "MSE")
            loss.backward()
            torch.nn.utils.clip_grad_norm_([p for p in params + [W, bias] if p.grad is not None], CLIP)
            adam.step()
            losses.append(float(loss))
        return losses

    ref, emu = oracle_run("fp32"), oracle_run("bf16emu")
    print("fine-tune loss over three steps: native", nat, "oracle fp32", ref, "oracle bf16emu", emu)
    assert ref[2] < ref[0]
    for i in range(3):
        assert abs(nat[i] - ref[i]) <= max(4 * abs(emu[i] - ref[i]), 1e-3 * abs(ref[i])), (i, nat[i], ref[i], emu[i])


# ------------------------------------------------------------------------------------------------ i. refusals, the dropout counter
def test_refusals(P, FT, monkeypatch):
    cfg, sd, batch = case(P, "mca")
    model = P.build_model(copy.deepcopy(cfg)).cuda()
    opt = optim.FusedAdamW(model, lr=1e-3)
    mk = lambda L=1, dim=cfg["dim"], **kw: FT.FineTuneStep(model, FT.TaskHead(dim, L), opt, **kw)
    with pytest.raises(NotImplementedError, match="data-parallel"):
        mk(dp=object())
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="WORLD_SIZE = 2"):
        mk()
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(ValueError, match="D = 128"):
        mk(dim=64)
    with pytest.raises(ValueError, match="at most 64"):
        mk(L=65, task=-1)
    with pytest.raises(NotImplementedError, match="L1, MSE and BCE"):
        mk(loss_type="CE")
    with pytest.raises(ValueError, match="must not be negative"):
        mk(task_weight=-1.0)
    with pytest.raises(ValueError, match="must not be negative"):
        mk(contrastive_weight=-0.5)
    with pytest.raises(ValueError, match="both 0"):
        mk(task_weight=0.0, contrastive_weight=0.0)
    with pytest.raises(KeyError, match="fusion"):
        mk(readout="smell")
    with pytest.raises(ValueError, match="one label column"):
        mk(L=3, task=0)
    monkeypatch.setattr(model.engine, "can_forward_backward", lambda: False)
    with pytest.raises(NotImplementedError, match="native encoders"):
        mk()
    monkeypatch.undo()
    eao = P.build_model(copy.deepcopy(small_config("eao"))).cuda()
    with pytest.raises(NotImplementedError, match="EAO"):
        FT.FineTuneStep(eao, FT.TaskHead(128, 1), optim.FusedAdamW(eao, lr=1e-3), readout="audio")
    step = mk(loss_type="BCE", task=1)
    with pytest.raises(ValueError, match="0 or 1"):
        step.check_labels(torch.tensor([[0.0, 0.5, 7.0], [1.0, 1.0, 0.0]]))
    step.check_labels(torch.tensor([[3.0, 1.0, 7.0], [5.0, 0.0, 0.0]]))          # only the task's column counts
    with pytest.raises(IndexError, match="3 columns"):
        mk(task=5).step(to_device(batch, "cuda"), labels_for("MSE").cuda())
    graph = importlib.import_module("mca-paper_amd.graph")
    g = graph.GraphedStep(model, opt, to_device(batch, "cuda"), clip=2.0)
    with pytest.raises(RuntimeError, match="GraphedStep"):
        mk()
    del g


def test_modality_dropout_counter_advances_once_a_step(P, FT):
    cfg, sd, batch = case(P, "mca")
    full = to_device(P.data.synthetic_batch(cfg, B, seed=SEED, p_drop=0.0), "cuda")
    m, opt, head, w0, step = build(P, FT, cfg, sd, 1)
    m.train()
    m.engine.set_modality_dropout({n: 0.5 for n in m.modality_types}, seed=42, keep_one=True, step=3)
    for t in (3, 4):
        out = step.step(full, labels_for("MSE").cuda())
        m.engine.assert_finite()
        assert m.engine.modality_dropout_step() == t + 1
        assert out["modality_dropped"].shape == (B, 3) and out["modality_dropped"].any()
        for i, n in enumerate(m.modality_types):
            assert torch.equal(out["modality_sample_mask"][n], ~out["modality_dropped"][:, i])
    pred, valid = step.predict(full)          # eval: nothing dropped, the counter stays
    assert valid.all() and pred.shape == (B, 1) and m.engine.modality_dropout_step() == 5 and m.training
