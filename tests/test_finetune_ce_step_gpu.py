"""GPU tests of the fine-tune step with loss_type="CE" (mca-paper_amd/finetune.py, csrc/class_head.hip) on the small model of
tests/test_finetune_step_gpu.py, whose helpers and bounds these tests take unchanged: one CE step against the oracle's pooled tokens +
torch's cross_entropy on the readout slot (loss, trunk gradients, head gradients against a float64 head on the native pooled tokens,
the updated weights), the multi-task form with unlabelled rows, class weights with smoothing, the head warm-up, a five-step run on a
separable labelling, the refusals, and finetune_accel_gpu.py with a CE YAML."""
import copy
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import class_head_util as CU
import test_finetune_step_gpu as FS
from conftest import REPO
from util_small import rel_err, small_config, to_device

pytestmark = pytest.mark.gpu
optim = importlib.import_module("mca-paper_amd.optim")
B, U = FS.B, FS.U
NC = 3          # classes


@pytest.fixture(scope="module")
def P():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("mca-paper_amd")


@pytest.fixture(scope="module")
def FT():
    return importlib.import_module("mca-paper_amd.finetune")


def class_labels(unlabelled=()):
    """(B, 3) labels: column 1 holds class indices (every class occurs), the other columns values CE must not read"""
    y = torch.full((B, 3), float("nan"))
    y[:, 1] = torch.tensor([0, 2, 1, 2, 0, 1][:B]).float()
    for r in unlabelled:
        y[r, 1] = -1.0
    return y


def oracle_ce(P, variant, mode, slot, any_bits, head_w, y, cw=None, eps=0.0):
    """torch's cross_entropy on the oracle's readout slot over the valid and labelled rows -> (loss, trunk gradients, valid)"""
    cfg = FS.case(P, variant)[0]
    params, pooled, sm = FS.oracle_forward(P, variant, mode)
    valid = FS.valid_of(sm, list(cfg["encoder_configs"]), any_bits)
    rows = valid & (y >= 0)
    z = pooled[rows, slot] @ head_w["head.weight"].t() + head_w["head.bias"]
    loss = F.cross_entropy(z, y[rows].long(), weight=cw, label_smoothing=eps)
    gs = torch.autograd.grad(loss, list(params.values()), retain_graph=True, allow_unused=True)
    return float(loss.detach()), {k: (torch.zeros_like(p) if g is None else g.detach()) for (k, p), g in zip(params.items(), gs)}, valid


def check_head(step, rec, w0, y, valid, cw=None, eps=0.0, tw=1.0):
    """pred, loss, gw, gb and d_pooled of the recorded kernel call against a float64 head on the NATIVE pooled tokens"""
    x = rec["pooled"][:, step.slot].cpu()
    ref = CU.general_reference(x, w0["head.weight"], w0["head.bias"], y, valid, cw, eps, tw)
    got = dict(pred=rec["pred"].cpu(), loss=rec["loss"].cpu(), gw=step.params.gviews[0].cpu(), gb=step.params.gviews[1].cpu())
    for k, v in got.items():
        want, tol = ref[k]
        assert ((v.double() - want).abs() <= tol).all(), (k, float((v.double() - want).abs().max()), float(tol.max()))
    dz, dz_tol = ref["dz"]
    return ref, dz, dz_tol


# ------------------------------------------------------------------------------------------------ a. one step against the oracle
@pytest.mark.parametrize("variant,readout", [("mca", "fusion"), ("tab", "audio")])
def test_ce_step_against_the_oracle(P, FT, variant, readout):
    cfg, sd, batch = FS.case(P, variant)
    y = class_labels()
    LR, CLIP = 1e-3, 0.05
    model, opt, head, w0, step = FS.build(P, FT, cfg, sd, NC, lr=LR, readout=readout, loss_type="CE", task=1, clip=CLIP)
    seen = FS.spy(step)
    out = step.step(to_device(batch, "cuda"), y.cuda())
    model.engine.assert_finite()
    yc = y[:, 1]
    l_ref, g_ref, valid = oracle_ce(P, variant, "fp32", step.slot, step.any_bits, w0, yc)
    l_emu, g_emu, _ = oracle_ce(P, variant, "bf16emu", step.slot, step.any_bits, w0, yc)
    assert int(out["n_valid"]) == int(valid.sum()) and out["pred"].shape == (B, NC)
    if readout == "audio":
        assert not valid.all()
    # the bounds of test_task_gradients_against_the_oracle, unchanged
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
    print(f"fine-tune {variant} CE {readout}: median gradient error {med:.2e} (bf16-emulating oracle {med_emu:.2e}) over {len(errs)} tensors")
    assert med < 1.3 * med_emu + 0.01, (med, med_emu)
    # the head on the native pooled tokens, within the kernel's bounds; d_pooled: dz . w in the readout slot, 0 elsewhere
    rec = seen[0]
    assert torch.equal((rec["present"].cpu() & step.any_bits) != 0, valid)
    ref, dz, dz_tol = check_head(step, rec, w0, yc, valid)
    assert float(step.params.gviews[0].abs().max()) > 0
    dp = rec["d_pooled"].cpu()
    want = dz @ ref["w"]
    tol = dz_tol @ ref["w"].abs() + (NC + 1) * CU.U1 * (dz.abs() @ ref["w"].abs())
    assert ((dp[:, step.slot].double() - want).abs() <= tol).all()
    other = torch.ones(dp.shape[1], dtype=torch.bool)
    other[step.slot] = False
    assert (dp[:, other] == 0).all() and (dp[~valid] == 0).all()
    # the updated weights: the first AdamW step on the native gradients with the joint clip (test_first_step_is_adamw_...'s bounds)
    coef = min(1.0, CLIP / (float(step.gnorm) + 1e-6))
    assert coef < 1.0, "the clip must be active"

    def upd(g, w):
        gc = g.double() * coef
        return -LR * (gc / ((gc * gc).sqrt() + 1e-8)) - LR * 0.01 * w.double()

    for i, k in enumerate(("head.weight", "head.bias")):
        d = (step.params.views[i].cpu().double() - w0[k].double() - upd(step.params.gviews[i].cpu(), w0[k])).abs().max()
        assert d < 2e-6, (k, float(d))
    moved = 0
    for n, p in model.named_parameters():
        if n.endswith("embedding.weight") or n not in sd:
            continue
        u = p.detach().cpu().double() - sd[n].double()
        assert (u - upd(p.grad.cpu(), sd[n])).abs().max() < 2e-6, n
        moved += int(u.abs().max() > 0)
    assert moved > 10


# ------------------------------------------------------------------------------------------------ b. multi-task, unlabelled rows
def test_unlabelled_rows_keep_the_contrastive_gradient_alone(P, FT):
    cfg, sd, batch = FS.case(P, "mca")
    unl = [1, 4]          # a third of the rows
    y = class_labels(unlabelled=unl)
    m, opt, head, w0, step = FS.build(P, FT, cfg, sd, NC, deterministic=True, loss_type="CE", task=1, task_weight=1.0, contrastive_weight=0.5)
    seen = FS.spy(step)
    out = step.step(to_device(batch, "cuda"), y.cuda())
    m.engine.assert_finite()
    rec = seen[0]
    valid = (rec["present"].cpu() & step.any_bits) != 0
    assert int(out["n_valid"]) == int((valid & (y[:, 1] >= 0)).sum()) < int(valid.sum())
    assert torch.equal(rec["d_pooled"][unl], 0.5 * rec["d_in"][unl]) and float(rec["d_in"][unl].abs().max()) > 0          # (0.5 x: exact)
    lab = [r for r in range(B) if r not in unl and valid[r]]
    assert not torch.equal(rec["d_pooled"][lab][:, step.slot], 0.5 * rec["d_in"][lab][:, step.slot])
    other = [s for s in range(rec["d_pooled"].shape[1]) if s != step.slot]
    assert torch.equal(rec["d_pooled"][:, other], 0.5 * rec["d_in"][:, other])
    check_head(step, rec, w0, y[:, 1], valid)
    assert torch.equal(out["loss"], 1.0 * out["task_loss"] + 0.5 * out["contrastive_loss"])


# ------------------------------------------------------------------------------------------------ c. class weights and smoothing
def test_class_weights_and_smoothing(P, FT):
    cfg, sd, batch = FS.case(P, "mca")
    y = class_labels(unlabelled=[3])
    cw, eps, tw = [2.0, 0.0, 0.5], 0.1, 0.7
    m, opt, head, w0, step = FS.build(P, FT, cfg, sd, NC, loss_type="CE", task=1, task_weight=tw, class_weights=cw, label_smoothing=eps)
    seen = FS.spy(step)
    out = step.step(to_device(batch, "cuda"), y.cuda())
    m.engine.assert_finite()
    rec = seen[0]
    valid = (rec["present"].cpu() & step.any_bits) != 0
    cwt = torch.tensor(cw)
    check_head(step, rec, w0, y[:, 1], valid, cwt, eps, tw)
    rows = valid & (y[:, 1] >= 0)
    z = rec["pooled"][:, step.slot].cpu().double() @ w0["head.weight"].double().t() + w0["head.bias"].double()
    want = F.cross_entropy(z[rows], y[rows, 1].long(), weight=cwt.double(), label_smoothing=float(torch.tensor(eps)))
    assert abs(float(out["task_loss"]) - float(want)) <= 1e-5 * float(want)
    assert float(rec["loss"][2]) == float(cwt[y[rows, 1].long()].sum()) and int(out["n_valid"]) == int(rows.sum())
    assert torch.equal(out["loss"], tw * out["task_loss"])


# ------------------------------------------------------------------------------------------------ d. head warm-up
def test_head_warmup_with_ce(P, FT):
    cfg, sd, batch = FS.case(P, "mca")
    dbatch, y = to_device(batch, "cuda"), class_labels().cuda()
    m, opt, head, w0, step = FS.build(P, FT, cfg, sd, NC, loss_type="CE", task=1, head_warmup_steps=1)
    flat0, h0 = m.engine.flat.clone(), step.params.flat.clone()
    step.step(dbatch, y)
    m.engine.assert_finite()
    assert torch.equal(m.engine.flat, flat0) and opt.step_count == 0 and not torch.equal(step.params.flat, h0)
    step.step(dbatch, y)
    m.engine.assert_finite()
    assert not torch.equal(m.engine.flat, flat0) and opt.step_count == 1


# ------------------------------------------------------------------------------------------------ e. five steps
def test_training_loss_falls_on_a_separable_labelling(P, FT):
    cfg, sd, batch = FS.case(P, "mca")
    has_audio = ~batch["audio"]["attention_mask"].bool().all(1)          # what the model can see separates the two classes
    y = torch.zeros(B, 3)
    y[:, 1] = has_audio.float() * 2
    m, opt, head, w0, step = FS.build(P, FT, cfg, sd, NC, lr=1e-3, loss_type="CE", task=1, head_lr=1e-2)
    step.check_labels(y)
    dbatch = to_device(batch, "cuda")
    losses = [float(step.step(dbatch, y.cuda())["task_loss"]) for _ in range(5)]
    m.engine.assert_finite()
    print("CE training loss over five steps:", losses)
    assert losses[4] < losses[0] and all(l == l for l in losses)
    pred, valid = step.predict(dbatch)
    assert pred.shape == (B, NC) and valid.all()
    sdict = step.state_dict()
    assert set(sdict) == {"head", "exp_avg", "exp_avg_sq", "step"} and sdict["head"]["head.weight"].shape == (NC, cfg["dim"])


# ------------------------------------------------------------------------------------------------ f. refusals
def test_ce_refusals(P, FT):
    cfg, sd, batch = FS.case(P, "mca")
    model = P.build_model(copy.deepcopy(cfg)).cuda()
    opt = optim.FusedAdamW(model, lr=1e-3)
    mk = lambda L=NC, **kw: FT.FineTuneStep(model, FT.TaskHead(cfg["dim"], L), opt, loss_type="CE", **kw)
    with pytest.raises(ValueError, match="task -1"):
        mk(task=-1)
    with pytest.raises(ValueError, match="the head has 3 outputs"):
        mk(num_classes=4)
    with pytest.raises(NotImplementedError, match="L1, MSE and BCE"):
        mk(L=1)
    with pytest.raises(ValueError, match="num_classes"):
        mk(L=2, num_classes=1)
    with pytest.raises(ValueError, match="at most 64"):
        mk(L=65, num_classes=65)
    with pytest.raises(ValueError, match="2 entries"):
        mk(class_weights=[1.0, 2.0])
    with pytest.raises(ValueError, match="label_smoothing"):
        mk(label_smoothing=1.0)
    with pytest.raises(ValueError, match="belong to loss_type CE"):
        FT.FineTuneStep(model, FT.TaskHead(cfg["dim"], 1), opt, loss_type="MSE", label_smoothing=0.1)
    step = mk(task=1)
    with pytest.raises(ValueError, match=r"\[3\.0\]"):
        step.check_labels(torch.tensor([[9.0, 0.0, 9.0], [9.0, 3.0, 9.0]]))
    with pytest.raises(ValueError, match=r"0\.5"):
        step.check_labels(torch.tensor([[9.0, 0.5, 9.0]]))
    step.check_labels(torch.tensor([[9.0, 2.0, 0.5], [9.0, -1.0, 7.0]]))          # only the task's column counts; negative: unlabelled


# ------------------------------------------------------------------------------------------------ g. the script
def test_finetune_script_with_a_ce_yaml(P, tmp_path):
    import yaml
    ft = {"loss_type": "CE", "task": 2, "num_classes": 4, "class_weights": [1.0, 2.0, 0.5, 1.0], "label_smoothing": 0.05, "head_lr": 5e-3}
    cfg = small_config("mca")
    mod_cfg = {name: {"type": "embedded_sequence", "pad_len": enc["max_tokens"], "embedding_size": enc["input_size"], "data_col_name": "data"}
               for name, enc in cfg["encoder_configs"].items()}
    out = tmp_path / "ce"
    y = dict(encoder_configs=cfg["encoder_configs"], modality_config=mod_cfg, hidden_size=cfg["dim"], layers=cfg["depth"], heads=cfg["heads"],
             dim_head=cfg["dim_head"], num_fusion_tokens=cfg["num_fusion_tokens"], batch_size=4, fcl=cfg["fcl"], fcl_root=cfg["fcl_root"],
             bimodal_contrastive=cfg["bimodal_contrastive"], non_fusion_fcl=cfg["non_fusion_fcl"], fusion_combos=cfg["fusion_combos"],
             zorro=cfg["zorro"], eao=cfg["eao"], no_fusion=cfg["no_fusion"], mean_pool=cfg["mean_pool"], epochs=2, lr=1e-3,
             lr_scheduler_type="cosine", num_warmup_steps=1, clip=2.0, seed=7, output_dir=str(out), dataset="unused", label_col="Labels",
             finetune=ft)
    ypath = tmp_path / "ce.yaml"
    ypath.write_text(yaml.safe_dump(y, sort_keys=False))
    r = subprocess.run([sys.executable, os.path.join(REPO, "finetune_accel_gpu.py"), str(ypath), "--synthetic", "2"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in open(out / "log.jsonl")]
    assert [rec["epoch"] for rec in recs] == [0, 1]
    M = P.metrics.MULTICLASS_METRICS
    for rec in recs:
        assert set(rec) == {"epoch", "train_loss", "eval_loss", "lr", "grad_norm"} | {f"eval_{k}" for k in M}, rec
        cm = rec["eval_cm"]
        assert len(cm) == 4 and all(len(row) == 4 for row in cm) and sum(map(sum, cm)) > 0
        assert rec["eval_loss"] == rec["eval_loss"] and rec["eval_loss"] > 0 and 0 <= rec["eval_accuracy"] <= 1
    assert os.path.exists(out / "head_state.pt")
    hs = torch.load(out / "head_state.pt", weights_only=True)
    assert hs["head"]["head.weight"].shape == (4, 128) and hs["step"] == 4
