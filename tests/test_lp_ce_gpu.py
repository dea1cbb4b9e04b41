"""GPU tests of the probe with loss_type CE (mca_probe_head_ce_f32 through probe.Probe): one step against a float64 restatement and
three epochs against the reference's loop restated with nn.CrossEntropyLoss, by the rules and floors of tests/test_lp_gpu.py
(test_probe_step_against_fp64, test_probe_three_epochs_against_reference_loop), and lp_accel_gpu.py end to end on a tiny
saved-embedding directory."""
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from eval_edge_util import _mask_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    importlib.import_module("mca-paper_amd.build").build(verbose=False)
    return importlib.import_module("mca-paper_amd.metrics"), importlib.import_module("mca-paper_amd.probe")


def _restated_step(module, x, y, keep, p, dtype):
    m = [t.detach().to(DEV, dtype).clone().requires_grad_(True) for t in module.parameters()]
    x = x.to(DEV, dtype)
    if len(m) == 2:
        z = x @ m[0].T + m[1]
    else:
        h = torch.relu((x @ m[0].T + m[1]) * keep.to(DEV, dtype) / (1 - p))
        z = h @ m[2].T + m[3]
    loss = F.cross_entropy(z, y.to(DEV).long())
    loss.backward()
    return z.detach(), loss.detach(), torch.cat([t.grad.reshape(-1) for t in m])


@pytest.mark.parametrize("model", ["linear", "mlp"])
@pytest.mark.parametrize("C", [3, 33])
def test_ce_probe_step_against_fp64(mods, model, C):
    M, P = mods
    D, H, p, seed = 96, 40, 0.25, 11
    g = torch.Generator().manual_seed(C)
    n = 301                                   # batches of 150, 150 and a one-row batch
    x = torch.randn(n, D, generator=g)
    y = torch.randint(0, C, (n,), generator=g).float()
    torch.manual_seed(0)
    module = P.build_module(model, D, H, C, p)
    perm = torch.randperm(n, generator=g)
    pr = P.Probe(module, model, "CE", x, y, x[:5], y[:5], 150, 1e-3, lambda s: 1.0, 4, 0.0, p, seed, torch.device(DEV))
    assert pr.L == C and pr.y_train.shape == (n, 1) and pr.dz.shape == (150, C) and pr.pred_train.shape == (n, C)
    pr.perm.copy_(perm.to(torch.int32))
    for step, (r0, b) in enumerate([(0, 150), (150, 150), (300, 1)]):
        rows = perm[r0:r0 + b]
        pr.step = step
        rp = pr.perm.data_ptr() + 4 * r0
        pr.acc.zero_()
        nb = pr._forward(pr.x_train, rp, pr.y_train, rp, b, pr.pred_train.data_ptr() + 4 * r0 * C, True)
        gv = pr.params.gviews
        if model == "linear":
            P.call("mca_probe_tn_f32", pr.dz.data_ptr(), C, pr.x_train.data_ptr(), D, rp, b, C, D, pr.ws.data_ptr(), pr.ws.numel(),
                   gv[0].data_ptr(), gv[1].data_ptr(), P.stream_ptr())
        else:
            P.call("mca_probe_tn_f32", pr.dz.data_ptr(), C, pr.hid.data_ptr(), H, None, b, C, H, pr.ws.data_ptr(), pr.ws.numel(),
                   gv[2].data_ptr(), gv[3].data_ptr(), P.stream_ptr())
            P.call("mca_probe_tn_f32", pr.dhid.data_ptr(), H, pr.x_train.data_ptr(), D, rp, b, H, D, pr.ws.data_ptr(), pr.ws.numel(),
                   gv[0].data_ptr(), gv[1].data_ptr(), P.stream_ptr())
        P.call("mca_probe_loss_accum", pr.part.data_ptr(), nb, b, pr.acc.data_ptr(), P.stream_ptr())
        keep = _mask_ref(seed, step, b, H, p) if model == "mlp" else None
        z64, l64, g64 = _restated_step(module, x[rows], y[rows], keep, p, torch.float64)
        z32, l32, g32 = _restated_step(module, x[rows], y[rows], keep, p, torch.float32)
        pred = pr.pred_train[r0:r0 + b]
        for got, r32, r64, floor in ((pred, z32, z64, 1e-6), (pr.acc[0], l32, l64, 1e-6), (pr.params.gflat, g32, g64, 1e-7)):
            e = (got.double() - r64).abs().max().item()
            e32 = (r32.double() - r64).abs().max().item()
            print(f"{model} C={C} step {step}: native error {e:.3e}, fp32 restatement {e32:.3e}")
            assert e <= 2 * e32 + floor * max(1.0, r64.abs().max().item()), (model, C, step, e, e32)


def _reference_loop(P, M, model, data, C, B, H, lr, lam, clip, p, seed, epochs, dtype):
    """test_lp_gpu._reference_loop with nn.CrossEntropyLoss, a head of C outputs and the multiclass metrics of the softmax"""
    from torch.utils.data import DataLoader, TensorDataset
    from utils.training import get_grad_norm, get_param_norm
    x, y, xe, ye = data
    torch.manual_seed(seed)
    tdl = DataLoader(TensorDataset(x, y), batch_size=B, shuffle=True)
    edl = DataLoader(TensorDataset(xe, ye), batch_size=B)
    next(iter(tdl))
    mod = P.build_module(model, x.shape[1], H, C, p).to(DEV, dtype)

    def fwd(xb, step):
        if model == "linear":
            return mod(xb)
        z1 = mod[0](xb)
        if step is not None:
            z1 = z1 * _mask_ref(seed, step, xb.shape[0], H, p).to(DEV, dtype) / (1 - p)
        return mod[3](torch.relu(z1))
    opt = torch.optim.AdamW(mod.parameters(), lr=lr)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    lossf = torch.nn.CrossEntropyLoss()
    recs, step = [], 0
    for _ in range(epochs):
        tl, preds, labs = 0.0, [], []
        for xb, yb in tdl:
            xb, yb = xb.to(DEV, dtype), yb.to(DEV).long()
            z = fwd(xb, step)
            loss = lossf(z, yb)
            opt.zero_grad()
            loss.backward()
            tl += loss.item()
            preds.append(z.detach()); labs.append(yb)
            torch.nn.utils.clip_grad_norm_(mod.parameters(), clip)
            opt.step(); sch.step()
            step += 1
        el, ep = 0.0, []
        with torch.no_grad():
            for xb, yb in edl:
                z = fwd(xb.to(DEV, dtype), None)
                el += lossf(z, yb.to(DEV).long()).item()
                ep.append(z)
        rec = {"train_loss": tl / len(tdl), "eval_loss": el / len(edl), "lr": opt.param_groups[0]["lr"],
               "param_norm": get_param_norm(mod).item(), "grad_norm": get_grad_norm(mod).item()}
        for split, pr_, lb in (("train", torch.cat(preds), torch.cat(labs)), ("eval", torch.cat(ep), ye.to(DEV).long())):
            rec.update({f"{split}_{k}": v.item() for k, v in M.multiclass_metrics(torch.softmax(pr_.double(), 1), lb).items() if k != "cm"})
        recs.append(rec)
    return recs, torch.cat([q.detach().reshape(-1) for q in mod.parameters()])


@pytest.mark.parametrize("model", ["linear", "mlp"])
def test_ce_probe_three_epochs_against_reference_loop(mods, model):
    M, P = mods
    sys.path.insert(0, REPO)
    lr_factor = importlib.import_module("train_accel_gpu").lr_factor
    C, D, H, B, seed, lr, clip, p, epochs = 5, 64, 32, 256, 3, 3e-3, 0.5, 0.1 if model == "mlp" else 0.0, 3
    g = torch.Generator().manual_seed(9)
    x, xe = torch.randn(2500, D, generator=g), torch.randn(700, D, generator=g)
    w = torch.randn(D, C, generator=g)
    y, ye = (x @ w).argmax(1).float(), (xe @ w).argmax(1).float()
    total = epochs * (-(-2500 // B))
    lam = lambda s: lr_factor("cosine", s, 2, total)
    torch.manual_seed(seed)
    sm = P.EpochSampler(2500, 700, B)
    sm.first_batch()
    mod = P.build_module(model, D, H, C, p)
    pr = P.Probe(mod, model, "CE", x, y, xe, ye, B, lr, lam, total, clip, p, seed, torch.device(DEV))
    recs = []
    for e in range(epochs):
        pr.train_epoch(sm.draw())
        pr.eval_epoch()
        rec = P.Probe.read(pr.epoch_device_values())
        rec["lr"] = lr * lam(pr.step)
        recs.append(rec)
    assert len(recs[0]["eval_cm"]) == C and all(len(r) == C for r in recs[0]["eval_cm"]) and sum(map(sum, recs[0]["eval_cm"])) == 700
    data = (x, y, xe, ye)
    r32, w32 = _reference_loop(P, M, model, data, C, B, H, lr, lam, clip, p, seed, epochs, torch.float32)
    r64, w64 = _reference_loop(P, M, model, data, C, B, H, lr, lam, clip, p, seed, epochs, torch.float64)
    # the floors of test_probe_three_epochs_against_reference_loop: 1e-5 relative for losses, lr and norms, one prediction of the split
    # (2 / rows) for the argmax / ranking metrics as BCE's get there, 2e-4 for a weight
    floor = lambda k: (2.0 / (2500 if k.startswith("train_") else 700)) if k.split("_", 1)[-1] in M.MULTICLASS_METRICS else 1e-5
    for e in range(epochs):
        assert set(recs[e]) - {"train_cm", "eval_cm"} == set(r64[e]), (set(recs[e]), set(r64[e]))
        for k, v64 in r64[e].items():
            err, err32 = abs(recs[e][k] - v64), abs(r32[e][k] - v64)
            assert err <= 2 * err32 + floor(k) * max(1.0, abs(v64)), (e, k, recs[e][k], r32[e][k], v64)
    err, err32 = (pr.params.flat.double() - w64).abs().max().item(), (w32.double() - w64).abs().max().item()
    assert err <= 2 * err32 + 2e-4, (err, err32)
    assert recs[2]["train_loss"] < recs[0]["train_loss"]


def test_lp_script_with_ce(mods, tmp_path):
    """lp_accel_gpu.py on saved embeddings with loss_type: CE: num_classes from the YAML, and from the largest train label without it"""
    M, P = mods
    g = torch.Generator().manual_seed(4)
    emb = tmp_path / "emb"
    emb.mkdir()
    D, C = 32, 4
    for split, n in (("train", 90), ("eval", 40)):
        x = torch.randn(n, D, generator=g)
        lab = torch.randn(n, 3, generator=g)
        lab[:, 1] = torch.randint(0, C, (n,), generator=g).float()
        lab[:C, 1] = torch.arange(C).float()          # every class occurs
        torch.save({"fusion": x, "audio": x + 0.1 * torch.randn(n, D, generator=g)}, emb / f"{split}_embeddings.pt")
        torch.save({"fusion": torch.ones(n, dtype=torch.bool), "audio": torch.ones(n, dtype=torch.bool)}, emb / f"{split}_masks.pt")
        torch.save(lab, emb / f"{split}_labels.pt")
    want = {"train_loss", "eval_loss", "lr", "param_norm", "grad_norm"} | {f"{s}_{m}" for s in ("train", "eval") for m in M.MULTICLASS_METRICS}
    for name, body, classes in (("given", "model_type: linear\nnum_classes: 6\n", 6), ("inferred", "model_type: mlp\nhidden_size: 16\n", C)):
        out = tmp_path / name
        ypath = tmp_path / f"{name}.yaml"
        ypath.write_text(f"embedding_dir: {emb}\noutput_dir: {out}\nepochs: 2\nbatch_size: 32\nnum_warmup_steps: 2\nrank_metrics: False\n"
                         f"loss_type: CE\ntask: 1\n" + body)
        r = subprocess.run([sys.executable, "lp_accel_gpu.py", str(ypath)], cwd=REPO, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        recs = [json.loads(l) for l in open(out / "log.jsonl")]
        assert len(recs) == 2 and all(set(rec) == want for rec in recs), [set(rec) ^ want for rec in recs]
        for rec in recs:
            assert len(rec["train_cm"]) == classes and sum(map(sum, rec["train_cm"])) == 90 and sum(map(sum, rec["eval_cm"])) == 40
    ypath = tmp_path / "bad.yaml"
    ypath.write_text(f"embedding_dir: {emb}\noutput_dir: {tmp_path / 'bad'}\nloss_type: CE\ntask: 1\nnum_classes: 3\nrank_metrics: False\n")
    r = subprocess.run([sys.executable, "lp_accel_gpu.py", str(ypath)], cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode != 0 and "CE targets must be class indices 0 .. 2, found [3.0]" in r.stderr, r.stderr[-2000:]
