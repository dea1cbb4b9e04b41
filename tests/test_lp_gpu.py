"""GPU tests of the probe stage (lp_accel_gpu.py): the HIP rank, uniformity and probe kernels against fp64 restatements of the
reference's formulas, a 3-epoch probe against a torch restatement of the reference's loop, and the script end to end."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eval_edge_util import _mask_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def mods():
    importlib.import_module("mca-paper_amd.build").build(verbose=False)
    return importlib.import_module("mca-paper_amd.metrics"), importlib.import_module("mca-paper_amd.probe")


def _fp64_counts(q, t, idx, delta):
    qn = F.normalize(q.double(), dim=1)
    tn = F.normalize(t.double(), dim=1)
    s = qn[idx] @ tn.T
    st = s[torch.arange(len(idx)), idx]
    above = s > (st - delta)[:, None]
    above[torch.arange(len(idx)), idx] = False          # the true target never counts itself
    return (s > (st + delta)[:, None]).sum(1), above.sum(1)


@pytest.mark.parametrize("nq,nt,d,c", [(1000, 1531, 512, 0.15), (257, 4099, 96, 0.4)])
def test_rank_kernel_against_fp64(mods, nq, nt, d, c):
    M, _ = mods
    g = torch.Generator().manual_seed(nq)
    t = torch.randn(nt, d, generator=g)
    q = c * t[:nq] + torch.randn(nq, d, generator=g)          # coupling c: about half the ranks above 0, up to several hundred
    mask = torch.rand(nq, generator=g) > 0.2
    idx = torch.nonzero(mask).reshape(-1)
    r = M.cosine_ranks(q.to(DEV), t.to(DEV), idx).cpu().long()
    lo, hi = _fp64_counts(q, t, idx, 2e-6)
    assert bool(((lo <= r) & (r <= hi)).all())
    assert (lo > 0).double().mean().item() > 0.3          # the counts are exercised, not just rank 0
    exact = ((lo == hi) & (r == lo)).double().mean().item()
    assert exact >= 0.999, exact
    assert torch.equal(r, M.cosine_ranks(q.to(DEV), t.to(DEV), idx).cpu().long())          # bitwise repeatable
    # get_rank_metrics against a chunked cosine_similarity restatement of the reference's loop
    ranks = []
    for c in range(0, len(idx), 128):
        ii = idx[c:c + 128]
        cs = F.cosine_similarity(q[ii].to(DEV)[:, None, :], t.to(DEV)[None, :, :], dim=2)
        ranks.append((cs > cs[torch.arange(len(ii)), ii.to(DEV)][:, None]).long().sum(1).cpu())
    ranks = torch.cat(ranks)
    med, r1, r5, r10 = M.get_rank_metrics(q, mask, t, device=DEV)
    n = len(ranks)
    assert abs(int(med) - int(ranks.median())) <= 1
    for got, k in ((r1, 1), (r5, 5), (r10, 10)):
        assert got.dim() == 0 and abs(float(got) - float((ranks < k).sum()) / n) <= 3.0 / n


def test_rank_strict_ties(mods):
    M, _ = mods
    g = torch.Generator().manual_seed(5)
    t = torch.randn(300, 64, generator=g)
    t[10] = t[3]                      # a duplicate of query 3's target: a tie, never counted
    t[200] = 2.5 * t[7]               # same direction as query 7's target: cosine ties up to rounding
    t[201] = t[5]                     # an exact duplicate of query 5's target: bitwise the same cosine, never counted
    q = torch.randn(300, 64, generator=g)
    q[3] = t[3]                       # query equal to its target: cosine 1, nothing strictly above
    r = M.cosine_ranks(q.to(DEV), t.to(DEV), torch.arange(300)).cpu()
    assert int(r[3]) == 0
    s = F.normalize(q.double(), dim=1) @ F.normalize(t.double(), dim=1).T
    for i, twin in ((5, 201), (7, 200)):
        others = torch.ones(300, dtype=torch.bool)
        others[[i, twin]] = False
        base = int((s[i, others] > s[i, i]).sum())          # no other target lies near the true one here (checked below)
        assert not bool(((s[i, others] - s[i, i]).abs() < 1e-5).any())
        assert int(r[i]) == base if i == 5 else int(r[i]) in (base, base + 1), (i, int(r[i]), base)
    with pytest.raises(RuntimeError):
        M.get_rank_metrics(q, torch.zeros(300, dtype=torch.bool), t, device=DEV)


@pytest.mark.parametrize("n", [2, 3, 1000, 4097])
@pytest.mark.parametrize("norm", [True, False])
def test_uniformity_against_fp64(mods, n, norm):
    M, _ = mods
    x = torch.randn(n, 96, generator=torch.Generator().manual_seed(n)) * (1.0 if norm else 0.1)
    ref = M.lunif(x.double(), 2, norm).item()
    torch32 = M.lunif(x.to(DEV), 2, norm).item()
    got = M.uniformity(x.to(DEV), 2, norm)
    assert got.dim() == 0 and got.dtype == torch.float32
    assert abs(got.item() - ref) <= 2 * abs(torch32 - ref) + 1e-6, (got.item(), ref, torch32)
    assert torch.equal(got, M.uniformity(x.to(DEV), 2, norm))


def test_uniformity_edges(mods):
    M, _ = mods
    assert np.isnan(M.uniformity(torch.randn(1, 8, device=DEV)).item())
    far = torch.tensor([[0.0] * 4, [100.0] + [0.0] * 3, [0.0, 100.0, 0.0, 0.0]], device=DEV)
    assert M.uniformity(far, 2, False).item() == float("-inf")
    assert M.lunif(far, 2, False).item() == float("-inf")
    u = M.Uniformity()
    v = u(far)                                          # torchmetrics forward: this call's value (norm=False), rows kept
    assert v.item() == float("-inf") and len(u.preds) == 1


def test_compute_cosines_and_cpu_inputs(mods):
    """compute_cosines against torch's cosine_similarity; cpu inputs of the HIP-backed names are copied to the HIP device
    (the reference's script loads its embeddings on the cpu), and a cpu ``device`` is refused before any launch"""
    M, _ = mods
    g = torch.Generator().manual_seed(2)
    e, es = torch.randn(96, generator=g), torch.randn(777, 96, generator=g)
    got = M.compute_cosines(e, es)                                  # cpu inputs
    assert got.device.type == "cuda" and got.shape == (777,)
    ref = F.cosine_similarity(e.double()[None, :], es.double(), dim=1)
    assert (got.double().cpu() - ref).abs().max().item() <= 1e-6
    x = torch.randn(300, 32, generator=g)
    u = M.Uniformity()
    v = u(x)                                                        # the reference's torchmetrics class takes cpu tensors
    assert v.device.type == "cuda" and abs(v.item() - M.lunif(x.double(), 2, False).item()) <= 1e-5
    mask = torch.rand(300, generator=g) > 0.5
    a = M.get_rank_metrics(x, mask, x * 0.5 + torch.randn(300, 32, generator=g), device=DEV)
    assert all(t.device.type == "cuda" and t.dim() == 0 for t in a)
    with pytest.raises(ValueError, match="cpu"):
        M.get_rank_metrics(x, mask, x, device="cpu")


def _loss(kind, z, y):
    if kind == "L1":
        return (z - y).abs().mean()
    if kind == "MSE":
        return ((z - y) ** 2).mean()
    return F.binary_cross_entropy_with_logits(z, y)


def _restated_step(module, x, y, kind, keep, p, dtype):
    m = [t.detach().to(DEV, dtype).clone().requires_grad_(True) for t in module.parameters()]
    x, y = x.to(DEV, dtype), y.to(DEV, dtype)
    if len(m) == 2:
        z = x @ m[0].T + m[1]
    else:
        h = torch.relu((x @ m[0].T + m[1]) * keep.to(DEV, dtype) / (1 - p))
        z = h @ m[2].T + m[3]
    loss = _loss(kind, z, y)
    loss.backward()
    return z.detach(), loss.detach(), torch.cat([t.grad.reshape(-1) for t in m])


@pytest.mark.parametrize("model", ["linear", "mlp"])
@pytest.mark.parametrize("kind", ["L1", "MSE", "BCE"])
@pytest.mark.parametrize("L", [1, 7, 33])
def test_probe_step_against_fp64(mods, model, kind, L):
    M, P = mods
    D, H, p, seed = 96, 40, 0.25, 11
    g = torch.Generator().manual_seed(L)
    n = 301                                   # batches of 150, 150 and a one-row batch
    x = torch.randn(n, D, generator=g)
    y = (torch.rand(n, L, generator=g) > 0.5).float() if kind == "BCE" else torch.randn(n, L, generator=g)
    torch.manual_seed(0)
    module = P.build_module(model, D, H, L, p)
    perm = torch.randperm(n, generator=g)
    pr = P.Probe(module, model, kind, x, y, x[:5], y[:5], 150, 1e-3, lambda s: 1.0, 4, 0.0, p, seed, torch.device(DEV))
    pr.perm.copy_(perm.to(torch.int32))
    for step, (r0, b) in enumerate([(0, 150), (150, 150), (300, 1)]):
        rows = perm[r0:r0 + b]
        pr.step = step
        rp = pr.perm.data_ptr() + 4 * r0
        pr.acc.zero_()
        nb = pr._forward(pr.x_train, rp, pr.y_train, rp, b, pr.pred_train.data_ptr() + 4 * r0 * L, True)
        gv = pr.params.gviews
        if model == "linear":
            P.call("mca_probe_tn_f32", pr.dz.data_ptr(), L, pr.x_train.data_ptr(), D, rp, b, L, D, pr.ws.data_ptr(), pr.ws.numel(),
                   gv[0].data_ptr(), gv[1].data_ptr(), P.stream_ptr())
        else:
            P.call("mca_probe_tn_f32", pr.dz.data_ptr(), L, pr.hid.data_ptr(), H, None, b, L, H, pr.ws.data_ptr(), pr.ws.numel(),
                   gv[2].data_ptr(), gv[3].data_ptr(), P.stream_ptr())
            P.call("mca_probe_tn_f32", pr.dhid.data_ptr(), H, pr.x_train.data_ptr(), D, rp, b, H, D, pr.ws.data_ptr(), pr.ws.numel(),
                   gv[0].data_ptr(), gv[1].data_ptr(), P.stream_ptr())
        P.call("mca_probe_loss_accum", pr.part.data_ptr(), nb, b * L, pr.acc.data_ptr(), P.stream_ptr())
        keep = _mask_ref(seed, step, b, H, p) if model == "mlp" else None
        z64, l64, g64 = _restated_step(module, x[rows], y[rows], kind, keep, p, torch.float64)
        z32, l32, g32 = _restated_step(module, x[rows], y[rows], kind, keep, p, torch.float32)
        pred = pr.pred_train[r0:r0 + b]
        for got, r32, r64, floor in ((pred, z32, z64, 1e-6), (pr.acc[0], l32, l64, 1e-6), (pr.params.gflat, g32, g64, 1e-7)):
            e = (got.double() - r64).abs().max().item()
            e32 = (r32.double() - r64).abs().max().item()
            assert e <= 2 * e32 + floor * max(1.0, r64.abs().max().item()), (model, kind, L, step, e, e32)


def _reference_loop(P, M, model, kind, data, B, H, lr, lam, clip, p, seed, epochs, dtype):
    """the reference's loop restated in torch (DataLoader over the tensors, AdamW, clip_grad_norm_, LambdaLR, the
    utils.training norms after the epoch's last step); the MLP's dropout draws the kernel's hash mask (``_mask_ref``), torch's
    device generator being out of reach.  -> per-epoch records and the final flat weights"""
    from torch.utils.data import DataLoader, TensorDataset
    from utils.training import get_grad_norm, get_param_norm
    x, y, xe, ye = data
    torch.manual_seed(seed)
    tdl = DataLoader(TensorDataset(x, y), batch_size=B, shuffle=True)
    edl = DataLoader(TensorDataset(xe, ye), batch_size=B)
    next(iter(tdl))
    mod = P.build_module(model, x.shape[1], H, 1, p).to(DEV, dtype)

    def fwd(xb, step):
        if model == "linear":
            return mod(xb).squeeze()
        z1 = mod[0](xb)
        if step is not None:
            z1 = z1 * _mask_ref(seed, step, xb.shape[0], H, p).to(DEV, dtype) / (1 - p)
        return mod[3](torch.relu(z1)).squeeze()
    opt = torch.optim.AdamW(mod.parameters(), lr=lr)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    lossf = {"L1": torch.nn.L1Loss(), "MSE": torch.nn.MSELoss(), "BCE": torch.nn.BCEWithLogitsLoss()}[kind]
    recs, step = [], 0
    for _ in range(epochs):
        tl, preds, labs = 0.0, [], []
        for xb, yb in tdl:
            xb, yb = xb.to(DEV, dtype), yb.to(DEV, dtype)
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
                el += lossf(z, yb.to(DEV, dtype)).item()
                ep.append(z)
        rec = {"train_loss": tl / len(tdl), "eval_loss": el / len(edl), "lr": opt.param_groups[0]["lr"],
               "param_norm": get_param_norm(mod).item(), "grad_norm": get_grad_norm(mod).item()}
        for split, pr_, lb in (("train", torch.cat(preds), torch.cat(labs)), ("eval", torch.cat(ep), ye.to(DEV, dtype))):
            if kind == "BCE":
                rec.update({f"{split}_{k}": v.item() for k, v in M.binary_metrics(M.binary_format(pr_, B, 1), lb).items() if k != "cm"})
            else:
                rec[f"{split}_PCC"] = M.pearson(pr_, lb).item()
        recs.append(rec)
    return recs, torch.cat([q.detach().reshape(-1) for q in mod.parameters()])


@pytest.mark.parametrize("model,kind", [("linear", "L1"), ("linear", "BCE"), ("mlp", "MSE"), ("mlp", "BCE")])
def test_probe_three_epochs_against_reference_loop(mods, model, kind):
    """every logged number of three epochs (losses, lr, param_norm, grad_norm = clip coefficient x norm, metrics) and the
    final weights against the reference's loop: the native error from the fp64 loop is at most 2 x the fp32 loop's plus a
    stated floor.  The MLP runs with dropout 0.1 through train_epoch."""
    M, P = mods
    sys.path.insert(0, REPO)
    lr_factor = importlib.import_module("train_accel_gpu").lr_factor
    D, H, B, seed, lr, clip, p, epochs = 64, 32, 256, 3, 3e-3, 0.5, 0.1 if model == "mlp" else 0.0, 3
    g = torch.Generator().manual_seed(9)
    x, xe = torch.randn(2500, D, generator=g), torch.randn(700, D, generator=g)
    w = torch.randn(D, generator=g)
    y, ye = x @ w / 8, xe @ w / 8
    if kind == "BCE":
        y, ye = (y > 0).float(), (ye > 0).float()
    total = epochs * (-(-2500 // B))
    lam = lambda s: lr_factor("cosine", s, 2, total)
    torch.manual_seed(seed)
    sm = P.EpochSampler(2500, 700, B)
    sm.first_batch()
    mod = P.build_module(model, D, H, 1, p)
    pr = P.Probe(mod, model, kind, x, y, xe, ye, B, lr, lam, total, clip, p, seed, torch.device(DEV))
    recs = []
    for e in range(epochs):
        pr.train_epoch(sm.draw())
        pr.eval_epoch()
        rec = P.Probe.read(pr.epoch_device_values())
        rec["lr"] = lr * lam(pr.step)          # what lp_accel_gpu.py logs
        recs.append(rec)
    data = (x, y, xe, ye)
    r32, w32 = _reference_loop(P, M, model, kind, data, B, H, lr, lam, clip, p, seed, epochs, torch.float32)
    r64, w64 = _reference_loop(P, M, model, kind, data, B, H, lr, lam, clip, p, seed, epochs, torch.float64)
    # floors: 1e-5 relative for losses, lr, norms and PCC (other fp32 reduction orders, carried through ten to thirty Adam
    # steps whose update m / sqrt(v) is normalised per element, move the trained weights by a few 1e-6 relative); one
    # prediction of the split for the threshold / ranking metrics (a score that lands on the other side of 0.5, or swaps
    # with a neighbour, moves them by about 1 / rows); 2e-4 for a weight (a few of those Adam steps of size ~lr)
    floor = lambda k: (2.0 / (2500 if k.startswith("train_") else 700)) if (kind == "BCE" and k.split("_", 1)[-1] in M.BINARY_METRICS) else 1e-5
    for e in range(epochs):
        assert set(recs[e]) - {"train_cm", "eval_cm"} == set(r64[e]), (set(recs[e]), set(r64[e]))
        for k, v64 in r64[e].items():
            err, err32 = abs(recs[e][k] - v64), abs(r32[e][k] - v64)
            assert err <= 2 * err32 + floor(k) * max(1.0, abs(v64)), (e, k, recs[e][k], r32[e][k], v64)
    err, err32 = (pr.params.flat.double() - w64).abs().max().item(), (w32.double() - w64).abs().max().item()
    assert err <= 2 * err32 + 2e-4, (err, err32)


def _run(args, env=None, timeout=240):
    return subprocess.run([sys.executable, *args], cwd=REPO, capture_output=True, text=True, timeout=timeout, env=env)


def test_lp_script_end_to_end(mods, tmp_path):
    emb = tmp_path / "emb"
    emb.mkdir()
    import yaml
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from util_small import small_config
    cfg = small_config("mca")
    y = dict(encoder_configs=cfg["encoder_configs"], hidden_size=cfg["dim"], layers=cfg["depth"], heads=cfg["heads"],
             dim_head=cfg["dim_head"], num_fusion_tokens=cfg["num_fusion_tokens"], batch_size=16, fcl=cfg["fcl"], fcl_root=cfg["fcl_root"],
             bimodal_contrastive=cfg["bimodal_contrastive"], non_fusion_fcl=cfg["non_fusion_fcl"], fusion_combos=cfg["fusion_combos"],
             zorro=cfg["zorro"], eao=cfg["eao"], no_fusion=cfg["no_fusion"], mean_pool=cfg["mean_pool"], output_dir=str(emb))
    tcfg = tmp_path / "train.yaml"
    tcfg.write_text(yaml.safe_dump(y, sort_keys=False))
    r = _run(["infer_accel_gpu.py", str(tcfg), "--synthetic", "4"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for split in ("train", "eval"):          # 0/1 labels for the BCE cases, intensities in [0, 3] for the refused one
        lab = torch.load(emb / f"{split}_labels.pt", weights_only=False)
        torch.save((lab > 0).float(), tmp_path / f"{split}_bin.pt")
        torch.save(lab.abs().clamp(max=3).round(), tmp_path / f"{split}_int.pt")
    bdir, idir = tmp_path / "emb_bin", tmp_path / "emb_int"
    for dd, suf in ((bdir, "bin"), (idir, "int")):
        dd.mkdir()
        for split in ("train", "eval"):
            for kind in ("embeddings", "masks"):
                os.symlink(emb / f"{split}_{kind}.pt", dd / f"{split}_{kind}.pt")
            os.symlink(tmp_path / f"{split}_{suf}.pt", dd / f"{split}_labels.pt")
    mods_ = [k for k in torch.load(emb / "train_embeddings.pt", weights_only=False) if isinstance(k, str) and k != "fusion"]
    rank_keys = [{f"{m}_{s}_{x}" for s in ("train", "test") for x in ("median_rank", "r1", "r5", "r10", "uniformity", "alignment")}
                 for m in mods_]
    cases = {
        "lin_l1": (emb, "model_type: linear\nloss_type: L1\ntask: 0\n", 0, {"PCC"}),
        "mlp_bce": (bdir, "model_type: mlp\nloss_type: BCE\ntask: -1\nlr: '1e-4'\n", 0,
                    {"precision", "recall", "accuracy", "cm", "f1", "specificity", "auroc", "auprc"}),
        "skip": (emb, "model_type: skip\n", 0, None),
        "ce": (emb, "model_type: linear\nloss_type: CE\n", 1, None),
        "bce_int": (idir, "model_type: linear\nloss_type: BCE\ntask: 2\n", 1, None),
    }
    for name, (d, body, rc, mets) in cases.items():
        msg = {"ce": "NotImplementedError: loss_type CE", "bce_int": "ValueError: BCE probe: targets must be 0 or 1, found"}.get(name)
        logs = []
        for rep in range(2 if rc == 0 else 1):
            out = tmp_path / f"{name}_{rep}"
            y = tmp_path / f"{name}_{rep}.yaml"
            y.write_text(f"embedding_dir: {d}\noutput_dir: {out}\nepochs: 3\nbatch_size: 24\nnum_warmup_steps: 2\nrank_metrics: True\n" + body)
            r = _run(["lp_accel_gpu.py", str(y)])
            assert r.returncode == rc, (name, r.returncode, r.stderr[-2000:])
            if rc:
                assert msg in r.stderr, (name, r.stderr[-2000:])
                continue
            assert (out / "config.yaml").exists()
            logs.append([json.loads(l) for l in open(out / "log.jsonl")])
        if rc:
            continue
        recs = logs[0]
        nm = len(mods_)
        assert [set(r) for r in recs[:nm]] == rank_keys
        assert set(recs[nm]) == {"train_uniformity_fusion", "test_uniformity_fusion"}
        probe_recs = recs[nm + 1:]
        if mets is None:
            assert probe_recs == []
        else:
            assert len(probe_recs) == 3
            want = {"train_loss", "eval_loss", "lr", "param_norm", "grad_norm"} | {f"{s}_{m}" for s in ("train", "eval") for m in mets}
            assert all(set(r) == want for r in probe_recs)
        assert logs[0] == logs[1], name          # two runs write identical values
