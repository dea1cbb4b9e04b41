"""CPU tests of the probe stage (lp_accel_gpu.py): the eval config loader, the script's import block, the per-epoch metric
formulas against sklearn / scipy, and the host RNG order of the probe against a restatement of the reference's loop."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
C = importlib.import_module("mca-paper_amd.config")
M = importlib.import_module("mca-paper_amd.metrics")
P = importlib.import_module("mca-paper_amd.probe")

DEFAULTS = {"embedding_dir": "", "task": 0, "loss_type": "L1", "model_type": "linear", "hidden_size": 256, "dropout": 0.1,
            "wandb_name": "MCA", "lr": 1e-5, "lr_scheduler_type": "cosine", "num_warmup_steps": 1000, "rank_metrics": True,
            "epochs": 1024, "clip": 2.0, "metric": "PCC", "output_dir": "", "wandb_job_name": "MCA-DefaultJobName", "seed": 42,
            "batch_size": 1024, "threshold": 0.0}


def test_eval_config_defaults():
    d = C.get_cfg_defaults_embedding_eval()
    assert dict(d) == DEFAULTS
    assert all(type(d[k]) is type(v) for k, v in DEFAULTS.items())


def test_eval_config_merge(tmp_path, monkeypatch):
    import yaml
    monkeypatch.chdir(tmp_path)
    out = tmp_path / "probe_out"
    y = tmp_path / "a.yaml"
    y.write_text(f"lr: '1e-4'\nnew_key: [1, 2]\nmodel_type: mlp\noutput_dir: {out}\n")
    cfg = C.embedding_eval_config(str(y))
    assert cfg.lr == 1e-4 and type(cfg.lr) is float
    assert cfg.new_key == [1, 2] and cfg.model_type == "mlp"
    assert cfg.output_dir == str(out)                          # the YAML's output_dir wins over the timestamped one
    dumped = yaml.safe_load(open(out / "config.yaml"))
    assert dumped["lr"] == 1e-4 and dumped["new_key"] == [1, 2] and set(DEFAULTS) <= set(dumped)
    bad = tmp_path / "b.yaml"
    bad.write_text("lr: 1\n")                                  # int for a float default: yacs refuses
    with pytest.raises(ValueError):
        C.embedding_eval_config(str(bad))
    plain = tmp_path / "c.yaml"
    plain.write_text("epochs: 3\n")
    cfg = C.embedding_eval_config(str(plain))
    assert cfg.output_dir.startswith("training_output_") and os.path.isfile(os.path.join(cfg.output_dir, "config.yaml"))


def test_eval_yaml_census_resolves(golden_dir):
    census = json.load(open(os.path.join(golden_dir, "ref_eval_yaml_census.json")))
    assert len(census) == 99
    kinds = {}
    for name, ent in census.items():
        cfg = C.get_cfg_defaults_embedding_eval()
        C._merge_yacs(cfg, ent["settings"])
        plan = P.plan(cfg, n_labels_all=33)
        if plan is None:
            kinds[name] = "rank only"
            continue
        assert plan["model"] in ("linear", "mlp") and plan["loss"] in ("L1", "BCE")
        assert plan["L"] == (33 if cfg.task == -1 else 1)
        assert plan["metrics"] == (list(M.BINARY_METRICS) if plan["loss"] == "BCE" else ["PCC"])
        kinds[name] = plan["model"]
    assert sum(v == "rank only" for v in kinds.values()) == 30
    assert sum(v == "linear" for v in kinds.values()) == 42 and sum(v == "mlp" for v in kinds.values()) == 27


def test_plan_refusals():
    cfg = C.get_cfg_defaults_embedding_eval()
    cfg.loss_type = "CE"
    with pytest.raises(NotImplementedError):
        P.plan(cfg)
    cfg.loss_type, cfg.task = "L1", -1
    with pytest.raises(NotImplementedError):
        P.plan(cfg, 7)
    with pytest.raises(ValueError, match="3.0"):
        P.check_binary_targets(torch.tensor([0.0, 1.0, 3.0]))


def test_lp_script_imports_resolve():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from utils.training import get_param_norm, get_grad_norm, count_parameters, move_to\n"
            "from utils.config import embedding_eval_config\n"
            "from utils.metrics import Alignment, Uniformity, get_rank_metrics\n"
            "assert callable(Uniformity.__call__) and callable(Alignment.__call__)\n" % REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr


def _data(seed):
    g = torch.Generator().manual_seed(seed)
    n = 997
    y = (torch.rand(n, generator=g) > 0.4).float()
    p = torch.round(torch.randn(n, generator=g) * 4) / 4          # heavy ties
    p[:300] = torch.rand(300, generator=g)                          # first batches: probabilities, no sigmoid
    p[300:350] = torch.round(p[300:350].clamp(0, 1) * 4) / 4
    return p, y


def test_binary_metrics_against_sklearn():
    from sklearn import metrics as skm
    p, y = _data(1)
    B = 100
    probs = M.binary_format(p, B, 1)
    ref = p.clone()
    for b0 in range(0, len(p), B):
        seg = ref[b0:b0 + B]
        if ((seg < 0) | (seg > 1)).any():
            ref[b0:b0 + B] = torch.sigmoid(seg)
    assert torch.equal(probs, ref)
    assert torch.equal(probs[:300], p[:300])                       # batches inside [0, 1] are left alone
    got = M.binary_metrics(probs, y)
    yn, pn = y.numpy().astype(int), probs.double().numpy()
    hard = (pn > 0.5).astype(int)
    want = {"precision": skm.precision_score(yn, hard, zero_division=0), "recall": skm.recall_score(yn, hard, zero_division=0),
            "accuracy": skm.accuracy_score(yn, hard), "f1": skm.f1_score(yn, hard, zero_division=0),
            "specificity": skm.recall_score(1 - yn, 1 - hard, zero_division=0),
            "auroc": skm.roc_auc_score(yn, pn), "auprc": skm.average_precision_score(yn, pn)}
    for k, v in want.items():
        assert abs(got[k].item() - v) <= 1e-6, (k, got[k].item(), v)
    assert got["cm"].tolist() == skm.confusion_matrix(yn, hard, labels=[0, 1]).tolist()


def test_binary_metrics_zero_division_and_single_class():
    p = torch.tensor([0.1, 0.2, 0.3, 0.2])
    got = M.binary_metrics(p, torch.zeros(4))
    assert got["precision"].item() == 0 and got["recall"].item() == 0 and got["f1"].item() == 0
    assert got["specificity"].item() == 1 and got["auroc"].item() == 0 and got["auprc"].item() == 0
    got = M.binary_metrics(p, torch.ones(4))
    assert got["auroc"].item() == 0 and got["auprc"].item() == 1 and got["specificity"].item() == 0


def test_pearson_against_scipy():
    from scipy.stats import pearsonr
    p, _ = _data(2)
    y = p * 0.5 + torch.randn(len(p), generator=torch.Generator().manual_seed(3))
    assert abs(M.pearson(p, y).item() - pearsonr(p.double().numpy(), y.double().numpy())[0]) <= 1e-6


@pytest.mark.parametrize("model", ["linear", "mlp"])
def test_host_rng_order_matches_reference_loop(model):
    """initial weights and every epoch's permutation, bitwise, against a real DataLoader over the tensors in the reference's
    order (manual_seed, next(iter(train_dl)), the model, then per epoch a shuffled train and an eval iterator)"""
    from torch.utils.data import DataLoader, Dataset
    n, ne, D, B, epochs = 2500, 700, 16, 1024, 3

    class Rows(Dataset):          # row i holds the value i, so the batches name the rows they carry
        def __init__(self, n):
            self.e = torch.arange(n, dtype=torch.float32)[:, None].repeat(1, D)
            self.l = torch.zeros(n)

        def __len__(self):
            return n if self is rows_t else ne

        def __getitem__(self, i):
            return self.e[i], self.l[i]

    rows_t, rows_e = Rows(n), Rows(ne)
    torch.manual_seed(42)
    tdl, edl = DataLoader(rows_t, batch_size=B, shuffle=True), DataLoader(rows_e, batch_size=B)
    next(iter(tdl))
    ref = P.build_module(model, D, 8, 1, 0.1)
    ref_perms = []
    for _ in range(epochs):
        ref_perms.append(torch.cat([e[:, 0].long() for e, _ in tdl]))
        for _ in edl:
            pass
    torch.manual_seed(42)
    sm = P.EpochSampler(n, ne, B)
    sm.first_batch()
    mine = P.build_module(model, D, 8, 1, 0.1)
    for a, b in zip(ref.parameters(), mine.parameters()):
        assert torch.equal(a, b)
    for e in range(epochs):
        assert torch.equal(sm.draw(), ref_perms[e])
    flat = P.ProbeParams(mine, "cpu")
    assert [tuple(p.shape) for p in flat.parameters()] == [tuple(p.shape) for p in ref.parameters()]
    assert torch.equal(flat.flat, torch.cat([p.detach().reshape(-1) for p in ref.parameters()]))


def test_get_rank_restates_reference():
    g = torch.Generator().manual_seed(4)
    x = torch.round(torch.randn(40, 90, generator=g) * 2) / 2          # ties: equal entries never count
    idx = torch.randint(0, 90, (40,), generator=g)
    want = torch.tensor([int((x[i] > x[i, idx[i]]).sum()) for i in range(40)])
    assert torch.equal(M.get_rank(x, idx.tolist()), want)


def test_hip_metrics_refuse_inputs_the_kernels_cannot_read(monkeypatch):
    """without a HIP device every HIP-backed name raises ValueError before the library is called (the kernels read device
    memory only: a host pointer would fault the GPU); a ``device`` that is not a HIP device is refused the same way"""
    hip = importlib.import_module("mca-paper_amd.hip")
    calls = []
    monkeypatch.setattr(hip, "call", lambda name, *a, **k: calls.append(name))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x, mask = torch.randn(6, 4), torch.ones(6, dtype=torch.bool)
    for fn in (lambda: M.normalize_rows(x), lambda: M.uniformity(x), lambda: M.Uniformity()(x),
               lambda: M.compute_cosines(x[0], x), lambda: M.cosine_ranks(x, x, torch.arange(6)),
               lambda: M.get_rank_metrics(x, mask, x), lambda: M.get_rank_metrics(x, mask, x, device="cpu")):
        with pytest.raises(ValueError, match="cpu|HIP device"):
            fn()
    assert calls == []
    monkeypatch.undo()
    monkeypatch.setattr(hip, "call", lambda name, *a, **k: calls.append(name))
    with pytest.raises(ValueError, match="not on cpu"):
        M.get_rank_metrics(x, mask, x, device="cpu")
    assert calls == []
