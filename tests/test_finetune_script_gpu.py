"""finetune_accel_gpu.py end to end on a tiny config with --synthetic 6, in a child process: exit status, the per-epoch records, the
saved state, and a second run that restarts from it and evaluates what it loaded (the refusals need no GPU: tests/test_task_head_cpu.py)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import REPO
from util_small import small_config

pytestmark = pytest.mark.gpu
KEYS = {"epoch", "train_loss", "eval_loss", "eval_PCC", "lr", "grad_norm"}


def run(tmp_path, tag, extra=(), **keys):
    import yaml
    cfg = small_config("mca")
    mod_cfg = {name: {"type": "embedded_sequence", "pad_len": enc["max_tokens"], "embedding_size": enc["input_size"], "data_col_name": "data", "dropout": 0.2}
               for name, enc in cfg["encoder_configs"].items()}
    out = tmp_path / tag
    y = dict(encoder_configs=cfg["encoder_configs"], modality_config=mod_cfg, hidden_size=cfg["dim"], layers=cfg["depth"], heads=cfg["heads"],
             dim_head=cfg["dim_head"], num_fusion_tokens=cfg["num_fusion_tokens"], batch_size=4, fcl=cfg["fcl"], fcl_root=cfg["fcl_root"],
             bimodal_contrastive=cfg["bimodal_contrastive"], non_fusion_fcl=cfg["non_fusion_fcl"], fusion_combos=cfg["fusion_combos"],
             zorro=cfg["zorro"], eao=cfg["eao"], no_fusion=cfg["no_fusion"], mean_pool=cfg["mean_pool"], epochs=2, lr=1e-3,
             lr_scheduler_type="cosine", num_warmup_steps=1, clip=2.0, seed=7, output_dir=str(out), dataset="unused", label_col="Labels")
    y.update(keys)
    ypath = tmp_path / f"{tag}.yaml"
    ypath.write_text(yaml.safe_dump(y, sort_keys=False))
    r = subprocess.run([sys.executable, os.path.join(REPO, "finetune_accel_gpu.py"), str(ypath), "--synthetic", "6", *extra],
                       capture_output=True, text=True, timeout=600)
    return r, out


def test_finetune_script_trains_saves_and_restarts(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ft = {"task": 2, "readout": "audio", "head_lr": 5e-3, "head_warmup_steps": 2}
    r, out = run(tmp_path, "first", batch_dropout=True, finetune=ft)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "starts from the seed" in r.stdout and "batch_dropout" in r.stdout
    recs = [json.loads(l) for l in open(out / "log.jsonl")]
    assert [rec["epoch"] for rec in recs] == [0, 1]
    for rec in recs:
        assert set(rec) == KEYS, rec
        assert all(v == v and abs(v) < 1e9 for v in rec.values() if isinstance(v, float)), rec
        assert isinstance(rec["eval_PCC"], list) and len(rec["eval_PCC"]) == 1 and rec["grad_norm"] > 0 and rec["lr"] >= 0
    for f in ("model.safetensors", "optimizer.bin", "meta.json", "head_state.pt"):
        assert os.path.exists(out / f), f
    hs = torch.load(out / "head_state.pt", weights_only=True)
    assert hs["step"] == 12 and hs["head"]["head.weight"].shape == (1, 128) and float(hs["exp_avg"].abs().max()) > 0
    # a second run from that state: it evaluates what it loaded before it trains (epoch -1)
    r2, out2 = run(tmp_path, "second", restart=str(out), epochs=1, finetune=ft)
    assert r2.returncode == 0, r2.stderr[-3000:]
    assert "head_state.pt" in r2.stdout
    recs2 = [json.loads(l) for l in open(out2 / "log.jsonl")]
    assert [rec["epoch"] for rec in recs2] == [-1, 0] and all(set(rec) == KEYS for rec in recs2)
    a, b = recs[-1]["eval_loss"], recs2[0]["eval_loss"]
    print("eval_loss of the first run's last epoch", a, "and of the restarted run before training", b)
    assert abs(a - b) <= 2.0 ** -20 * abs(a), (a, b)          # the same weights and kernels: fp32 roundings of a sum at most
    assert torch.load(out2 / "head_state.pt", weights_only=True)["step"] == 18
