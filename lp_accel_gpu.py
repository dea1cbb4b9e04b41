"""Linear / MLP probe of the embeddings infer_accel_gpu.py writes, with the retrieval rank metrics (the reference's
lp_accel_gpu.py), on HIP kernels.  One process on cuda:0; logs to stdout and <output_dir>/log.jsonl (no wandb).

    python lp_accel_gpu.py <eval.yaml>

``loss_type: CE`` (softmax cross-entropy over the class indices of label column ``task``) takes the class count from the YAML key
``num_classes`` when present, else from the largest train label, and logs the eight multiclass metrics of
``metrics.multiclass_metrics``; the reference names the case but its label handling cannot run it.

Deviation from the reference: the rank block ranks each modality's rows against the SAME split's fusion rows (row i of the
fusion embeddings is row i's positive).  The reference's call site stacks the two splits' fusion rows, which fails for
splits of different lengths, and passes the targets in the mask slot."""
import importlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
from utils.training import get_param_norm, get_grad_norm, count_parameters, move_to  # noqa: E402,F401  (the reference's imports)
from utils.config import embedding_eval_config  # noqa: E402
from utils.metrics import Alignment, Uniformity, get_rank_metrics  # noqa: E402

probe = importlib.import_module("mca-paper_amd.probe")


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("lp_accel_gpu.py runs as one process (WORLD_SIZE > 1 given)")
    config = embedding_eval_config(sys.argv[1])
    device = torch.device("cuda", 0)
    torch.manual_seed(config.seed)
    log = open(os.path.join(config.output_dir, "log.jsonl"), "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    d = config.embedding_dir          # the files infer_accel_gpu.py wrote (dicts with frozenset keys: not weights-only)
    e_train = torch.load(f"{d}/train_embeddings.pt", map_location="cpu", weights_only=False)
    m_train = torch.load(f"{d}/train_masks.pt", map_location="cpu", weights_only=False)
    s_train = torch.load(f"{d}/train_labels.pt", map_location="cpu", weights_only=False).squeeze()
    e_test = torch.load(f"{d}/eval_embeddings.pt", map_location="cpu", weights_only=False)
    m_test = torch.load(f"{d}/eval_masks.pt", map_location="cpu", weights_only=False)
    s_test = torch.load(f"{d}/eval_labels.pt", map_location="cpu", weights_only=False).squeeze()
    print(f"Shape of test labels: {s_test.shape}\nShape of train labels: {s_train.shape}", flush=True)

    # the probe's plan is settled before any work, so that an unsupported loss fails fast
    n_all = s_train.shape[1] if (config.task == -1 and s_train.dim() > 1) else 1
    n_classes = None
    if config.loss_type == "CE" and config.task != -1:
        # the class count: the YAML's num_classes (no default: the defaults are the reference's 19 keys), else the largest train label + 1
        # when that column holds class indices; a column that does not gives no count, and the plan refuses CE as it always has
        n_classes = config.get("num_classes")
        col = s_train[:, config.task].double()
        if n_classes is None and bool(((col >= 0) & (col == col.floor())).all()):
            n_classes = int(col.max()) + 1
    plan = probe.plan(config, n_all, n_classes)
    if config.task != -1:
        s_train, s_test = s_train[:, config.task], s_test[:, config.task]
    if plan is not None and plan["loss"] == "BCE":
        probe.check_binary_targets(s_train, s_test)
    if plan is not None and plan["loss"] == "CE":
        probe.check_class_targets(s_train, s_test, n_classes=plan["L"])

    if config.rank_metrics:
        ua, al = Uniformity(), Alignment()
        for k in [x for x in e_train.keys() if isinstance(x, str) and x != "fusion"]:
            print(f"Ranking embeddings for {k}.", flush=True)
            tr = get_rank_metrics(e_train[k], m_train[k], e_train["fusion"], device=device)
            te = get_rank_metrics(e_test[k], m_test[k], e_test["fusion"], device=device)
            mtr, mte = m_train[k].bool(), m_test[k].bool()
            vals = {"train_median_rank": tr[0], "train_r1": tr[1], "train_r5": tr[2], "train_r10": tr[3],
                    "test_median_rank": te[0], "test_r1": te[1], "test_r5": te[2], "test_r10": te[3],
                    "train_uniformity": ua(e_train[k][mtr].to(device)),
                    "train_alignment": al(e_train[k][mtr].to(device), e_train["fusion"][mtr].to(device)),
                    "test_uniformity": ua(e_test[k][mte].to(device)),
                    "test_alignment": al(e_test[k][mte].to(device), e_test["fusion"][mte].to(device))}
            emit({f"{k}_{x}": v.item() for x, v in vals.items()})
        emit({"train_uniformity_fusion": ua(e_train["fusion"].to(device)).item(),
              "test_uniformity_fusion": ua(e_test["fusion"].to(device)).item()})

    x_train, x_test = e_train["fusion"], e_test["fusion"]
    sampler = probe.EpochSampler(x_train.shape[0], x_test.shape[0], config.batch_size)
    first = sampler.first_batch()          # lp_accel_gpu.py:120 of the reference: one draw before the model exists
    del first
    if plan is None:
        log.close()
        sys.exit(0)
    module = probe.build_module(config.model_type, x_train.shape[1], config.hidden_size, plan["L"], config.dropout)
    steps = -(-x_train.shape[0] // config.batch_size)
    total = config.epochs * steps
    lr_at = probe.lr_schedule(config.lr_scheduler_type, config.lr, config.num_warmup_steps, total)
    p = probe.Probe(module, config.model_type, plan["loss"], x_train, s_train.float(), x_test, s_test.float(), config.batch_size,
                    config.lr, lr_at, total, config.clip, config.dropout, config.seed, device)
    perm = sampler.draw()
    for epoch in range(config.epochs):
        p.train_epoch(perm)
        p.eval_epoch()
        vals = p.epoch_device_values()
        if epoch + 1 < config.epochs:
            perm = sampler.draw()          # the next epoch's host draws overlap this epoch's kernels
        rec = probe.Probe.read(vals)
        rec["lr"] = config.lr * lr_at(p.step)
        emit({k: rec[k] for k in ["train_loss", "eval_loss", "lr", "param_norm", "grad_norm"] +
              [k for k in rec if k.startswith("train_") and k != "train_loss"] +
              [k for k in rec if k.startswith("eval_") and k != "eval_loss"]})
    log.close()


if __name__ == "__main__":
    main()
