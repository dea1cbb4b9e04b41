"""Supervised fine-tuning of a pretrained fusion model on labels, through the native step (mca-paper_amd/finetune.py,
INTEGRATION.md section I):

    python finetune_accel_gpu.py <config.yaml> [--synthetic N]

The config is the training YAML (train_accel_gpu.py) plus a ``finetune:`` mapping: loss_type (L1 | MSE | BCE | CE, default MSE), task (a
column of ``label_col``, -1 = all columns; default 0), readout (a pooled slot: a modality name, "fusion" or a list of modality names for
a combination; default fusion), head_lr (default: lr), task_weight (1.0), contrastive_weight (0.0), head_warmup_steps (0).  Unknown
keys are an error.  loss_type CE (softmax cross-entropy; column ``task`` holds class indices, a negative one marks an unlabelled row)
adds num_classes (2 .. 64, required), class_weights (a list of num_classes weights) and label_smoothing (0.0); they are an error with
any other loss.  ``restart`` names the pretrained checkpoint (model only; a ``head_state.pt`` beside it is loaded too, and the
restored pair is evaluated once before training, logged as epoch -1); empty: training starts from the seed, and the run says so.

One linear head is trained with the trunk for ``epochs`` epochs, both learning rates on the configured schedule; after every epoch the
eval split is predicted and ONE JSON record is printed and appended to <output_dir>/log.jsonl: epoch, train_loss, eval_loss,
eval_PCC (per task column), eval_<the probe's binary metrics> or, for CE, eval_<the multiclass metrics> over the valid and labelled rows
(eval_loss is then float64 cross_entropy with the same weights and smoothing, eval_cm a nested list), lr, grad_norm.  At the end <output_dir> holds the state
(checkpoint.save_state) and head_state.pt.  --synthetic N: N random train and N random eval batches with randn (b, 7) labels
(thresholded at 0 for BCE; CE: column ``task`` drawn uniformly from 0 .. num_classes - 1).  ``batch_dropout: true`` works as in training.  grad_cache_chunks > 1 and --graph are refused."""
import importlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
P = importlib.import_module("mca-paper_amd")
optim = importlib.import_module("mca-paper_amd.optim")
cached = importlib.import_module("mca-paper_amd.cached")
finetune = importlib.import_module("mca-paper_amd.finetune")
from train_accel_gpu import lr_factor, move_to  # noqa: E402

def element_loss(pred, y, loss_type):
    """mean element loss in float64 (the evaluation's, not the step's: that one comes from the kernel)"""
    pred, y = pred.double(), y.double()
    if loss_type == "BCE":
        return torch.nn.functional.binary_cross_entropy_with_logits(pred, y)
    return ((pred - y) ** 2).mean() if loss_type == "MSE" else (pred - y).abs().mean()


def evaluate(step, batches, label_col, device):
    """predict over a split -> the record's eval_* entries, over the rows the readout is valid for"""
    preds, labels = [], []
    for batch in batches:
        y = batch.pop(label_col)["data"]
        pred, valid = step.predict(move_to(batch, device))
        y = y.to(device=device, dtype=torch.float32)
        y = y.reshape(-1, 1) if y.dim() < 2 else y.reshape(y.shape[0], -1)
        y = y if step.task < 0 else y[:, step.task:step.task + 1]
        preds.append(pred[valid]); labels.append(y[valid])
    pred, y = torch.cat(preds), torch.cat(labels)
    if step.loss_type == "CE":
        y = y[:, 0]
        keep = y >= 0          # the labelled rows
        pred, y = pred[keep], y[keep].long()
        cw = None if step.class_weights is None else step.class_weights.double()
        rec = {"eval_loss": float(torch.nn.functional.cross_entropy(pred.double(), y, weight=cw, label_smoothing=step.label_smoothing))
               if pred.numel() else None}
        if pred.numel():
            for k, v in P.metrics.multiclass_metrics(torch.softmax(pred.double(), 1), y).items():
                rec[f"eval_{k}"] = v.tolist()
        return rec
    rec = {"eval_loss": float(element_loss(pred, y, step.loss_type)) if pred.numel() else None}
    if step.loss_type == "BCE":
        for k, v in P.metrics.binary_metrics(torch.sigmoid(pred), y).items():
            rec[f"eval_{k}"] = v.tolist()
    else:
        rec["eval_PCC"] = [float(P.metrics.pearson(pred[:, j], y[:, j])) for j in range(pred.shape[1])]
    return rec


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    synthetic = int(sys.argv[sys.argv.index("--synthetic") + 1]) if "--synthetic" in sys.argv else 0
    config = P.config.training_config(sys.argv[1], make_output_dir=False)
    settings = finetune.finetune_settings(config)
    finetune.refuse_with(cached.grad_cache_chunks(config), "--graph" in sys.argv)          # (before anything touches the GPU)
    config = P.config.training_config(sys.argv[1])
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    torch.manual_seed(config.seed)
    model_config = P.config.get_model_config(config)
    modality_config = config.get("modality_config", config.get("modality_configs", {}))
    label_col = config.label_col

    # ---- data
    if synthetic:
        def split(seed0):
            for i in range(synthetic):
                b = P.data.synthetic_batch(model_config, config.batch_size, seed=seed0 + i, p_drop=0.2)
                y = torch.randn(config.batch_size, 7, generator=torch.Generator().manual_seed(seed0 + i))
                if settings["loss_type"] == "CE":
                    y[:, settings["task"]] = torch.randint(0, settings["num_classes"], (config.batch_size,),
                                                           generator=torch.Generator().manual_seed(seed0 + i)).float()
                b[label_col] = {"data": (y > 0).float() if settings["loss_type"] == "BCE" else y}
                yield b
        train_batches, eval_batches = (lambda epoch: split(100 + 1000 * epoch)), (lambda: split(10_000))
        steps_per_epoch, n_labels = synthetic, 7
    else:
        from torch.utils.data import DataLoader
        ds = P.data.setup_data(config.dataset, split=config.split, ds_frac=config.ds_frac, ds_seed=config.ds_seed,
                               predrop=bool(config.get("predrop", False)), predrop_config=modality_config)
        coll = P.MultimodalCollator(modality_config, labels=label_col)
        train_dl = DataLoader(ds["train"], collate_fn=coll, batch_size=config.batch_size, shuffle=True, num_workers=8, prefetch_factor=4,
                              drop_last=True, pin_memory=True)
        eval_dl = DataLoader(ds["test"], collate_fn=coll, batch_size=config.batch_size)
        train_batches, eval_batches = (lambda epoch: iter(train_dl)), (lambda: iter(eval_dl))
        steps_per_epoch = len(train_dl)
        first = coll([ds["train"][0]])[label_col]["data"]
        n_labels = 1 if first.dim() < 2 else first.reshape(first.shape[0], -1).shape[1]

    # ---- model, head, optimizer
    model = P.build_model(model_config).to(device)
    opt = optim.FusedAdamW(model, lr=config.lr)
    model.engine.check_finite = "deferred"
    n_outputs = settings["num_classes"] if settings["loss_type"] == "CE" else (n_labels if settings["task"] < 0 else 1)
    head = finetune.TaskHead(model_config["dim"], n_outputs)
    step = finetune.FineTuneStep(model, head, opt, clip=config.clip or 0.0, **settings)
    restored = False
    if config.restart:
        meta = P.checkpoint.load_state(config.restart, model)          # the pretrained weights: model only
        if meta.get("warnings"):
            print("\n".join(meta["warnings"]), flush=True)
        hs = os.path.join(config.restart, "head_state.pt")
        if os.path.exists(hs):
            step.load_state_dict(torch.load(hs, map_location=device, weights_only=True))
            restored = True
        print(f"restart: model from {config.restart}; head " + ("and its moments from head_state.pt" if restored else "from the seed"), flush=True)
    else:
        print("restart is empty: fine-tuning starts from the seed, not from pretrained weights", flush=True)
    drop_cfg = P.config.modality_dropout_settings(config)
    if drop_cfg is not None:
        model.engine.set_modality_dropout(drop_cfg["rates"], seed=drop_cfg["seed"], keep_one=drop_cfg["keep_one"], step=step.step_count)
        print(f"batch_dropout: {model.engine.modality_dropout}", flush=True)
    log = open(os.path.join(config.output_dir, "log.jsonl"), "a")

    def emit(rec):
        print(json.dumps(rec), flush=True)
        log.write(json.dumps(rec) + "\n"); log.flush()

    if restored:
        emit({"epoch": -1, "train_loss": None, **evaluate(step, eval_batches(), label_col, device), "lr": 0.0, "grad_norm": None})
    total_steps = config.epochs * steps_per_epoch
    head_base = settings["head_lr"]
    n = 0
    model.train()
    for epoch in range(config.start_epoch, config.epochs):
        loss_sum, steps = torch.zeros((), device=device), 0
        for batch in train_batches(epoch):
            y = batch.pop(label_col)["data"]
            step.check_labels(y)          # (BCE: targets other than 0 / 1 end the run here, before the step)
            f = lr_factor(config.lr_scheduler_type, n, config.num_warmup_steps, total_steps)
            for g in opt.param_groups:
                g["lr"] = config.lr * f
            step.head_lr = None if head_base is None else head_base * f
            out = step.step(move_to(batch, device), y.to(device, non_blocking=True))
            loss_sum += out["loss"]
            steps, n = steps + 1, n + 1
            model.engine.poll_finite()
        model.engine.assert_finite()
        emit({"epoch": epoch, "train_loss": float(loss_sum) / max(1, steps), **evaluate(step, eval_batches(), label_col, device),
              "lr": opt.param_groups[0]["lr"], "grad_norm": None if step.gnorm is None else float(step.gnorm)})
    P.checkpoint.save_state(config.output_dir, model, opt, opt.step_count)
    torch.save({k: (v.cpu() if torch.is_tensor(v) else ({kk: vv.cpu() for kk, vv in v.items()} if isinstance(v, dict) else v))
                for k, v in step.state_dict().items()}, os.path.join(config.output_dir, "head_state.pt"))
    print(f"saved the model state and head_state.pt to {config.output_dir}", flush=True)


if __name__ == "__main__":
    main()
