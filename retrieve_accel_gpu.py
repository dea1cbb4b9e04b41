"""Top-k retrieval and kNN readout over the embeddings infer_accel_gpu.py writes, on the HIP top-k kernel.  One process on
cuda:0; logs to stdout and <output_dir>/log.jsonl, and saves the neighbour lists to <output_dir>/retrieval.pt.

    python retrieve_accel_gpu.py <eval.yaml>

The YAML is lp_accel_gpu.py's (``embedding_dir``, ``output_dir``, ``task``, ``loss_type``, ...), with two optional keys:
``retrieval_k`` (10) and ``knn_k`` (10), both at most 64.

Cross-modal retrieval, per split and ordered pair of embedding names a != b: the queries are a's rows of the samples that have
both, the gallery b's rows of the samples that have b, the positive of a query its own sample; ``{split}_{a}_to_{b}_hit1`` /
``_hit5`` / ``_hit10`` are the fractions of queries whose positive is among the first 1 / 5 / 10 neighbours, ``_n`` the queries.

kNN readout (skipped when ``task`` is -1), per name: the gallery is the train rows that have it, the queries the eval rows that
have it, the prediction the mean label of the ``knn_k`` nearest train rows; ``knn_{name}_{metric}`` are the probe's binary
metrics (``loss_type`` BCE, 0/1 labels) or ``pearson`` (L1 / MSE)."""
import importlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
from utils.config import embedding_eval_config  # noqa: E402
from utils.metrics import cosine_topk, knn_predict, hits_at  # noqa: E402

metrics = importlib.import_module("mca-paper_amd.metrics")
probe = importlib.import_module("mca-paper_amd.probe")


def presence(masks, name, n):
    """true = the sample has ``name`` (as lp_accel_gpu.py reads the masks); a name without a mask is present everywhere"""
    return masks[name].reshape(-1).bool() if name in masks else torch.ones(n, dtype=torch.bool)


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("retrieve_accel_gpu.py runs as one process (WORLD_SIZE > 1 given)")
    config = embedding_eval_config(sys.argv[1])
    retrieval_k, knn_k = int(config.get("retrieval_k", 10)), int(config.get("knn_k", 10))
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    log = open(os.path.join(config.output_dir, "log.jsonl"), "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    d = config.embedding_dir          # the files infer_accel_gpu.py wrote (dicts with frozenset keys: not weights-only)
    load = lambda name: torch.load(f"{d}/{name}.pt", map_location="cpu", weights_only=False)
    emb = {"train": load("train_embeddings"), "eval": load("eval_embeddings")}
    msk = {"train": load("train_masks"), "eval": load("eval_masks")}
    lab = {"train": load("train_labels").squeeze(), "eval": load("eval_labels").squeeze()}
    names = [k for k in emb["train"].keys() if isinstance(k, str)]
    saved = {"retrieval": {"train": {}, "eval": {}}, "knn": {}}

    def keep(query, scores, indices):
        return {"query": query.clone(), "index": indices.to(device="cpu", dtype=torch.int32), "score": scores.cpu()}

    k = max(10, retrieval_k)
    for split in ("train", "eval"):
        e = emb[split]
        for a in names:
            for b in names:
                if a == b:
                    continue
                n = e[a].shape[0]
                pa, pb = presence(msk[split], a, n), presence(msk[split], b, n)
                sel = torch.nonzero(pa & pb).reshape(-1)
                rec = {f"{split}_{a}_to_{b}_n": int(sel.numel())}
                if sel.numel():
                    scores, indices = cosine_topk(e[a], e[b], k, query_index=sel, target_mask=pb, device=device)
                    for m in (1, 5, 10):
                        rec[f"{split}_{a}_to_{b}_hit{m}"] = hits_at(indices, sel.to(device), m).float().mean().item()
                    saved["retrieval"][split][f"{a}_to_{b}"] = keep(sel, scores, indices)
                emit(rec)

    if config.task == -1:
        print("kNN readout skipped: task is -1 (no single label column)", flush=True)
    else:
        if config.loss_type not in ("BCE", "L1", "MSE"):
            raise NotImplementedError(f"loss_type {config.loss_type}: the kNN readout scores BCE, L1 and MSE tasks")
        y_train, y_eval = lab["train"][:, config.task].float(), lab["eval"][:, config.task].float()
        if config.loss_type == "BCE":
            probe.check_binary_targets(y_train, y_eval)
        for name in names:
            have = presence(msk["train"], name, emb["train"][name].shape[0])
            sel = torch.nonzero(presence(msk["eval"], name, emb["eval"][name].shape[0])).reshape(-1)
            if not bool(have.any()) or sel.numel() == 0:
                print(f"kNN readout of {name} skipped: no train row or no eval row has it", flush=True)
                continue
            scores, indices = cosine_topk(emb["eval"][name], emb["train"][name], knn_k, query_index=sel, target_mask=have, device=device)
            pred = knn_predict(scores, indices, y_train.to(device))
            target = y_eval[sel].to(device)
            if config.loss_type == "BCE":
                vals = metrics.binary_metrics(pred, target)
            else:
                vals = {"pearson": metrics.pearson(pred, target)}
            emit({f"knn_{name}_{m}": (v.tolist() if v.dim() else v.item()) for m, v in vals.items()})
            saved["knn"][name] = dict(keep(sel, scores, indices), pred=pred.cpu())
    torch.save(saved, os.path.join(config.output_dir, "retrieval.pt"))
    log.close()


if __name__ == "__main__":
    main()
