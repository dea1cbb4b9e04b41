"""Times the supervised fine-tune step (mca-paper_amd/finetune.py) on the CMU model against the plain eager step, in ONE process, and
prints ONE JSON line.  Per batch size (32 and 8):

  * plain_ms        forward_backward + clip_grad_norm_ + FusedAdamW, eager (not the replayed graph): the pretraining step
  * ft_task_ms      FineTuneStep with contrastive_weight 0: no contrastive loss, the task head kernel instead
  * ft_multi_ms     FineTuneStep with contrastive_weight 1: both losses
  * head_kernel_ms  mca_task_head_fwd_bwd alone (its two launches) on the step's pooled tokens, for a head of 1 and of 7 outputs
  * the two ratios ft_task / plain and head_kernel / ft_task

The three steps are timed in turn, --rounds times, each window --steps steps between two device events after --warmup steps of every
kind; the medians over the rounds are reported, with the rounds' extremes.

    python tools/bench_finetune.py [--steps 10] [--warmup 3] [--rounds 5]

The numbers go into profiles/finetune_step.md."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
P = importlib.import_module("mca-paper_amd")
optim = importlib.import_module("mca-paper_amd.optim")
finetune = importlib.import_module("mca-paper_amd.finetune")


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def one_size(b, args):
    cfg = P.config.cmu_model_config(batch_size=b)
    torch.manual_seed(0)
    model = P.build_model(cfg).cuda()
    eng = model.engine
    eng.check_finite = "deferred"
    opt = optim.FusedAdamW(model, lr=1e-4)
    batch = {k: {kk: vv.cuda() for kk, vv in v.items()} for k, v in P.data.synthetic_batch(cfg, b, seed=11, lengths="full").items()}
    labels = torch.randn(b, 7, generator=torch.Generator().manual_seed(5)).cuda()
    task = finetune.FineTuneStep(model, finetune.TaskHead(cfg["dim"], 1), opt, task=0, clip=2.0)
    multi = finetune.FineTuneStep(model, finetune.TaskHead(cfg["dim"], 1), opt, task=0, clip=2.0, contrastive_weight=1.0)
    wide = finetune.FineTuneStep(model, finetune.TaskHead(cfg["dim"], 7), opt, task=-1, clip=2.0)

    def plain():
        eng.forward_backward(batch)
        optim.clip_grad_norm_(model, 2.0)
        opt.step()

    kinds = {"plain_ms": plain, "ft_task_ms": lambda: task.step(batch, labels), "ft_multi_ms": lambda: multi.step(batch, labels)}
    for fn in kinds.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k, fn in kinds.items():
            times[k].append(window(fn, args.steps))
    rec = {"b": b}
    for k, v in times.items():
        rec[k] = round(statistics.median(v), 4)
        rec[k + "_range"] = [round(min(v), 4), round(max(v), 4)]
    # the kernel alone, on the pooled tokens and presence words the last step left in the workspace
    with torch.no_grad():
        ws, pooled, _ = eng.forward_chunk(batch, 0)
    for name, st in (("head_kernel_ms", task), ("head_kernel_L7_ms", wide)):
        y, off, ld = st._label_window(labels)
        call = lambda st=st, y=y, off=off, ld=ld: st._task_kernel(pooled, ws["present_cur"], b, y, off, ld, None, 0.0)
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        rec[name] = round(statistics.median(window(call, 200) for _ in range(args.rounds)), 5)
    rec["ft_task_over_plain"] = round(rec["ft_task_ms"] / rec["plain_ms"], 4)
    rec["ft_multi_over_plain"] = round(rec["ft_multi_ms"] / rec["plain_ms"], 4)
    rec["head_kernel_share_of_ft_task"] = round(rec["head_kernel_ms"] / rec["ft_task_ms"], 5)
    eng.assert_finite()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch-sizes", type=int, nargs="*", default=[32, 8])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune.py measures on the GPU and found none")
    rec = {"tool": "bench_finetune", "model": "CMU", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "sizes": [one_size(b, args) for b in args.batch_sizes]}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
