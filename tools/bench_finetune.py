"""Times the supervised fine-tune step (mca-paper_amd/finetune.py) on the CMU model against the plain eager step, in ONE process, and
prints ONE JSON line.  Per batch size (32 and 8):

  * plain_ms        forward_backward + clip_grad_norm_ + FusedAdamW, eager (not the replayed graph): the pretraining step
  * ft_task_ms      FineTuneStep with contrastive_weight 0: no contrastive loss, the task head kernel instead
  * ft_multi_ms     FineTuneStep with contrastive_weight 1: both losses
  * head_kernel_ms  mca_task_head_fwd_bwd alone (its two launches) on the step's pooled tokens, for a head of 1 and of 7 outputs
  * the two ratios ft_task / plain and head_kernel / ft_task

The three steps are timed in turn, --rounds times, each window --steps steps between two device events after --warmup steps of every
kind; the medians over the rounds are reported, with the rounds' extremes.

    python tools/bench_finetune.py [--steps 10] [--warmup 3] [--rounds 5] [--loss MSE] [--classes 7]

--loss L1 | MSE | BCE | CE chooses the task loss of the two fine-tune steps (default MSE); with CE the head has --classes outputs over
one column of class indices (mca_class_head_fwd_bwd), head_kernel_ms is that kernel's and head_kernel_bytes what it has to move
(the readout slot, the weights, d_pooled, its workspace slots twice, gw), and probe_head_ce_ms / probe_head_ce_bytes time
mca_probe_head_ce_f32 alone on 4096 rows of 1024 features.

The numbers go into profiles/finetune_step.md and profiles/class_head.md."""
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


def telemetry(fn, steps=60):
    """the GPU's clock and power while `steps` calls of fn are in flight, read with rocm-smi (a query, nothing is set); None
    where the tool or a field is missing"""
    import subprocess
    for _ in range(steps):
        fn()
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=60)
        card = next(iter(json.loads(r.stdout).values()))
        out = {k: v for k, v in card.items() if "sclk" in k.lower() or "mclk" in k.lower() or "power" in k.lower()}
    except Exception as e:          # noqa: BLE001  (a missing tool must not end the measurement)
        out = {"error": f"{type(e).__name__}: {e}"[:200]}
    torch.cuda.synchronize()
    return out


def one_size(b, args):
    cfg = P.config.cmu_model_config(batch_size=b)
    torch.manual_seed(0)
    model = P.build_model(cfg).cuda()
    eng = model.engine
    eng.check_finite = "deferred"
    opt = optim.FusedAdamW(model, lr=1e-4)
    batch = {k: {kk: vv.cuda() for kk, vv in v.items()} for k, v in P.data.synthetic_batch(cfg, b, seed=11, lengths="full").items()}
    labels = torch.randn(b, 7, generator=torch.Generator().manual_seed(5))
    ce = args.loss == "CE"
    if args.loss == "BCE":
        labels = (labels > 0).float()
    if ce:
        labels[:, 0] = torch.randint(0, args.classes, (b,), generator=torch.Generator().manual_seed(6)).float()
    labels = labels.cuda()
    n_out = args.classes if ce else 1
    task = finetune.FineTuneStep(model, finetune.TaskHead(cfg["dim"], n_out), opt, task=0, clip=2.0, loss_type=args.loss)
    multi = finetune.FineTuneStep(model, finetune.TaskHead(cfg["dim"], n_out), opt, task=0, clip=2.0, contrastive_weight=1.0, loss_type=args.loss)
    wide = None if ce else finetune.FineTuneStep(model, finetune.TaskHead(cfg["dim"], 7), opt, task=-1, clip=2.0, loss_type=args.loss)

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
    rec = {"b": b, "loss": args.loss, "head_outputs": n_out, "telemetry_during_ft_task": telemetry(kinds["ft_task_ms"])}
    for k, v in times.items():
        rec[k] = round(statistics.median(v), 4)
        rec[k + "_range"] = [round(min(v), 4), round(max(v), 4)]
    # the kernel alone, on the pooled tokens and presence words the last step left in the workspace
    with torch.no_grad():
        ws, pooled, _ = eng.forward_chunk(batch, 0)
    for name, st in (("head_kernel_ms", task),) + ((("head_kernel_L7_ms", wide),) if wide is not None else ()):
        y, off, ld = st._label_window(labels)
        call = lambda st=st, y=y, off=off, ld=ld: st._task_kernel(pooled, ws["present_cur"], b, y, off, ld, None, 0.0)
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        rec[name] = round(statistics.median(window(call, 200) for _ in range(args.rounds)), 5)
    if ce:
        D, R, nblk = cfg["dim"], eng.R, (b + 63) // 64
        rec["head_kernel_bytes"] = 4 * (b * D + n_out * D + b * R * D + 2 * nblk * (n_out * D + n_out + 4) + n_out * D + b * n_out)
    rec["ft_task_over_plain"] = round(rec["ft_task_ms"] / rec["plain_ms"], 4)
    rec["ft_multi_over_plain"] = round(rec["ft_multi_ms"] / rec["plain_ms"], 4)
    rec["head_kernel_share_of_ft_task"] = round(rec["head_kernel_ms"] / rec["ft_task_ms"], 5)
    eng.assert_finite()
    return rec


def probe_head_ce(args, B=4096, K=1024):
    """mca_probe_head_ce_f32 alone: B rows of K features, --classes classes, with dz and da (the MLP probe's call)"""
    hip = importlib.import_module("mca-paper_amd.hip")
    C = args.classes
    g = torch.Generator().manual_seed(1)
    a, w, bias = torch.randn(B, K, generator=g).cuda(), (torch.randn(C, K, generator=g) / 32).cuda(), torch.zeros(C).cuda()
    y = torch.randint(0, C, (B,), generator=g).float().cuda()
    pred, dz, da = torch.empty(B, C).cuda(), torch.empty(B, C).cuda(), torch.empty(B, K).cuda()
    part = torch.empty(hip.lib().mca_probe_head_blocks(B)).cuda()
    call = lambda: hip.call("mca_probe_head_ce_f32", a.data_ptr(), K, None, K, w.data_ptr(), bias.data_ptr(), C, y.data_ptr(), 1, None, B,
                            pred.data_ptr(), dz.data_ptr(), da.data_ptr(), 1.0, part.data_ptr(), hip.stream_ptr())
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    return {"probe_head_ce_rows": B, "probe_head_ce_features": K, "probe_head_ce_ms": round(statistics.median(window(call, 200) for _ in range(args.rounds)), 5),
            "probe_head_ce_bytes": 4 * (2 * B * K + C * K + 2 * B * C + B)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch-sizes", type=int, nargs="*", default=[32, 8])
    ap.add_argument("--loss", choices=["L1", "MSE", "BCE", "CE"], default="MSE")
    ap.add_argument("--classes", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune.py measures on the GPU and found none")
    rec = {"tool": "bench_finetune", "model": "CMU", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "sizes": [one_size(b, args) for b in args.batch_sizes]}
    if args.loss == "CE":
        rec.update(probe_head_ce(args))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
