"""Times the gradient-cached step (mca-paper_amd/cached.py) and the two contrastive-loss kernels, in ONE process, and prints ONE JSON
line:

  * loss_ms: mca_contrastive_fwd_bwd ("dense") and mca_contrastive_stream_fwd_bwd ("stream") at B = 128, 256, 1024, 4096 with the CMU
    schedule (14 terms, D = 512), random pooled rows at production magnitude, HIP events around each call;
  * step_ms: the CMU training step at micro-batch 32: the plain eager step (forward, backward, clip, FusedAdamW) and CachedStep for
    n = 1, 2, 4, 8 and 128 chunks (B = 32 n; n = 128 cycles through the 8 distinct micro-batches), with the loss kernel "auto" picks and its share of the step;
  * forwards / backwards per cached step, for the expectation (2n - 1) forwards + n backwards.

    python tools/bench_cached_step.py [--steps 5] [--warmup 2]

The numbers go into profiles/cached_step.md."""
import argparse
import importlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
P = importlib.import_module("mca-paper_amd")
hip = importlib.import_module("mca-paper_amd.hip")
optim = importlib.import_module("mca-paper_amd.optim")
cached = importlib.import_module("mca-paper_amd.cached")


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def loss_table(eng, sizes, warmup, iters):
    rows = {}
    for B in sizes:
        g = torch.Generator(device="cuda").manual_seed(B)
        bank = torch.randn(B, eng.R, eng.D, device="cuda", generator=g) * 0.4
        present = torch.full((B,), (1 << eng.M) - 1, dtype=torch.int32, device="cuda")
        rows[str(B)] = {k: round(timed(lambda k=k: eng.loss_fwd_bwd_bank(bank, present, k), warmup, iters), 3) for k in ("dense", "stream")}
        del eng._ws[("lossws", B)]          # the dense workspace of this size: 14 B^2 floats
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--micro-batch", type=int, default=32)
    ap.add_argument("--chunks", type=int, nargs="*", default=[1, 2, 4, 8, 128],
                    help="chunks per cached step; beyond 8 the step reuses the 8 distinct micro-batches in turn (the work is the same)")
    ap.add_argument("--loss-sizes", type=int, nargs="*", default=[128, 256, 1024, 4096])
    args = ap.parse_args()
    mb = args.micro_batch
    cfg = P.config.cmu_model_config(batch_size=mb)
    torch.manual_seed(0)
    model = P.build_model(cfg).cuda()
    eng = model.engine
    eng.check_finite = "deferred"
    opt = optim.FusedAdamW(model, lr=1e-4)
    rec = {"tool": "bench_cached_step", "micro_batch": mb, "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "terms": eng.n_terms, "R": eng.R, "D": eng.D}
    rec["loss_ms"] = loss_table(eng, args.loss_sizes, 1, 3)
    rec["auto_from_B"] = next(B for B in range(1, 1 << 20) if eng.loss_kernel_for(B) == "stream")
    if not args.chunks:          # --chunks with no value: the kernel table alone
        print(json.dumps(rec))
        return
    nmax = min(max(args.chunks), 8)
    batch = {k: {kk: vv.cuda() for kk, vv in v.items()} for k, v in P.data.synthetic_batch(cfg, mb * nmax, seed=11, lengths="full").items()}
    first = cached._rows(batch, 0, mb)

    def plain():
        out = model(first)
        opt.zero_grad()
        out["loss"].backward()
        optim.clip_grad_norm_(model, 2.0)
        opt.step()

    def forward_only():
        with torch.no_grad():
            eng.forward_chunk(first, 0)

    step_ms = {"plain_b%d" % mb: round(timed(plain, args.warmup, args.steps), 3), "forward_b%d" % mb: round(timed(forward_only, args.warmup, args.steps), 3)}
    for n in args.chunks:
        cs = cached.CachedStep(model, opt, mb, clip=2.0)
        sub = cached._rows(batch, 0, mb * n) if n <= nmax else [cached._rows(batch, (i % nmax) * mb, (i % nmax + 1) * mb) for i in range(n)]
        ms = timed(lambda: cs.step(sub), *((args.warmup, args.steps) if n <= nmax else (1, 2)))
        B = mb * n
        g = torch.Generator(device="cuda").manual_seed(B)
        bank = torch.randn(B, eng.R, eng.D, device="cuda", generator=g) * 0.4
        present = torch.full((B,), (1 << eng.M) - 1, dtype=torch.int32, device="cuda")
        loss_ms = timed(lambda: eng.loss_fwd_bwd_bank(bank, present, cs.last_kernel), 1, 3)
        plan = cached.pass_plan(n)
        step_ms["cached_n%d" % n] = {"B": B, "ms": round(ms, 3), "loss_kernel": cs.last_kernel, "loss_ms": round(loss_ms, 3),
                                     "forwards": sum(k == "forward" for k, _ in plan), "backwards": sum(k == "backward" for k, _ in plan)}
    rec["step_ms"] = step_ms
    eng.assert_finite()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
