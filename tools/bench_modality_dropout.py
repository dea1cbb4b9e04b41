"""Times the per-step modality dropout (FusionEngine.set_modality_dropout) at the CMU shapes (b = 32, N = 2538) and prints ONE JSON
line, the one profiles/modality_dropout.md quotes:

  * pack_us: HIP-event time of mca_pack_masks, of mca_pack_masks_drop and of mca_counter_add, interleaved in one process
    (rounds in alternating order, the median over the rounds; every form is its own launch alone);
  * step_ms: the replayed CMU training step (graph.GraphedStep, full-length synthetic batch) with every modality's rate at
    0 (the feature off) / 1e-9 (the feature on, the two extra nodes in the graph, and no drop in practice: a 24-bit uniform is
    below 1e-9 only when it is 0) / 0.2 / 0.4, each measurement in a process of its own, the rates in alternating order
    (up, down, up, ...), with the realised drop fraction of as many replays after the timed ones.

    python tools/bench_modality_dropout.py [--rounds 2] [--steps 20] [--batch 32]

The parent process never touches the GPU; it starts one child per measurement (--child kernels | --child step --rate R)."""
import argparse
import importlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
RATES = (0.0, 1e-9, 0.2, 0.4)


def median(v):
    return sorted(v)[len(v) // 2]


def child_kernels(args):
    import ctypes as C
    import torch
    P = importlib.import_module("mca-paper_amd")
    H = importlib.import_module("mca-paper_amd.hip"); H.lib()
    cfg = P.config.cmu_model_config(batch_size=args.batch)
    b, F = args.batch, cfg["num_fusion_tokens"]
    dims = [e["max_tokens"] for e in cfg["encoder_configs"].values()]
    N = sum(dims) + F
    batch = P.data.synthetic_batch(cfg, b, seed=1234, lengths="uniform", p_drop=0.2, device="cuda")
    masks = [v["attention_mask"].to(torch.uint8).contiguous() for v in batch.values()]
    rowm = [torch.empty(b * n, device="cuda", dtype=torch.uint8) for n in dims]
    pk, off = H.PackMasksArgs(), 0
    for i, (mk, n) in enumerate(zip(masks, dims)):
        d = pk.m[i]
        d.mask, d.elem_bytes, d.n, d.offset, d.rowmask = mk.data_ptr(), 1, n, off, rowm[i].data_ptr()
        off += n
    pk.n_mod, pk.batch, pk.n_tokens, pk.n_fusion = len(dims), b, N, F
    da = H.ModalityDropArgs()
    for i in range(len(dims)):
        da.p[i] = 0.2
    da.seed, da.sample0, da.keep_one = 42, 0, 1
    padding = torch.empty(b, N, device="cuda", dtype=torch.uint8)
    present, dropped = torch.empty(b, device="cuda", dtype=torch.int32), torch.empty(b, device="cuda", dtype=torch.int32)
    step = torch.zeros(1, device="cuda", dtype=torch.int64)
    S = H.stream_ptr
    forms = {"mca_pack_masks": lambda: H.call("mca_pack_masks", C.byref(pk), padding.data_ptr(), present.data_ptr(), S()),
             "mca_pack_masks_drop": lambda: H.call("mca_pack_masks_drop", C.byref(pk), C.byref(da), step.data_ptr(), padding.data_ptr(),
                                                   present.data_ptr(), dropped.data_ptr(), S()),
             "mca_counter_add": lambda: H.call("mca_counter_add", step.data_ptr(), 1, S())}

    def timed(fn, reps=50):
        for _ in range(5):
            fn()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record(); torch.cuda.synchronize()
        return s.elapsed_time(e) / reps * 1e3

    rows = {k: [] for k in forms}
    for p in range(args.pairs):
        for k in (list(forms) if p % 2 == 0 else list(forms)[::-1]):
            rows[k].append(timed(forms[k]))
    print(json.dumps({"pack_us": {k: {"median": round(median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in rows.items()},
                      "pairs": args.pairs, "b": b, "N": N, "device": torch.cuda.get_device_name(0)}))


def child_step(args):
    import torch
    P = importlib.import_module("mca-paper_amd")
    optim = importlib.import_module("mca-paper_amd.optim")
    graph = importlib.import_module("mca-paper_amd.graph")
    cfg = P.config.cmu_model_config(batch_size=args.batch)
    torch.manual_seed(43)
    model = P.MCA(**cfg).cuda()
    model.engine.check_finite = "deferred"
    opt = optim.FusedAdamW(model, lr=1e-4)
    batch = P.data.synthetic_batch(cfg, args.batch, seed=1234, lengths="full", device="cuda")
    if args.rate > 0:
        model.engine.set_modality_dropout({n: args.rate for n in model.modality_types}, seed=42, keep_one=True, step=0)
    g = graph.GraphedStep(model, opt, batch, clip=2.0)
    for _ in range(5):
        g.step()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    frac = torch.zeros((), device="cuda")
    s.record()
    for _ in range(args.steps):
        g.step()
    e.record(); torch.cuda.synchronize()
    ms = s.elapsed_time(e) / args.steps
    if args.rate > 0:          # the realised fraction, off the clock: that of as many further replays
        for _ in range(args.steps):
            g.step()
            frac += g.out["modality_dropped"].float().mean()
        torch.cuda.synchronize()
    model.engine.assert_finite()
    print(json.dumps({"rate": args.rate, "step_ms": round(ms, 3), "dropped_fraction": round(float(frac) / args.steps, 4),
                      "loss": float(g.loss)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["kernels", "step"])
    ap.add_argument("--rate", type=float, default=0.0)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    if args.child == "kernels":
        return child_kernels(args)
    if args.child == "step":
        return child_step(args)

    def run(*extra):
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--pairs", str(args.pairs), "--batch", str(args.batch), *extra]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:          # a failed measurement ends the tool: nothing more is started on the GPU
            raise SystemExit(f"{' '.join(extra)} failed ({r.returncode}):\n{r.stderr[-3000:]}")
        return json.loads(r.stdout.strip().splitlines()[-1])

    res = run("--child", "kernels")
    steps = {r: [] for r in RATES}
    for rd in range(args.rounds):
        for r in (RATES if rd % 2 == 0 else RATES[::-1]):
            steps[r].append(run("--child", "step", "--rate", str(r)))
    res["step_ms"] = {str(r): {"runs": [x["step_ms"] for x in v], "median": median([x["step_ms"] for x in v]),
                               "dropped_fraction": v[0]["dropped_fraction"]} for r, v in steps.items()}
    res.update(rounds=args.rounds, steps=args.steps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
