"""Probe-stage timings (lp_accel_gpu.py) on one GPU, one JSON line:

    python tools/bench_lp.py

rank_us: mca_cosine_rank_f32 at 16384 queries x 16384 targets x 512 (inputs normalised beforehand, not timed);
uniformity_us: ``metrics.uniformity`` at 16384 x 512 (normalisation included);
probe_ms_per_epoch_{linear,mlp}: one train + eval epoch of ``probe.Probe`` at n = 16384 train / 4096 eval rows, B = 1024,
D = 512, H = 256, L = 1, L1 loss, the log record read back;
eager_ms_per_epoch_{linear,mlp}: the same epoch as a torch-eager restatement of the reference's loop (loss read to the host
every step, clip_grad_norm_, torch AdamW, LambdaLR; without torchmetrics, which this project does not carry)."""
import importlib
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


HIP_ATTR_CLOCK_RATE = 5          # hipDeviceAttributeClockRate (hip_runtime_api.h): peak shader clock in kHz


def _peak_sclk_mhz(device: int = 0) -> float:
    """the box's peak shader clock from the HIP runtime torch already loaded (torch on ROCm exposes no clock_rate)"""
    import ctypes
    import glob
    names = ["libamdhip64.so"] + sorted(glob.glob(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so*")))
    for name in names:
        try:
            lib = ctypes.CDLL(name)
        except OSError:
            continue
        v = ctypes.c_int(0)
        if lib.hipDeviceGetAttribute(ctypes.byref(v), HIP_ATTR_CLOCK_RATE, device) == 0:
            return v.value / 1000.0
    raise RuntimeError("hipDeviceGetAttribute(hipDeviceAttributeClockRate) is not available")


def _events_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    out.sort()
    return out[len(out) // 2]


def _wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    out.sort()
    return out[len(out) // 2]


def main():
    importlib.import_module("mca-paper_amd.build").build(verbose=False)
    M = importlib.import_module("mca-paper_amd.metrics")
    P = importlib.import_module("mca-paper_amd.probe")
    hip = importlib.import_module("mca-paper_amd.hip")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    n, d = 16384, 512
    q = M.normalize_rows(torch.randn(n, d, device=dev, generator=g))
    t = M.normalize_rows(torch.randn(n, d, device=dev, generator=g))
    s_true = torch.empty(n, device=dev)
    ranks = torch.empty(n, dtype=torch.int32, device=dev)

    def rank():
        hip.call("mca_cosine_rank_f32", q.data_ptr(), d, None, n, t.data_ptr(), d, n, d, s_true.data_ptr(), ranks.data_ptr(), hip.stream_ptr())
    for _ in range(3):
        rank()
    rank_ms = _events_ms(rank, 10)
    x = torch.randn(n, d, device=dev, generator=g)
    for _ in range(3):
        M.uniformity(x)
    unif_ms = _events_ms(lambda: M.uniformity(x), 10)

    rec = {"what": "bench_lp", "device": torch.cuda.get_device_name(0),
           "sclk_mhz_max": _peak_sclk_mhz(0),
           "rank_us": round(rank_ms * 1e3, 1), "rank_tflops": round(2 * n * n * d / rank_ms / 1e9, 1),
           "uniformity_us": round(unif_ms * 1e3, 1)}
    B, H, ne = 1024, 256, 4096
    xt, xe = torch.randn(n, d), torch.randn(ne, d)
    w = torch.randn(d)
    yt, ye = xt @ w / 20, xe @ w / 20
    lf = importlib.import_module("train_accel_gpu").lr_factor
    for model in ("linear", "mlp"):
        torch.manual_seed(0)
        epochs = 12
        total = epochs * (n // B)
        lam = lambda s: lf("cosine", s, 100, total)
        sm = P.EpochSampler(n, ne, B)
        sm.first_batch()
        mod = P.build_module(model, d, H, 1, 0.1)
        pr = P.Probe(mod, model, "L1", xt, yt, xe, ye, B, 1e-4, lam, total, 2.0, 0.1, 0, dev)
        perms = [sm.draw() for _ in range(epochs)]

        def epoch(i=[0]):
            pr.train_epoch(perms[i[0] % epochs])
            pr.eval_epoch()
            P.Probe.read(pr.epoch_device_values())
            i[0] += 1
        for _ in range(2):
            epoch()
        rec[f"probe_ms_per_epoch_{model}"] = round(_wall_ms(epoch, 9), 3)
        # the reference's loop in torch eager
        ref = P.build_module(model, d, H, 1, 0.1).to(dev)
        opt = torch.optim.AdamW(ref.parameters(), lr=1e-4)
        sch = torch.optim.lr_scheduler.LambdaLR(opt, lam)
        lossf = torch.nn.L1Loss()
        xtd, ytd, xed, yed = xt.to(dev), yt.to(dev), xe.to(dev), ye.to(dev)

        def eager_epoch():
            perm = torch.randperm(n)
            tl = torch.zeros(1)
            ref.train()
            for s in range(0, n, B):
                idx = perm[s:s + B].to(dev)
                z = ref(xtd[idx]).squeeze()
                loss = lossf(z, ytd[idx])
                opt.zero_grad()
                loss.backward()
                tl += loss.detach().cpu()
                torch.nn.utils.clip_grad_norm_(ref.parameters(), 2.0)
                opt.step()
                sch.step()
            ref.eval()
            el = torch.zeros(1)
            with torch.no_grad():
                for s in range(0, ne, B):
                    el += lossf(ref(xed[s:s + B]).squeeze(), yed[s:s + B]).detach().cpu()
        for _ in range(2):
            eager_epoch()
        rec[f"eager_ms_per_epoch_{model}"] = round(_wall_ms(eager_epoch, 9), 3)
    rec["utc"] = time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime())
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
