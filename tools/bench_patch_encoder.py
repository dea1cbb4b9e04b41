"""The PatchEncoder front-end kernel and a step with a matrix modality, one GPU, one JSON line:

    python tools/bench_patch_encoder.py [--batch 32] [--steps 20] [--profile profiles/patch_encoder.md]

kernel: `mca_patch_ln_fwd` at b = BATCH, 1024 x 128 matrices in 16 x 16 patches (512 tokens, P = 256), with xp.  The figure is the
median over 30 rounds of (device-event time around 20 launches) / 20 after warm-up; beside it the bytes the algorithm moves (values
read once, xp and xn_bf16 written, three small vectors) and the time those bytes take at the HBM rate a float4 copy reaches on this
chip (6.29 TB/s; docs/kernels.md), the kernel's floor; then the A/B forms of knob 13 (staged with smaller spans, and the
wavefront-per-patch form that reads global memory directly) at 16 x 16 and at 64 x 4 patches.  The inputs of consecutive launches rotate over four buffer sets (160 MiB at
b = 32), so that a launch does not find its matrix in the cache the previous one left it in.
step: the CMU model with `FACET` replaced by a 512-token PatchEncoder over such matrices, eager loop (forward, backward, clip,
FusedAdamW), natively and with the encoder as the torch twin of tests/patch_twin.py (through ForeignStep and autograd, the way a
matrix modality had to run before).  A/B in ALTERNATING PROCESSES: this process starts one fresh child per window (native, twin,
native, twin, native, twin); each child warms up 5 steps and times STEPS steps with a host clock around a device synchronise.
Clock and power: `rocm-smi --showclocks --showpower` read once before and once after (read-only), kept in the JSON line.
--profile: also writes the figures as a markdown page (the default bench line against the parent commit is measured separately).

    python tools/bench_patch_encoder.py --mode image|video [--profile profiles/patch_nd_encoder.md]

kernel: `mca_patch_nd_ln_fwd` in both forms - images 3 x 224 x 224 in 16 x 16 patches (196 tokens, P = 768) and clips 3 x 8 x 112 x 112
in (2, 8, 8) tubelets (784 tokens, P = 384) - measured and set against their floors as above, beside `mca_patch_ln_fwd` at 1024 x 128
from the same run.  step: the CMU model with `FACET` replaced by such an image (--mode image) or video (--mode video) modality,
natively and with the torch twin of tests/patch_nd_twin.py, in the same alternating windows; the page states the native mean against
the twin's and the spread (max - min) of the twin's own windows."""
import argparse
import copy
import importlib
import json
import os
import subprocess
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
H_, W_, P1, P2, D = 1024, 128, 16, 16, 512
COPY_TB_S = 6.29          # float4 copy on an MI355X


def median_us(fn, per=20, rounds=30, warm=3):
    for _ in range(warm * per):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(rounds)]
    for s, e in evs:
        s.record()
        for _ in range(per):
            fn()
        e.record()
    torch.cuda.synchronize()
    t = sorted(s.elapsed_time(e) for s, e in evs)
    return t[len(t) // 2] * 1e3 / per


def kernel_us(H, b, p1, p2, knobs):
    """-> {knob 13 value: us} of `mca_patch_ln_fwd` over b matrices of H_ x W_ in (p1, p2) patches, with xp"""
    n, P = (H_ // p1) * (W_ // p2), p1 * p2
    rows = b * n
    g = torch.Generator(device="cuda").manual_seed(0)
    gamma, beta = torch.randn(P, generator=g, device="cuda"), torch.randn(P, generator=g, device="cuda")
    sets = []
    for _ in range(4):
        v = torch.randn(b, H_, W_, generator=g, device="cuda")
        v[:, H_ // 2:] = -10000.0          # half of the rows padded: those patches take the all-pad path
        sets.append((v, torch.empty(rows, P, device="cuda"), torch.empty(rows, P, dtype=torch.bfloat16, device="cuda"),
                     torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda"), torch.empty(rows, dtype=torch.uint8, device="cuda")))
    k = [0]

    def fn():
        v, xp, xn, m, r, pm = sets[k[0] % 4]
        k[0] += 1
        H.call("mca_patch_ln_fwd", v.data_ptr(), H_ * W_, W_, b, H_, W_, p1, p2, gamma.data_ptr(), beta.data_ptr(), -10000.0, 1e-5,
               xp.data_ptr(), xn.data_ptr(), P, P, m.data_ptr(), r.data_ptr(), pm.data_ptr(), H.stream_ptr())
    out = {}
    for name, knob in knobs.items():
        H.lib().mca_debug_set(13, knob)
        out[name] = round(median_us(fn), 2)
    H.lib().mca_debug_set(13, 0)
    return out


AB_ND = {"product": 0, "span8": 8, "span4": 4, "span2": 2, "span1": 1, "product_again": 0}
ND_SHAPES = {"image": dict(C=3, shape=(224, 224), patch=(16, 16)), "video": dict(C=3, shape=(8, 112, 112), patch=(2, 8, 8))}


def nd_dims(mode):
    sh = ND_SHAPES[mode]
    T, H, W = (1, *sh["shape"])[-3:]
    pt, p1, p2 = (1, *sh["patch"])[-3:]
    return sh["C"], T, H, W, pt, p1, p2, (T // pt) * (H // p1) * (W // p2), sh["C"] * pt * p1 * p2


def nd_kernel(H, b, mode):
    """`mca_patch_nd_ln_fwd` over b samples of ND_SHAPES[mode], with xp, against its floor; inputs rotate over four buffer sets"""
    C, T, Hh, W, pt, p1, p2, n, P = nd_dims(mode)
    rows = b * n
    g = torch.Generator(device="cuda").manual_seed(0)
    gamma, beta = torch.randn(P, generator=g, device="cuda"), torch.randn(P, generator=g, device="cuda")
    sets = []
    for _ in range(4):
        v = torch.randn(b, C, T, Hh, W, generator=g, device="cuda")
        v[:, :, :, Hh // 2:] = -10000.0          # half of the rows padded: those patches take the all-pad path
        sets.append((v, torch.empty(rows, P, device="cuda"), torch.empty(rows, P, dtype=torch.bfloat16, device="cuda"),
                     torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda"), torch.empty(rows, dtype=torch.uint8, device="cuda")))
    k = [0]

    def fn():
        v, xp, xn, m, r, pm = sets[k[0] % 4]
        k[0] += 1
        H.call("mca_patch_nd_ln_fwd", v.data_ptr(), C * T * Hh * W, T * Hh * W, Hh * W, W, b, C, T, Hh, W, pt, p1, p2, gamma.data_ptr(),
               beta.data_ptr(), -10000.0, 1e-5, xp.data_ptr(), xn.data_ptr(), P, P, m.data_ptr(), r.data_ptr(), pm.data_ptr(), H.stream_ptr())
    ab = {}
    for name, knob in AB_ND.items():          # knob 13: at most c patches per workgroup (the kernel has no direct form)
        H.lib().mca_debug_set(13, knob)
        ab[name] = round(median_us(fn), 2)
    H.lib().mca_debug_set(13, 0)
    us = ab["product"]
    nbytes = rows * P * (4 + 4 + 2) + rows * 9
    floor = nbytes / (COPY_TB_S * 1e12) * 1e6
    return {"rows": rows, "P": P, "us": us, "bytes": nbytes, "GB_per_s": round(nbytes / us * 1e-3, 1), "floor_us_at_6.29TB_s": round(floor, 2),
            "fraction_of_floor": round(floor / us, 3), "ab_us": ab}


def matrix_kernel(H, b):
    """the matrix kernel's product form alone, for the same-run comparison of the N-D page"""
    rows, P = b * (H_ // P1) * (W_ // P2), P1 * P2
    us = kernel_us(H, b, P1, P2, {"product": 0})["product"]
    nbytes = rows * P * (4 + 4 + 2) + rows * 9
    floor = nbytes / (COPY_TB_S * 1e12) * 1e6
    return {"rows": rows, "P": P, "us": us, "bytes": nbytes, "GB_per_s": round(nbytes / us * 1e-3, 1), "floor_us_at_6.29TB_s": round(floor, 2),
            "fraction_of_floor": round(floor / us, 3)}


AB = {"product": 0, "staged": 64, "staged_span4": 4, "staged_span2": 2, "staged_span1": 1, "direct": -64, "direct_span4": -4, "product_again": 0}


def kernel(H, b):
    """the product form at 16 x 16 patches against the floor, and the A/B forms of knob 13 (+c: staged, at most c patches per
    workgroup; -c: the wavefront-per-patch form that reads global memory directly) at 16 x 16 and at 64 x 4 patches (16-byte patch rows)"""
    rows, P = b * (H_ // P1) * (W_ // P2), P1 * P2
    ab = kernel_us(H, b, P1, P2, AB)
    us = ab["product"]
    nbytes = rows * P * (4 + 4 + 2) + rows * 9
    floor = nbytes / (COPY_TB_S * 1e12) * 1e6
    return {"rows": rows, "P": P, "us": us, "bytes": nbytes, "GB_per_s": round(nbytes / us * 1e-3, 1), "floor_us_at_6.29TB_s": round(floor, 2),
            "fraction_of_floor": round(floor / us, 3), "ab_16x16_us": ab, "ab_64x4_us": kernel_us(H, b, 64, 4, AB)}


def step_config(P, b, typ, mode="matrix"):
    cfg = P.config.cmu_model_config(batch_size=b)
    if mode != "matrix":
        C, T, Hh, W, pt, p1, p2, n, _ = nd_dims(mode)
        cfg["encoder_configs"]["FACET"] = {"type": typ, "patch_size": list(ND_SHAPES[mode]["patch"]), "num_channels": C,
                                           "input_shape": list(ND_SHAPES[mode]["shape"]), "max_tokens": n, "embedding_dim": D, "dropout": 0.0}
        return cfg
    cfg["encoder_configs"]["FACET"] = {"type": typ, "patch_size": [P1, P2], "input_shape": [H_, W_], "max_tokens": 512, "embedding_dim": D,
                                       "dropout": 0.0}
    return cfg


def child(which, b, steps, mode="matrix"):
    """one window in a fresh process: -> one JSON line {which, ms}"""
    P = importlib.import_module("mca-paper_amd")
    optim = importlib.import_module("mca-paper_amd.optim")
    if mode == "matrix":
        from patch_twin import TWIN as twin, TwinPatchEncoder
        native, P.encoders_dict[twin] = "PatchEncoder", TwinPatchEncoder
    else:
        from patch_nd_twin import TWIN_CLASSES, TWINS
        native = {"image": "ImagePatchEncoder", "video": "VideoPatchEncoder"}[mode]
        twin = TWINS[native]
        P.encoders_dict.update(TWIN_CLASSES)
    batch = P.data.synthetic_batch(step_config(P, b, native, mode), b, seed=1234, lengths="uniform", p_drop=0.2, device="cuda")
    torch.manual_seed(0)
    model = P.MCA(**copy.deepcopy(step_config(P, b, native if which == "native" else twin, mode))).cuda()
    model.engine.check_finite = "deferred"
    opt = optim.FusedAdamW(model, lr=1e-4)

    def step():
        out = model(batch); opt.zero_grad(); out["loss"].backward()
        optim.clip_grad_norm_(model, 2.0); opt.step()
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    print(json.dumps({"which": which, "ms": round((time.perf_counter() - t0) * 1e3 / steps, 3)}), flush=True)


def smi():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        keep = [" ".join(ln.split()) for ln in r.stdout.splitlines() if "GPU[0]" in ln and any(k in ln.lower() for k in ("sclk", "mclk", "power"))]
        return keep or ["rocm-smi printed nothing for GPU 0"]
    except Exception as e:          # noqa: BLE001  (the figures stand without it; the line says it is missing)
        return [f"rocm-smi not available: {e}"]


def write_profile(path, rec):
    k, ms = rec["kernel"], rec["step_ms"]
    lines = [
        "# PatchEncoder: the front-end kernel and the step against the torch twin", "",
        f"Measured on one {rec['device']} with `python tools/bench_patch_encoder.py` ({rec['utc']}).  Clock and power read with `rocm-smi`",
        "before and after: " + "; ".join(rec["smi_before"]) + " | " + "; ".join(rec["smi_after"]) + ".", "",
        f"## (a) `mca_patch_ln_fwd` (b = {rec['batch']}, {H_} x {W_} matrices, {P1} x {P2} patches: {k['rows']} rows of P = {k['P']})", "",
        f"- {k['us']} us per launch (median over 30 rounds of 20 launches, device events, inputs rotating over four buffer sets)",
        f"- bytes moved: {k['bytes']:,} (values read once, xp fp32 and xn bf16 written, mean / rstd / padmask): {k['GB_per_s']} GB/s",
        f"- floor: those bytes at the {COPY_TB_S} TB/s a float4 copy reaches = {k['floor_us_at_6.29TB_s']} us; floor / measured = {k['fraction_of_floor']}", "",
        "A/B forms of knob 13 in the same process, in this order (us per launch; `staged`: strip rows through LDS, at most c patches per",
        "workgroup; `direct`: each wavefront reads its patch from global memory; `product` = `staged` with the default span):", "",
        "| patches | " + " | ".join(AB) + " |", "|---|" + "---|" * len(AB),
        f"| {P1} x {P2} | " + " | ".join(str(k["ab_16x16_us"][n]) for n in AB) + " |",
        "| 64 x 4 | " + " | ".join(str(k["ab_64x4_us"][n]) for n in AB) + " |", "",
        f"## (b) The step: native `PatchStep` against `TwinPatchEncoder` through `ForeignStep`", "",
        "CMU model (D = 512, 5 layers) with `FACET` replaced by a 512-token PatchEncoder, ragged row counts, 20 % of the modalities",
        f"dropped, b = {rec['batch']}, eager loop (forward, backward, clip, `FusedAdamW`), {rec['steps']} steps per window after 5 warm-up steps, one fresh",
        "process per window, alternating native, twin, native, twin, native, twin:", "",
        "| | window 1 | window 2 | window 3 |", "|---|---|---|---|",
        "| native (ms / step) | " + " | ".join(f"{x:.3f}" for x in ms["native"]) + " |",
        "| torch twin (ms / step) | " + " | ".join(f"{x:.3f}" for x in ms["twin"]) + " |", "",
        "The bench line:", "", "```", json.dumps(rec), "```", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def write_profile_nd(path, rec):
    ks, ms, mode = rec["kernels"], rec["step_ms"], rec["mode"]
    nat, twin = sum(ms["native"]) / len(ms["native"]), sum(ms["twin"]) / len(ms["twin"])
    spread = max(ms["twin"]) - min(ms["twin"])
    what = {"image": "3 x 224 x 224 images in 16 x 16 patches", "video": "3 x 8 x 112 x 112 clips in (2, 8, 8) tubelets",
            "matrix": f"{H_} x {W_} matrices in {P1} x {P2} patches (`mca_patch_ln_fwd`)"}
    lines = [
        "# ImagePatchEncoder / VideoPatchEncoder: the N-D front-end kernel and the step against the torch twin", "",
        f"Measured on one {rec['device']} with `python tools/bench_patch_encoder.py --mode {mode}` ({rec['utc']}).  Clock and power read with",
        "`rocm-smi` before and after: " + "; ".join(rec["smi_before"]) + " | " + "; ".join(rec["smi_after"]) + ".", "",
        f"## (a) `mca_patch_nd_ln_fwd` (b = {rec['batch']}, with xp)", "",
        "us per launch: median over 30 rounds of 20 launches, device events, inputs rotating over four buffer sets.  Bytes moved: values",
        f"read once, xp fp32 and xn bf16 written, mean / rstd / padmask.  Floor: those bytes at the {COPY_TB_S} TB/s a float4 copy reaches.", "",
        "| input | rows | P | us | bytes | GB/s | floor us | floor / measured |", "|---|---|---|---|---|---|---|---|"]
    for m in ("image", "video", "matrix"):
        k = ks[m]
        lines.append(f"| {what[m]} | {k['rows']} | {k['P']} | {k['us']} | {k['bytes']:,} | {k['GB_per_s']} | {k['floor_us_at_6.29TB_s']} | {k['fraction_of_floor']} |")
    lines += [
        "", "Spans of knob 13 in the same process, in this order (us per launch; at most c patches per workgroup; `product` = the default span,",
        "`4096 / P` patches rounded down to a power of two: 4 for these images, 8 for these clips):", "",
        "| input | " + " | ".join(AB_ND) + " |", "|---|" + "---|" * len(AB_ND)]
    for m in ("image", "video"):
        lines.append(f"| {what[m]} | " + " | ".join(str(ks[m]["ab_us"][n]) for n in AB_ND) + " |")
    lines += [
        "", f"## (b) The step: native `PatchNDStep` against the torch twin through `ForeignStep` ({mode} modality)", "",
        f"CMU model (D = 512, 5 layers) with `FACET` replaced by {what[mode]}, a random tail padded, 20 % of the modalities dropped,",
        f"b = {rec['batch']}, eager loop (forward, backward, clip, `FusedAdamW`), {rec['steps']} steps per window after 5 warm-up steps, one fresh process per",
        "window, alternating native, twin, native, twin, native, twin:", "",
        "| | window 1 | window 2 | window 3 | mean |", "|---|---|---|---|---|",
        "| native (ms / step) | " + " | ".join(f"{x:.3f}" for x in ms["native"]) + f" | {nat:.3f} |",
        "| torch twin (ms / step) | " + " | ".join(f"{x:.3f}" for x in ms["twin"]) + f" | {twin:.3f} |", "",
        f"Native - twin = {nat - twin:+.3f} ms; the spread (max - min) of the twin's own windows is {spread:.3f} ms.", "",
        "The bench line:", "", "```", json.dumps(rec), "```", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="matrix", choices=["matrix", "image", "video"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--profile", default=None)
    ap.add_argument("--child", default=None, choices=["native", "twin"])
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.batch, a.steps, a.mode)
    importlib.import_module("mca-paper_amd.build").build(verbose=False)
    # the windows first: this process starts its children before it opens the GPU itself
    smi_before = smi()
    ms = {"native": [], "twin": []}
    for _ in range(3):
        for which in ("native", "twin"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--mode", a.mode, "--batch", str(a.batch), "--steps", str(a.steps)],
                               stdout=subprocess.PIPE, text=True, timeout=600, check=True)
            ms[which].append(json.loads(r.stdout.strip().splitlines()[-1])["ms"])
    H = importlib.import_module("mca-paper_amd.hip")
    if a.mode != "matrix":
        rec = {"what": "bench_patch_encoder", "mode": a.mode, "device": torch.cuda.get_device_name(0), "batch": a.batch, "steps": a.steps,
               "smi_before": smi_before, "kernels": {"image": nd_kernel(H, a.batch, "image"), "video": nd_kernel(H, a.batch, "video"),
                                                     "matrix": matrix_kernel(H, a.batch)}, "step_ms": ms, "smi_after": smi()}
        rec["utc"] = time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime())
        if a.profile:
            write_profile_nd(a.profile, rec)
        print(json.dumps(rec), flush=True)
        return
    rec = {"what": "bench_patch_encoder", "device": torch.cuda.get_device_name(0), "batch": a.batch, "steps": a.steps, "smi_before": smi_before,
           "kernel": kernel(H, a.batch), "step_ms": ms, "smi_after": smi()}
    rec["utc"] = time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime())
    if a.profile:
        write_profile(a.profile, rec)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
