"""Kernel time of the attention readout against the forward on the same operands, one GPU, one JSON line:

    python tools/bench_readout.py [BATCH]

CMU structure [1500, 450, 450, 50] + 88 fusion tokens (N = 2538), b = 32, 8 heads, one fusion layer's q | k | v (random bf16, q
at the magnitude the engine stores: scale * log2 e folded in).  readout_us: mca_attn_readout (mass only, no probs) on the layer's
operands and the log-sum-exp the forward wrote; fwd_us: mca_attn_fwd as the engine launches it (mask product, lazy softmax
reference) on the same operands in the same process.  The two launches alternate, each between its own pair of device events;
medians over 40 rounds after 12 warm-up rounds.  *_padded: the same with uniform valid lengths and 20 % of the modalities
dropped (tiles are skipped, blocks straddle the end of the valid keys)."""
import ctypes as C
import importlib
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools.bench_lp import _peak_sclk_mhz          # noqa: E402


def main():
    importlib.import_module("mca-paper_amd.build").build(verbose=False)
    P = importlib.import_module("mca-paper_amd")
    H = importlib.import_module("mca-paper_amd.hip")
    RO = importlib.import_module("mca-paper_amd.readout")
    b = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    cfg = P.config.cmu_model_config(batch_size=b)
    cfg["depth"] = 1
    torch.manual_seed(0)
    model = P.MCA(**cfg).cuda()
    eng = model.engine
    ws = eng.workspace(b)
    N, D, Hh = eng.N, eng.D, eng.H
    g = torch.Generator(device="cuda").manual_seed(7)
    a0 = ws["layers"][0]
    a0["qkv"].copy_(torch.randn(a0["qkv"].shape, device="cuda", generator=g).bfloat16())
    a0["qkv"][:, :D] *= 0.18
    ops = eng.layer_attention(ws, 0)[0]
    fa = importlib.import_module("mca-paper_amd.attention").fwd_args(ops, eng.attn_keys(ws), ws["vmean"])
    um = torch.from_numpy(RO.uniform_mass(eng.st)).cuda()
    mass = torch.empty(b, Hh, N, um.numel(), device="cuda")

    def fwd():
        H.call("mca_attn_fwd", C.byref(fa), H.stream_ptr())

    def readout():
        RO.launch(eng, ops, ws, mass, um)

    rec = {"what": "bench_readout", "device": torch.cuda.get_device_name(0), "sclk_mhz_max": _peak_sclk_mhz(0),
           "shape": f"b={b} heads={Hh} N={N} G={um.numel()}", "fwd_form": "mask product + lazy softmax reference" if ws.get("khot") is not None else "register-staged"}
    for tag in ("", "_padded"):
        ws["padding"].zero_()
        if tag:
            for mi, n in enumerate(eng.st.token_dims):
                ln = torch.randint(1, n + 1, (b,), device="cuda", generator=g)
                ln[torch.rand(b, device="cuda", generator=g) < 0.2] = 0
                ws["padding"][:, eng.offsets[mi]:eng.offsets[mi] + n] = (torch.arange(n, device="cuda")[None] >= ln[:, None]).to(ws["padding"].dtype)
        H.call("mca_build_keyinfo", ws["padding"].data_ptr(), eng.kgroup.data_ptr(), ws["keyinfo"].data_ptr(), ws["kflags"].data_ptr(), b, N,
               eng.nk_pad, H.stream_ptr())
        if ws.get("khot") is not None:
            H.call("mca_build_keyhot", ws["keyinfo"].data_ptr(), ws["khot"].data_ptr(), b, eng.nk_pad, H.stream_ptr())
        H.call("mca_attn_vmean", fa.v, fa.kv_bstride, fa.kv_ld, ws["vmean"].data_ptr(), b, N, Hh, H.stream_ptr())
        for _ in range(12):
            fwd(); readout()
        torch.cuda.synchronize()
        rounds = 40
        evs = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(rounds)] for k in ("fwd", "readout")}
        for i in range(rounds):
            for k, fn in (("fwd", fwd), ("readout", readout)):
                s, e = evs[k][i]
                s.record(); fn(); e.record()
        torch.cuda.synchronize()
        med = {}
        for k, lst in evs.items():
            t = sorted(s.elapsed_time(e) for s, e in lst)
            med[k] = t[len(t) // 2] * 1e3
        rec[f"fwd_us{tag}"], rec[f"readout_us{tag}"] = round(med["fwd"], 1), round(med["readout"], 1)
        rec[f"readout_over_fwd{tag}"] = round(med["readout"] / med["fwd"], 3)
        nonuni = ~torch.isinf(ops.lse)
        rec[f"max_row_sum_error{tag}"] = float((mass.sum(-1)[nonuni].double() - 1.0).abs().max())
    rec["utc"] = time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime())
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
