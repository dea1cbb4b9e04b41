"""Token-table kernels and a step with a token modality, one GPU, one JSON line:

    python tools/bench_token_encoders.py [BATCH] [STEPS]

kernels: `mca_embedding_lookup` (store form with a positional table: mark + renormalise-marked + gather), `mca_embedding_scatter_add`
and `mca_embedding_scatter_add_det` at b = BATCH (32), n in {50, 512}, V = 36602, D = 512, indices uniform in [1, V) with uniform
valid lengths and pad token 0 behind them.  Each figure is the median over 30 rounds of (device-event time around 20 launches) / 20
after warm-up; beside it the bytes the algorithm moves over that time (lookup: a table row read and a token row written per token +
the positional table once; scatter: a gradient row read and a table row added per non-pad token).
step: the CMU model with `glove_vectors` replaced by a 50-token SequenceEncoder, eager loop (forward, backward, clip, FusedAdamW),
natively and with the encoder as a torch module (nn.Embedding(max_norm = 1) + positional table under autograd, the way such a
modality ran before the native step).  Three alternating windows of STEPS (20) steps each, host clock around a device synchronise,
5 warm-up steps per model."""
import copy
import importlib
import json
import os
import sys
import time

import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
V, D = 36602, 512


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


def kernels(H, b):
    out = {}
    g = torch.Generator().manual_seed(0)
    table = torch.randn(V, D, generator=g)
    table = (table / table.norm(dim=1, keepdim=True) * 0.9).cuda()          # within max_norm: every round does the same work
    dtable, marker = torch.zeros(V, D, device="cuda"), torch.zeros(V, dtype=torch.int32, device="cuda")
    st = H.stream_ptr
    for n in (50, 512):
        rows = b * n
        ln = torch.randint(1, n + 1, (b,), generator=g)
        idx = torch.randint(1, V, (b, n), generator=g).masked_fill(torch.arange(n)[None] >= ln[:, None], 0).cuda()
        valid = int((idx != 0).sum())
        pe, x, dy = torch.randn(n, D, device="cuda"), torch.empty(b, n, D, device="cuda"), torch.randn(b, n, D, device="cuda")
        scratch = torch.empty(max(H.lib().mca_embedding_scatter_add_det_scratch(rows), 1), device="cuda")
        sc_args = (dy.data_ptr(), D, n * D, n, idx.data_ptr(), 8, rows, dtable.data_ptr(), V, D, 0)
        forms = {
            "lookup": (lambda: H.call("mca_embedding_lookup", table.data_ptr(), V, D, 1.0, idx.data_ptr(), 8, rows, n, pe.data_ptr(),
                                      x.data_ptr(), D, n * D, 0, marker.data_ptr(), None, 0, st()), (2 * rows + n) * D * 4),
            "scatter_add": (lambda: H.call("mca_embedding_scatter_add", *sc_args, st()), 2 * valid * D * 4),
            "scatter_add_det": (lambda: H.call("mca_embedding_scatter_add_det", *sc_args, scratch.data_ptr(), scratch.numel(), st()),
                                2 * valid * D * 4),
        }
        for name, (fn, nbytes) in forms.items():
            us = median_us(fn)
            out[f"{name}_n{n}"] = {"us": round(us, 2), "bytes": nbytes, "GB_per_s": round(nbytes / us * 1e-3, 1)}
        out[f"tokens_n{n}"] = {"rows": rows, "non_pad": valid}
    return out


class TorchSequenceEncoder(nn.Module):
    def __init__(self, num_embeddings=V, embedding_dim=D, padding_idx=0, dropout=0.0, max_tokens=1024, **kwargs):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.token_encoder = nn.ModuleDict({"embedding": nn.Embedding(num_embeddings, embedding_dim, padding_idx=padding_idx, max_norm=1.0)})
        encs = importlib.import_module("mca-paper_amd.encoders")
        self.positional_encoder = encs.PositionalEncoder(embedding_dim, dropout, max_tokens)

    def forward(self, batch):
        x = self.token_encoder["embedding"](batch["tokens"])
        return x + self.positional_encoder.pe[: x.shape[1]], batch["attention_mask"]


def step_models(P, b):
    optim = importlib.import_module("mca-paper_amd.optim")
    P.encoders_dict["TorchSequenceEncoder"] = TorchSequenceEncoder
    cfg = P.config.cmu_model_config(batch_size=b)
    cfg["encoder_configs"]["glove_vectors"] = {"type": "SequenceEncoder", "num_embeddings": V, "embedding_dim": D, "max_tokens": 50}
    batch = P.data.synthetic_batch(cfg, b, seed=1234, lengths="uniform", p_drop=0.2, device="cuda")
    runs = {}
    for key, typ in (("native", "SequenceEncoder"), ("torch_twin", "TorchSequenceEncoder")):
        c = copy.deepcopy(cfg)
        c["encoder_configs"]["glove_vectors"]["type"] = typ
        torch.manual_seed(0)
        model = P.MCA(**c).cuda()
        model.engine.check_finite = "deferred"
        opt = optim.FusedAdamW(model, lr=1e-4)

        def step(model=model, opt=opt):
            out = model(batch); opt.zero_grad(); out["loss"].backward()
            optim.clip_grad_norm_(model, 2.0); opt.step()
        runs[key] = step
    return runs


def main():
    importlib.import_module("mca-paper_amd.build").build(verbose=False)
    P = importlib.import_module("mca-paper_amd")
    H = importlib.import_module("mca-paper_amd.hip")
    b = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rec = {"what": "bench_token_encoders", "device": torch.cuda.get_device_name(0), "batch": b, "V": V, "D": D, "kernels": kernels(H, b)}
    runs = step_models(P, b)
    for fn in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(3):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _s in range(steps):
                fn()
            torch.cuda.synchronize()
            ms[k].append(round((time.perf_counter() - t0) * 1e3 / steps, 3))
    rec["step_ms"] = ms
    rec["step"] = f"CMU, glove_vectors -> SequenceEncoder(V={V}, 50 tokens), b={b}, eager loop, {steps} steps per window"
    rec["utc"] = time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime())
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
