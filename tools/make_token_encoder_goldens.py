"""Fixture of the reference's two token-table encoders (encoders.py:100-120 SparseTabularEncoder, :145-166 SequenceEncoder).

    python tools/make_token_encoder_goldens.py <reference checkout>

Imports the reference's own ``encoders`` module from that checkout and writes tests/golden/token_encoders_tiny.pt: data only
(configs, seeds, weights, inputs, outputs, gradients).  Per encoder type, at V = 37, D = 128, n = 9, b = 3:
  config, seed      constructor keywords; state_dict ``init`` right after construction under torch.manual_seed(seed)
  table_in          the table the forward starts from: row r rescaled to L2 norm 3 (r even) or 0.5 (r odd), row 0 (padding) zero
  batch             repeated indices, index 0, index V - 1, one fully padded sample (sparse: data with zeros, one value > max_value)
  tokens, mask      the reference's output
  table_out         the table after the forward (nn.Embedding(max_norm = 1) rescales the looked-up rows in place)
  upstream, grads   a seeded gradient of the output tokens and the parameter gradients it gives
Consumed by tests/test_token_encoders_cpu.py and tests/test_token_encoders_gpu.py."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, D, N, B, SEED = 37, 128, 9, 3, 11


def record(cls, config, batch):
    torch.manual_seed(SEED)
    enc = cls(**config)
    rec = {"config": dict(config), "seed": SEED, "init": {k: v.clone() for k, v in enc.state_dict().items()}}
    w = enc.token_encoder.embedding.weight
    with torch.no_grad():
        norm = w.norm(dim=1, keepdim=True).clamp(min=1e-12)
        want = torch.where(torch.arange(V)[:, None] % 2 == 0, 3.0, 0.5)
        w.mul_(want / norm)
        w[0].zero_()
    rec["table_in"] = w.detach().clone()
    rec["batch"] = {k: v.clone() for k, v in batch.items()}
    tokens, mask = enc(batch)
    rec["tokens"], rec["mask"] = tokens.detach().clone(), mask.clone()
    rec["table_out"] = w.detach().clone()
    rec["upstream"] = torch.randn(tokens.shape, generator=torch.Generator().manual_seed(SEED + 1))
    tokens.backward(rec["upstream"])
    rec["grads"] = {k: p.grad.clone() for k, p in enc.named_parameters()}
    return rec


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.dont_write_bytecode = True
    sys.path.insert(0, sys.argv[1])
    import encoders as ref
    idx = torch.tensor([[5, 5, 5, V - 1, 1, 2, 0, 0, 0], [0] * N, [V - 1, 7, 7, 1, 3, 9, 10, 11, 12]], dtype=torch.int64)
    mask = (idx == 0).to(torch.long)
    data = (torch.rand(B, N, generator=torch.Generator().manual_seed(SEED + 2)) * 9.0 + 1.0).masked_fill(idx == 0, 0.0)
    data[0, 1], data[2, 4], data[2, 8] = 0.0, 250.0, 0.0          # a zero value at a real index, one above max_value
    out = {
        "SequenceEncoder": record(ref.SequenceEncoder, dict(type="SequenceEncoder", num_embeddings=V, embedding_dim=D, max_tokens=N),
                                  {"tokens": idx, "attention_mask": mask}),
        "SparseTabularEncoder": record(ref.SparseTabularEncoder,
                                       dict(type="SparseTabularEncoder", num_embeddings=V, embedding_dim=D, max_value=100, max_tokens=N),
                                       {"indices": idx, "data": data, "attention_mask": mask}),
    }
    path = os.path.join(REPO, "tests", "golden", "token_encoders_tiny.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
