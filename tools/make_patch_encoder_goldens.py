"""Fixture of the reference's PatchEncoder (encoders.py:217-274), mode "matrix".

    python tools/make_patch_encoder_goldens.py <reference checkout>

Imports the reference's own ``encoders`` module from that checkout (it needs einops) and writes tests/golden/patch_encoder_tiny.pt:
data only.  Under "configs", for (4, 5) patches of a 40 x 35 matrix (70 tokens, D = 128) and (2, 3) patches of a 6 x 15 matrix
(15 tokens, D = 64), b = 3:
  config, seed      constructor keywords; state_dict ``init`` right after construction under torch.manual_seed(seed)
  weights           the state_dict the forward ran with: ``init`` with both LayerNorms' gamma and beta moved off 1 and 0
  batch             ``values``: sample 0 real with its last rows -10000 from the middle of a patch row on (partly padded patches,
                    then all-pad ones), sample 1 all -10000, sample 2 real with a single -10000 inside one patch
  tokens, mask      the reference's output
  upstream, grads   d/d tokens and every parameter gradient of tokens[mask == 0].square().sum()
Under "unrunnable", for modes "image" and "video": the exception class and text the reference raises when it is constructed and
called (its forward can only run mode "matrix").
Consumed by tests/test_patch_encoder_cpu.py and tests/test_patch_encoder_gpu.py."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 3
CASES = (dict(seed=21, patch_size=[4, 5], shape=(40, 35), max_tokens=70, embedding_dim=128, cut=22, lone=(9, 17)),
         dict(seed=22, patch_size=[2, 3], shape=(6, 15), max_tokens=15, embedding_dim=64, cut=3, lone=(4, 7)))


def record(ref, case):
    H, W = case["shape"]
    config = dict(type="PatchEncoder", patch_size=list(case["patch_size"]), input_shape=[H, W], max_tokens=case["max_tokens"],
                  embedding_dim=case["embedding_dim"], dropout=0.0)
    torch.manual_seed(case["seed"])
    enc = ref.PatchEncoder(**config)
    rec = {"config": config, "seed": case["seed"], "init": {k: v.clone() for k, v in enc.state_dict().items()}}
    g = torch.Generator().manual_seed(case["seed"] + 100)
    with torch.no_grad():
        for i in (1, 3):
            ln = enc.batch_to_tokens[i]
            ln.weight.add_(0.1 * torch.randn(ln.weight.shape, generator=g))
            ln.bias.add_(0.1 * torch.randn(ln.bias.shape, generator=g))
    rec["weights"] = {k: v.clone() for k, v in enc.state_dict().items()}
    vals = torch.randn(B, H, W, generator=g)
    vals[0, case["cut"]:] = -10000.0
    vals[1] = -10000.0
    vals[2][case["lone"]] = -10000.0
    rec["batch"] = {"values": vals.clone()}
    tokens, mask = enc({"values": vals})
    rec["tokens"], rec["mask"] = tokens.detach().clone(), mask.clone()
    tokens.retain_grad()
    tokens[mask == 0].square().sum().backward()
    rec["upstream"] = tokens.grad.clone()
    rec["grads"] = {k: p.grad.clone() for k, p in enc.named_parameters()}
    return rec


def unrunnable(ref, mode):
    """the reference constructed and called in a mode other than "matrix": -> {stage, class, text} of what it raises.  max_tokens is
    the second dimension of its 4-D / 5-D token tensor, so that the call gets past the token-count assertion to what stops it"""
    patch, shape = ((2, 2), (2, 3, 4, 4)) if mode == "image" else ((2, 2, 2), (2, 3, 4, 4, 4))
    stage = "construct"
    try:
        enc = ref.PatchEncoder(patch_size=patch, mode=mode, num_channels=3, embedding_dim=8, max_tokens=2, dropout=0.0)
        stage = "call"
        enc({"values": torch.randn(*shape, generator=torch.Generator().manual_seed(5))})
    except Exception as e:          # noqa: BLE001  (whatever it raises is the record)
        return {"stage": stage, "class": type(e).__name__, "text": str(e)}
    return {"stage": "none", "class": "", "text": ""}


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.dont_write_bytecode = True
    sys.path.insert(0, sys.argv[1])
    import encoders as ref
    out = {"configs": [record(ref, c) for c in CASES], "unrunnable": {m: unrunnable(ref, m) for m in ("image", "video")}}
    for m, r in out["unrunnable"].items():
        print(m, r)
    path = os.path.join(REPO, "tests", "golden", "patch_encoder_tiny.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
