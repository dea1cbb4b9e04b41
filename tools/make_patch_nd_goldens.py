"""Fixture of the reference's PatchEncoder (encoders.py:217-274) in modes "image" and "video", for ImagePatchEncoder / VideoPatchEncoder.

    python tools/make_patch_nd_goldens.py <reference checkout>

Imports the reference's own ``encoders`` module from that checkout (it needs einops) and writes tests/golden/patch_encoder_nd_tiny.pt:
data only.  The reference's forward cannot run these modes (tests/golden/patch_encoder_tiny.pt, "unrunnable"), but its constructor
and its ``batch_to_tokens`` can: what is recorded is what those give, with the patch grid axes flattened where a (b, l, D) token
tensor is needed.  Under "image" (C = 3, (2, 3) patches, grid 3 x 5) and "video" (C = 3, (2, 2, 3) patches, grid 2 x 2 x 3), D = 128,
b = 3:
  config, seed      constructor keywords of the native class (the reference's, without ``mode``, plus ``input_shape``); state_dict
                    ``init`` right after the reference's construction under torch.manual_seed(seed)
  ln                the four LayerNorm tensors moved off 1 and 0: the forward ran with dict(init, **ln)
  batch             ``values``: sample 0 real, with one patch in which a single channel is all -10000 and the others real, partly padded
                    patches (an image's rows / a clip's last frame -10000 from inside a patch on) and all-pad patches; sample 1 all
                    -10000; sample 2 real with a single -10000
  rearranged        the output of the reference's ``batch_to_tokens[0]``: (b, h, w, P) / (b, t, h, w, P)
  pre               the output of the reference's ``batch_to_tokens``, before the position table: (b, h, w, D) / (b, t, h, w, D)
  mask              all(rearranged == -10000) over P, grid axes flattened: (b, l) int64
  grads             with tokens = pre (grid axes flattened) + embedding(index): every parameter gradient of
                    tokens[mask == 0].square().sum(); its upstream gradient d/d tokens is 2 tokens on the rows with mask 0 and zero
                    elsewhere, which the tests recompute (upstream() in tests/patch_nd_twin.py) instead of reading it from here
Consumed by tests/test_patch_nd_cpu.py and tests/test_patch_nd_step_gpu.py."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, D, C = 3, 128, 3
PAD = -10000.0


def image_batch(g):
    v = torch.randn(B, C, 6, 15, generator=g)
    v[0, 1, 0:2, 3:6] = PAD          # patch (0, 1): channel 1 all pad, channels 0 and 2 real
    v[0, :, 3:] = PAD                # rows 3 .. 5: grid row 1 partly padded, grid row 2 all pad
    v[1] = PAD
    v[2, 2, 4, 7] = PAD              # a lone pad value
    return v


def video_batch(g):
    v = torch.randn(B, C, 4, 4, 9, generator=g)
    v[0, 2, 0:2, 0:2, 3:6] = PAD     # patch (0, 0, 1): channel 2 all pad, channels 0 and 1 real
    v[0, :, 3] = PAD                 # the last frame: temporal patch 1 partly padded
    v[0, :, 2:, 2:] = PAD            # and its grid row 1 all pad
    v[1] = PAD
    v[2, 1, 1, 2, 7] = PAD           # a lone pad value
    return v


CASES = {"image": dict(seed=31, patch_size=[2, 3], input_shape=[6, 15], max_tokens=15, batch=image_batch, cls="ImagePatchEncoder"),
         "video": dict(seed=32, patch_size=[2, 2, 3], input_shape=[4, 4, 9], max_tokens=12, batch=video_batch, cls="VideoPatchEncoder")}


def record(ref, mode, case):
    kw = dict(patch_size=list(case["patch_size"]), num_channels=C, max_tokens=case["max_tokens"], embedding_dim=D, dropout=0.0)
    torch.manual_seed(case["seed"])
    enc = ref.PatchEncoder(mode=mode, **kw)
    rec = {"config": dict(kw, type=case["cls"], input_shape=list(case["input_shape"])), "seed": case["seed"],
           "init": {k: v.clone() for k, v in enc.state_dict().items()}}
    g = torch.Generator().manual_seed(case["seed"] + 100)
    with torch.no_grad():
        for i in (1, 3):
            ln = enc.batch_to_tokens[i]
            ln.weight.add_(0.1 * torch.randn(ln.weight.shape, generator=g))
            ln.bias.add_(0.1 * torch.randn(ln.bias.shape, generator=g))
    rec["ln"] = {k: v.clone() for k, v in enc.state_dict().items() if k.startswith(("batch_to_tokens.1.", "batch_to_tokens.3."))}
    vals = case["batch"](g)
    rec["batch"] = {"values": vals.clone()}
    rearranged = enc.batch_to_tokens[0](vals)
    pre = enc.batch_to_tokens(vals)
    rec["rearranged"], rec["pre"] = rearranged.clone(), pre.detach().clone()
    tokens = pre.flatten(1, -2) + enc.embedding(enc.index.unsqueeze(0).expand(B, -1))
    mask = torch.all(rearranged == enc.pad_token, dim=-1).flatten(1).to(torch.long)
    assert tokens.shape == (B, case["max_tokens"], D) and mask.shape == tokens.shape[:2]
    rec["mask"] = mask.clone()
    tokens[mask == 0].square().sum().backward()
    rec["grads"] = {k: p.grad.clone() for k, p in enc.named_parameters()}
    return rec


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.dont_write_bytecode = True
    sys.path.insert(0, sys.argv[1])
    import encoders as ref
    out = {mode: record(ref, mode, case) for mode, case in CASES.items()}
    path = os.path.join(REPO, "tests", "golden", "patch_encoder_nd_tiny.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
