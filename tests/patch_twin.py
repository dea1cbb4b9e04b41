"""TwinPatchEncoder: the reference's PatchEncoder (encoders.py:217-274, mode "matrix") restated in plain torch, without einops
(reshape / permute) and with the reference's key names.  Registered under the type name "TwinPatchEncoder" it is a foreign encoder:
the engine runs it under autograd through ForeignStep, the way a matrix modality had to run before the native PatchEncoder.  Shared
by tests/test_patch_encoder_cpu.py (held against the reference's fixture) and tests/test_patch_encoder_gpu.py (the yardstick of the
native step), and by tools/bench_patch_encoder.py."""
import copy

import torch
from torch import nn

TWIN = "TwinPatchEncoder"
PATCH_CFG = {"type": "PatchEncoder", "patch_size": [4, 5], "input_shape": [40, 35], "max_tokens": 70, "embedding_dim": 128, "dropout": 0.0}


def patches(values, p1, p2):
    """(b, H, W) -> (b, (H/p1)(W/p2), p1 p2): 'b (h p1) (w p2) -> b (h w) (p1 p2)'"""
    b, H, W = values.shape
    return values.reshape(b, H // p1, p1, W // p2, p2).permute(0, 1, 3, 2, 4).reshape(b, (H // p1) * (W // p2), p1 * p2)


class TwinPatchEncoder(nn.Module):
    def __init__(self, patch_size=(16, 16), mode="matrix", num_channels=0, embedding_dim=512, max_tokens=1024, dropout=0.1,
                 attn_mask=True, pad_token=-10000, **kwargs):
        super().__init__()
        assert mode == "matrix" and len(patch_size) == 2
        self.patch_size, self.pad_token = tuple(patch_size), -10000
        P = patch_size[0] * patch_size[1]
        self.dropout = nn.Dropout(p=dropout)
        self.batch_to_tokens = nn.Sequential(nn.Identity(), nn.LayerNorm(P), nn.Linear(P, embedding_dim), nn.LayerNorm(embedding_dim))
        self.register_buffer("index", torch.arange(max_tokens))
        self.embedding = nn.Embedding(max_tokens, embedding_dim)

    def forward(self, batch):
        x = patches(batch["values"].float(), *self.patch_size)
        x_t = self.batch_to_tokens(x)
        assert x_t.shape[1] == self.index.shape[0], f"{x_t.shape[1]} - {self.index.shape[0]}"
        x_p = self.embedding(self.index.unsqueeze(0).expand(x_t.shape[0], -1))
        mask = torch.all(x == self.pad_token, dim=-1).to(torch.long)
        return self.dropout(x_t + x_p), mask


def patch_config(small_config, variant):
    """small_config(variant) with `audio` (70 tokens) as a PatchEncoder over 40 x 35 matrices in (4, 5) patches"""
    cfg = small_config(variant)
    cfg["encoder_configs"]["audio"] = copy.deepcopy(PATCH_CFG)
    return cfg


def twin_config(cfg):
    c = copy.deepcopy(cfg)
    for e in c["encoder_configs"].values():
        if e["type"] == "PatchEncoder":
            e["type"] = TWIN
    return c
