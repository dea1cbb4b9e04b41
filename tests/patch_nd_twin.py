"""TwinImagePatchEncoder / TwinVideoPatchEncoder: ImagePatchEncoder and VideoPatchEncoder restated in plain torch (reshape / permute,
no einops) with the reference's key names: the reference's PatchEncoder in modes "image" / "video" (encoders.py:252-267) with the
patch grid axes merged, which is the one way its rearrangements yield (b, l, D) tokens.  Registered under their own type names they
are foreign encoders: the engine runs them under autograd through ForeignStep, the way an image or video modality had to run before
the native classes.  Shared by tests/test_patch_nd_cpu.py (held against the reference's fixture), tests/test_patch_nd_step_gpu.py
(the yardstick of the native step) and tools/bench_patch_encoder.py."""
import copy

import torch
from torch import nn

TWINS = {"ImagePatchEncoder": "TwinImagePatchEncoder", "VideoPatchEncoder": "TwinVideoPatchEncoder"}
# util_small's `audio` slot: 3 x 8 x 15 images in (4, 5) patches, 6 tokens; 2 x 4 x 8 x 10 clips in (2, 4, 5) patches, 8 tokens
IMAGE_CFG = {"type": "ImagePatchEncoder", "patch_size": [4, 5], "num_channels": 3, "input_shape": [8, 15], "max_tokens": 6,
             "embedding_dim": 128, "dropout": 0.0}
VIDEO_CFG = {"type": "VideoPatchEncoder", "patch_size": [2, 4, 5], "num_channels": 2, "input_shape": [4, 8, 10], "max_tokens": 8,
             "embedding_dim": 128, "dropout": 0.0}
ND_CFG = {"image": IMAGE_CFG, "video": VIDEO_CFG}


def patches_nd(values, patch):
    """(b, C, T, H, W) -> (b, gt, gh, gw, C pt p1 p2): 'b c (t pt) (h p1) (w p2) -> b t h w (c pt p1 p2)'; (b, C, H, W) with a
    2-entry patch -> (b, gh, gw, C p1 p2): 'b c (h p1) (w p2) -> b h w (c p1 p2)'"""
    if len(patch) == 2:
        return patches_nd(values.unsqueeze(2), (1, *patch)).squeeze(1)
    pt, p1, p2 = patch
    b, C, T, H, W = values.shape
    x = values.reshape(b, C, T // pt, pt, H // p1, p1, W // p2, p2).permute(0, 2, 4, 6, 1, 3, 5, 7)
    return x.reshape(b, T // pt, H // p1, W // p2, C * pt * p1 * p2)


def unpatch_nd(rows, C, patch, grid, b):
    """the inverse, grid axes flattened: (b gt gh gw, P) -> (b, C, T, H, W)"""
    (pt, p1, p2), (gt, gh, gw) = patch, grid
    x = rows.reshape(b, gt, gh, gw, C, pt, p1, p2).permute(0, 4, 1, 5, 2, 6, 3, 7)
    return x.reshape(b, C, gt * pt, gh * p1, gw * p2).contiguous()


class _TwinPatchND(nn.Module):
    ndim = 0

    def __init__(self, patch_size=(16, 16), num_channels=0, embedding_dim=512, max_tokens=1024, dropout=0.1, attn_mask=True,
                 pad_token=-10000, **kwargs):
        super().__init__()
        assert len(patch_size) == self.ndim
        self.patch_size, self.pad_token = tuple(patch_size), -10000
        P = num_channels
        for p in patch_size:
            P *= p
        self.dropout = nn.Dropout(p=dropout)
        self.batch_to_tokens = nn.Sequential(nn.Identity(), nn.LayerNorm(P), nn.Linear(P, embedding_dim), nn.LayerNorm(embedding_dim))
        self.register_buffer("index", torch.arange(max_tokens))
        self.embedding = nn.Embedding(max_tokens, embedding_dim)

    def forward(self, batch):
        x = patches_nd(batch["values"].float(), self.patch_size).flatten(1, -2)
        x_t = self.batch_to_tokens(x)
        assert x_t.shape[1] == self.index.shape[0], f"{x_t.shape[1]} - {self.index.shape[0]}"
        x_p = self.embedding(self.index.unsqueeze(0).expand(x_t.shape[0], -1))
        mask = torch.all(x == self.pad_token, dim=-1).to(torch.long)
        return self.dropout(x_t + x_p), mask


class TwinImagePatchEncoder(_TwinPatchND):
    ndim = 2


class TwinVideoPatchEncoder(_TwinPatchND):
    ndim = 3


TWIN_CLASSES = {"TwinImagePatchEncoder": TwinImagePatchEncoder, "TwinVideoPatchEncoder": TwinVideoPatchEncoder}


def reference_tokens(rec):
    """the (b, l, D) tokens of a record of tests/golden/patch_encoder_nd_tiny.pt: the reference's `batch_to_tokens` output with the
    grid axes flattened + its position table (index = arange), and the upstream gradient d/d tokens of
    tokens[mask == 0].square().sum() that the record's `grads` were computed for"""
    tokens = rec["pre"].flatten(1, -2) + rec["init"]["embedding.weight"]
    return tokens, 2 * tokens * (rec["mask"] == 0)[..., None]


def nd_config(small_config, variant, mode):
    """small_config(variant) with `audio` as an ImagePatchEncoder (6 tokens) or a VideoPatchEncoder (8 tokens)"""
    cfg = small_config(variant)
    cfg["encoder_configs"]["audio"] = copy.deepcopy(ND_CFG[mode])
    return cfg


def twin_config(cfg):
    c = copy.deepcopy(cfg)
    for e in c["encoder_configs"].values():
        e["type"] = TWINS.get(e["type"], e["type"])
    return c
