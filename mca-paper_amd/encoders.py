"""Modality encoders and collators: the reference's plugin surface (encoders.py:277-283 ``encoders_dict``,
:367-371 ``collators``, :374-403 ``MultimodalCollator``).

The encoder classes here are PARAMETER CONTAINERS with the reference's module tree (so state_dict keys and
``torch.manual_seed`` initialisation are identical); their arithmetic runs in the HIP kernels driven by
``engine.FusionEngine``.  A modality whose ``type`` is registered by the user with an ordinary
``nn.Module`` (any class not derived from ``NativeEncoder``) still works: the engine runs it with torch
and feeds its tokens to the native trunk.

Encoder contract (encoders.py:196-214, :90-96): ``forward(batch_for_modality) -> (tokens (b,n,D),
attention_mask (b,n))`` with non-zero / True = padded position.
"""
from __future__ import annotations

import math
from collections import defaultdict
from typing import Dict, List, Optional

import torch
from torch import nn
from torch.nn.functional import pad


class NativeEncoder(nn.Module):
    """Marker base class: the engine has a fused HIP path for this encoder type."""
    kind = ""

    def forward(self, batch):
        raise NotImplementedError("a native encoder is a parameter container: its arithmetic is fused into the model's step "
                                  "(construct an MCA / EAO model and call it)")


class PositionalEncoder(nn.Module):
    """Sinusoidal table, buffer ``pe`` (max_len, d_model) (encoders.py:123-142).  Dropout p is 0.0 as the
    sequence encoders construct it, so the table is added as is."""

    def __init__(self, d_model: int, dropout: float = 0.1, max_len: int = 2048, **kwargs):
        super().__init__()
        self.p = dropout
        pos = torch.arange(max_len, dtype=torch.float32).unsqueeze(1)
        freq = torch.exp(torch.arange(0, d_model, 2) * (-math.log(10000.0) / d_model))
        table = torch.zeros(max_len, d_model)
        table[:, 0::2] = torch.sin(pos * freq)
        table[:, 1::2] = torch.cos(pos * freq)
        self.register_buffer("pe", table)


class EmbeddedSequenceEncoder(NativeEncoder):
    """Pre-embedded sequence: LN(in) -> Linear(in, D) -> LN(D), pad rows zeroed, + positional table
    (encoders.py:169-214)."""
    kind = "embedded_sequence"

    def __init__(self, input_size=128, embedding_dim=512, padding_idx=0, dropout=0.0, max_tokens=1024, **kwargs):
        super().__init__()
        self.input_size = input_size
        self.embedding_dim = embedding_dim
        self.max_tokens = max_tokens
        self.token_encoder = nn.Sequential(nn.LayerNorm(input_size), nn.Linear(input_size, embedding_dim),
                                           nn.LayerNorm(embedding_dim))
        self.positional_encoder = PositionalEncoder(embedding_dim, dropout, max_tokens)


class _TokenTable(nn.Module):
    """``nn.Embedding(n, D, padding_idx, max_norm=1.0)`` as a parameter holder (encoders.py:17-37).  The
    max_norm renormalisation (rows with L2 norm > 1 rescaled in place on every forward) is done by the
    engine before the table is used: of the whole table for TabularEncoder (every row is looked up), of the rows a
    batch names for the indexed encoders."""

    def __init__(self, num_embeddings, embedding_dim, padding_idx=None, max_norm=1.0):
        super().__init__()
        self.max_norm = max_norm
        self.num_embeddings = num_embeddings
        self.embedding = nn.Embedding(num_embeddings, embedding_dim, padding_idx=padding_idx)


class _ValueMLP(nn.Module):
    """Linear(1,D) -> ReLU -> Linear(D,D) -> LN(D), zero where x == padding_value (encoders.py:40-72)."""

    def __init__(self, d_model, dropout=0.1, max_value=512, padding_value=0.0):
        super().__init__()
        self.linear1 = nn.Linear(1, d_model)
        self.linear2 = nn.Linear(d_model, d_model)
        self.norm = nn.LayerNorm(d_model)
        self.max_value = max_value
        self.padding_value = padding_value


class TabularEncoder(NativeEncoder):
    """Dense table: learned per-column embedding + value MLP (encoders.py:75-96)."""
    kind = "tabular"

    def __init__(self, num_embeddings=128, embedding_dim=512, padding_idx=-1, dropout=0.0, max_value=10000, **kwargs):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.num_embeddings = num_embeddings
        self.register_buffer("index", torch.arange(num_embeddings))
        self.token_encoder = _TokenTable(num_embeddings, embedding_dim, padding_idx)
        self.value_encoder = _ValueMLP(embedding_dim, dropout, max_value, padding_idx)


class SequenceEncoder(NativeEncoder):
    """Token ids: table row of ``batch["tokens"]`` (b, n) + positional table; padded positions are NOT zeroed, the mask is handed
    through (encoders.py:145-166)."""
    kind = "token_sequence"

    def __init__(self, num_embeddings=36602, embedding_dim=512, padding_idx=0, dropout=0.0, max_tokens=1024, **kwargs):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.num_embeddings = num_embeddings
        self.max_tokens = max_tokens
        self.token_encoder = _TokenTable(num_embeddings, embedding_dim, padding_idx)
        self.positional_encoder = PositionalEncoder(embedding_dim, dropout, max_tokens)


class SparseTabularEncoder(NativeEncoder):
    """Index / value lists: table row of ``batch["indices"]`` (b, n) + value MLP of ``batch["data"]`` (b, n), the value part zero
    where data == padding_idx; no ``index`` buffer (encoders.py:100-120)."""
    kind = "sparse_tabular"

    def __init__(self, num_embeddings=36602, embedding_dim=512, padding_idx=0, dropout=0.0, max_value=10000, **kwargs):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.num_embeddings = num_embeddings
        self.token_encoder = _TokenTable(num_embeddings, embedding_dim, padding_idx)
        self.value_encoder = _ValueMLP(embedding_dim, dropout, max_value, padding_idx)


class _PatchRearrange(nn.Module):
    """Parameter-less stand-in for the reference's ``Rearrange('b (h p1) (w p2) -> b (h w) (p1 p2)')`` at index 0 of
    ``batch_to_tokens``: it keeps the state_dict keys of the layers after it (``batch_to_tokens.1`` ...) where the reference has
    them.  The rearrangement itself is the gather of ``mca_patch_ln_fwd`` (``mca_patch_nd_ln_fwd`` for images and video)."""

    def __init__(self, p1, p2):
        super().__init__()
        self.p1, self.p2 = p1, p2


class PatchEncoder(NativeEncoder):
    """2-D matrix (a spectrogram) cut into (p1, p2) patches: ``batch["values"]`` (b, H, W) -> token t = i * (W / p2) + j is patch
    (i, j), its P = p1 * p2 elements in (row, column) order; LN(P) -> Linear(P, D) -> LN(D) + a learned (max_tokens, D) position
    table looked up by ``arange``.  ``attention_mask[s, t]`` = every element of the patch equals ``pad_token`` (-10000 whatever
    the argument says, as the reference overwrites it); padded tokens are NOT zeroed (encoders.py:217-274).

    Refused at construction (docs/scope_and_gaps.md): mode "image" / "video" (the reference's own forward cannot run them),
    ``attn_mask=False`` (MCA.forward compares the returned None with 0), ``dropout != 0`` (the native step has no dropout) and
    patches of more than 1024 elements (the kernel's limit).  Optional ``input_shape: [H, W]``, which the reference swallows in
    ``**kwargs``, is checked against ``patch_size`` and ``max_tokens``.  Images and video clips: ImagePatchEncoder,
    VideoPatchEncoder."""
    kind = "patch"

    def __init__(self, patch_size=(16, 16), mode="matrix", num_channels=0, embedding_dim=512, max_tokens=1024, dropout: float = 0.1,
                 attn_mask=True, pad_token=-10000, input_shape=None, **kwargs):
        super().__init__()
        assert mode in ["matrix", "image", "video"]                                                                  # encoders.py:242
        if mode != "matrix":
            raise NotImplementedError(f"PatchEncoder: mode '{mode}' is not supported: the reference's forward can only run mode "
                                      "'matrix' (its mask layer exists for that mode alone and its other rearrangements do not "
                                      "yield (b, l, D) tokens)")
        assert len(patch_size) == 2                                                                                  # encoders.py:244
        if not attn_mask:
            raise NotImplementedError("PatchEncoder: attn_mask=False is not supported: the encoder would return None as its mask, "
                                      "which MCA.forward compares with 0")
        if dropout != 0.0:
            raise NotImplementedError(f"PatchEncoder: dropout={dropout} is not supported: the native step has no dropout; pass "
                                      "'dropout: 0.0' in the encoder's config")
        p1, p2 = int(patch_size[0]), int(patch_size[1])
        if p1 < 1 or p2 < 1 or p1 * p2 > 1024:
            raise NotImplementedError(f"PatchEncoder: patch_size {tuple(patch_size)} has {p1 * p2} elements; the native kernel takes "
                                      "1 to 1024 (32 x 32)")
        if input_shape is not None:
            H, W = int(input_shape[0]), int(input_shape[1])
            if H % p1 or W % p2 or (H // p1) * (W // p2) != max_tokens:
                raise ValueError(f"PatchEncoder: input_shape {(H, W)} in patches of {(p1, p2)} does not give max_tokens = {max_tokens} "
                                 "whole patches")
        self.attn_mask = attn_mask
        self.pad_token = -10000                                                                                      # encoders.py:239
        self.patch_size = patch_size
        self.embedding_dim = embedding_dim
        self.max_tokens = max_tokens
        self.input_shape = None if input_shape is None else (int(input_shape[0]), int(input_shape[1]))
        self.batch_to_tokens = nn.Sequential(_PatchRearrange(p1, p2), nn.LayerNorm(p1 * p2), nn.Linear(p1 * p2, embedding_dim),
                                             nn.LayerNorm(embedding_dim))
        self.register_buffer("index", torch.arange(max_tokens))
        self.embedding = nn.Embedding(max_tokens, embedding_dim)


class _PatchNDEncoder(NativeEncoder):
    """What ImagePatchEncoder and VideoPatchEncoder share: the reference's PatchEncoder constructor in mode "image" / "video"
    (encoders.py:226-267: same keywords, module tree, state_dict keys and RNG order) with the one repair that yields (b, l, D)
    tokens: the patch grid axes are merged.  ``patch`` is (pt, p1, p2) and ``input_shape`` (T, H, W), an image having pt = T = 1."""
    ndim = 0

    def __init__(self, patch_size, num_channels=0, embedding_dim=512, max_tokens=1024, dropout: float = 0.1, attn_mask=True,
                 pad_token=-10000, input_shape=None, **kwargs):
        super().__init__()
        name = type(self).__name__
        assert len(patch_size) == self.ndim                                                                      # encoders.py:243-246
        C = int(num_channels)
        if C < 1:
            raise ValueError(f"{name}: num_channels = {num_channels}: pass the number of channels of the input (the reference's "
                             "default 0 gives a Linear of zero width)")
        if not attn_mask:
            raise NotImplementedError(f"{name}: attn_mask=False is not supported: the encoder would return None as its mask, "
                                      "which MCA.forward compares with 0")
        if dropout != 0.0:
            raise NotImplementedError(f"{name}: dropout={dropout} is not supported: the native step has no dropout; pass "
                                      "'dropout: 0.0' in the encoder's config")
        patch = (1,) * (3 - self.ndim) + tuple(int(p) for p in patch_size)
        P = C * patch[0] * patch[1] * patch[2]
        if min(patch) < 1 or P > 1024:
            raise NotImplementedError(f"{name}: patch_size {tuple(patch_size)} over {C} channels has {P} elements; the native "
                                      "kernel takes 1 to 1024")
        if input_shape is not None:
            if len(input_shape) != self.ndim:
                raise ValueError(f"{name}: input_shape {tuple(input_shape)} does not have {self.ndim} entries")
            shape = (1,) * (3 - self.ndim) + tuple(int(x) for x in input_shape)
            grid = [x // p for x, p in zip(shape, patch)]
            if any(x % p for x, p in zip(shape, patch)) or grid[0] * grid[1] * grid[2] != max_tokens:
                raise ValueError(f"{name}: input_shape {tuple(input_shape)} in patches of {tuple(patch_size)} does not give "
                                 f"max_tokens = {max_tokens} whole patches")
            self.input_shape = tuple(int(x) for x in input_shape)
        else:
            self.input_shape = None
        self.attn_mask = attn_mask
        self.pad_token = -10000                                                                                  # encoders.py:239
        self.patch_size = patch_size
        self.patch = patch
        self.num_channels = C
        self.embedding_dim = embedding_dim
        self.max_tokens = max_tokens
        self.batch_to_tokens = nn.Sequential(_PatchRearrange(*patch[1:]), nn.LayerNorm(P), nn.Linear(P, embedding_dim),
                                             nn.LayerNorm(embedding_dim))
        self.register_buffer("index", torch.arange(max_tokens))
        self.embedding = nn.Embedding(max_tokens, embedding_dim)


class ImagePatchEncoder(_PatchNDEncoder):
    """Image (b, C, H, W) cut into (p1, p2) patches, 'b c (h p1) (w p2) -> b (h w) (c p1 p2)': token t = hi * (W / p2) + wi, its
    P = C * p1 * p2 elements in (channel, row, column) order; then as PatchEncoder: LN(P) -> Linear(P, D) -> LN(D) + the learned
    position table.  ``attention_mask[s, t]`` = every element of every channel of the patch equals ``pad_token`` (-10000).
    Refused at construction (docs/scope_and_gaps.md): ``num_channels < 1``, ``attn_mask=False``, ``dropout != 0``, more than
    1024 elements per patch, an ``input_shape: [H, W]`` that does not give ``max_tokens`` whole patches."""
    kind = "image_patch"
    ndim = 2

    def __init__(self, patch_size=(16, 16), num_channels=0, embedding_dim=512, max_tokens=1024, dropout: float = 0.1, attn_mask=True,
                 pad_token=-10000, input_shape=None, **kwargs):
        super().__init__(patch_size, num_channels, embedding_dim, max_tokens, dropout, attn_mask, pad_token, input_shape, **kwargs)


class VideoPatchEncoder(_PatchNDEncoder):
    """Video clip (b, C, T, H, W) cut into (pt, p1, p2) tubelets, 'b c (t p1) (h p2) (w p3) -> b (t h w) (c p1 p2 p3)': token
    (ti * (H / p1) + hi) * (W / p2) + wi, its P = C * pt * p1 * p2 elements in (channel, frame, row, column) order; otherwise as
    ImagePatchEncoder, with ``input_shape: [T, H, W]``."""
    kind = "video_patch"
    ndim = 3

    def __init__(self, patch_size=(2, 16, 16), num_channels=0, embedding_dim=512, max_tokens=1024, dropout: float = 0.1,
                 attn_mask=True, pad_token=-10000, input_shape=None, **kwargs):
        super().__init__(patch_size, num_channels, embedding_dim, max_tokens, dropout, attn_mask, pad_token, input_shape, **kwargs)


encoders_dict: Dict[str, type] = {
    "EmbeddedSequenceEncoder": EmbeddedSequenceEncoder,
    "TabularEncoder": TabularEncoder,
    "SequenceEncoder": SequenceEncoder,
    "SparseTabularEncoder": SparseTabularEncoder,
    "PatchEncoder": PatchEncoder,
    "ImagePatchEncoder": ImagePatchEncoder,
    "VideoPatchEncoder": VideoPatchEncoder,
}


# ------------------------------------------------------------------------------------------------------
# collators (host side; run in DataLoader workers)
# ------------------------------------------------------------------------------------------------------
def _batch_buffer(shape, fill, dtype):
    """The output buffer of a collator, filled with ``fill``.  Inside a DataLoader worker it is allocated in shared memory, as
    torch's default_collate does: a batch built in ordinary memory is copied into shared memory again when the worker hands it
    to the loop (58 MB per CMU batch of 32: 46 ms per batch with 8 workers against 12 ms, the difference between a loader-bound
    and a GPU-bound training loop, profiles/r04_slow_regime.md).  Same values either way."""
    if torch.utils.data.get_worker_info() is None:
        return torch.full(shape, fill, dtype=dtype)
    proto = torch.empty(0, dtype=dtype)
    numel = 1
    for d in shape:
        numel *= int(d)
    storage = proto._typed_storage()._new_shared(numel, device="cpu")
    return proto.new(storage).resize_(*shape).fill_(fill)


class SequenceCollator:
    """1-D sequences / dense tables padded (or cropped) to ``pad_len`` with ``pad_token``; ``attention_mask`` is int64 with
    1 where the padded value equals pad_token (encoders.py:286-311).  A missing sample (None) becomes an all-pad row.
    ``other_col`` is accepted and ignored, as in the reference (its ``__call__`` rebuilds the input dict with the data
    column only, so the second column never reaches the output).  One output buffer is filled in place."""

    def __init__(self, pad_token=0, pad_len=2048, data_col_name="indices", other_col="data", attn_mask=True, **kwargs):
        self.pad_token, self.pad_len, self.attn_mask = pad_token, pad_len, attn_mask
        self.data_col_name, self.other_col = data_col_name, other_col

    def _fill(self, rows, fill):
        # dtype of the stacked batch: promotion over the rows, a missing row counting as the float32 empty tensor the
        # reference substitutes (an int index column with a missing sample therefore comes out float32)
        dtype = None
        for x in rows:
            d = x.dtype if x is not None else torch.float32
            dtype = d if dtype is None else torch.promote_types(dtype, d)
        out = _batch_buffer((len(rows), self.pad_len), fill, dtype or torch.float32)
        for i, x in enumerate(rows):
            if x is not None and x.numel():
                n = min(x.shape[-1], self.pad_len)          # longer rows are cropped (the reference's negative F.pad does that)
                out[i, :n] = x[..., :n]
        return out

    def __call__(self, data):
        out = {self.data_col_name: self._fill(data[self.data_col_name], self.pad_token)}
        if self.attn_mask:
            out["attention_mask"] = (out[self.data_col_name] == self.pad_token).to(torch.long)
        return out


class EmbeddedSequenceCollator:
    """(len, emb) float sequences truncated / padded with ``fill_value`` to ``pad_len``; bool ``attention_mask`` True = pad
    (encoders.py:314-343).  None -> fully padded row.  NaN / inf are cleaned (``nan_to_num``) when ``clean``."""

    def __init__(self, pad_token=-1, fill_value=0.0, pad_len=2048, embedding_size=512, data_col_name="values",
                 attn_mask=True, truncate=True, clean=True, **kwargs):
        self.fill_value, self.pad_len, self.embedding_size = fill_value, pad_len, embedding_size
        self.data_col_name, self.attn_mask, self.truncate, self.clean = data_col_name, attn_mask, truncate, clean

    def __call__(self, data):
        seqs = data[self.data_col_name]
        first = next((x for x in seqs if x is not None), None)
        width = first.shape[-1] if first is not None else self.embedding_size
        dtype = first.dtype if first is not None else torch.float32
        tokens = _batch_buffer((len(seqs), self.pad_len, width), self.fill_value, dtype)
        mask = _batch_buffer((len(seqs), self.pad_len), True, torch.bool)
        for i, x in enumerate(seqs):
            if x is None:
                continue
            n = min(x.shape[0], self.pad_len)          # truncate=False crops as well: the reference's negative F.pad
            tokens[i, :n] = x[:n]
            mask[i, :n] = False
        if self.clean:
            tokens = tokens.nan_to_num_()
        out = {}
        if self.attn_mask:
            out["attention_mask"] = mask
        out["tokens"] = tokens
        return out


class MatrixCollator:
    """(rows, channels) float matrices padded along rows to ``pad_len`` with ``pad_token`` and cut to the first
    ``max_channels`` columns when that is non-zero; a missing sample is a (max_channels, pad_len) block of pad_token,
    as the reference builds it (encoders.py:346-364: note the transposed shape of the placeholder, kept)."""

    def __init__(self, pad_token=-10000, pad_len=2048, attn_mask=True, max_channels=0, **kwargs):
        self.pad_token, self.pad_len, self.max_channels = pad_token, pad_len, max_channels

    def __call__(self, data):
        mats = [torch.full((self.max_channels, self.pad_len), self.pad_token, dtype=torch.float) if x is None else x
                for x in data["values"]]
        outs = []
        for x in mats:
            n = min(x.shape[0], self.pad_len)
            o = torch.full((self.pad_len, x.shape[1]), self.pad_token, dtype=x.dtype)
            o[:n] = x[:n]
            outs.append(o[:, : self.max_channels] if self.max_channels else o)
        return {"values": torch.stack(outs)}


class PatchNDCollator:
    """Images (C, H, W) (type "image", ``input_shape: [H, W]``) or video clips (C, T, H, W) (type "video", ``input_shape:
    [T, H, W]``) of ``num_channels`` channels stacked into ``values`` (b, C, H, W) / (b, C, T, H, W) float32; no
    ``attention_mask``: the encoder derives it from the patches.  A missing sample (None) is a block of ``pad_token``.  A clip
    with fewer than T frames is padded at the end with ``pad_token`` (its wholly missing temporal patches come out masked), a
    longer one is cropped; any other shape mismatch is an error.  One output buffer is filled in place."""
    ndim = 0

    def __init__(self, num_channels, input_shape, pad_token=-10000, **kwargs):
        if len(input_shape) != self.ndim:
            raise ValueError(f"{type(self).__name__}: input_shape {tuple(input_shape)} does not have {self.ndim} entries")
        self.pad_token = pad_token
        self.shape = (int(num_channels),) + tuple(int(x) for x in input_shape)

    def __call__(self, data):
        samples = data["values"]
        out = _batch_buffer((len(samples),) + self.shape, self.pad_token, torch.float32)
        for i, x in enumerate(samples):
            if x is None:
                continue
            want, got = self.shape, tuple(x.shape)
            if self.ndim == 3 and len(got) == 4:          # the frame axis alone may differ
                want, got = want[:1] + want[2:], got[:1] + got[2:]
            if got != want:
                raise ValueError(f"{type(self).__name__}: sample {i} has shape {tuple(x.shape)}; the modality's samples are "
                                 f"{self.shape}" + (" (any number of frames)" if self.ndim == 3 else ""))
            if self.ndim == 3:
                t = min(x.shape[1], self.shape[1])
                out[i, :, :t] = x[:, :t]
            else:
                out[i] = x
        return {"values": out}


class ImageCollator(PatchNDCollator):
    ndim = 2


class VideoCollator(PatchNDCollator):
    ndim = 3


collators: Dict[str, type] = {
    "matrix": MatrixCollator,
    "sequence": SequenceCollator,
    "embedded_sequence": EmbeddedSequenceCollator,
    "image": ImageCollator,
    "video": VideoCollator,
}


class MultimodalCollator:
    """list of samples {modality: {column: tensor|None}} -> {modality: {name: batched tensor}}
    (encoders.py:374-403)."""

    def __init__(self, modality_config, labels=None, **kwargs):
        self.modality_collators = {name: collators[c["type"]](**c) for name, c in modality_config.items()}
        self.labels = labels

    def __call__(self, batch: List[dict]):
        assert self.modality_collators.keys() <= batch[0].keys(), f"{self.modality_collators.keys()} - {batch[0].keys()}"
        cols = defaultdict(lambda: defaultdict(list))
        for sample in batch:
            for name in self.modality_collators:
                for col, v in sample[name].items():
                    cols[name][col].append(v)
        out = {name: self.modality_collators[name](cols[name]) for name in self.modality_collators}
        if self.labels:
            lab = defaultdict(list)
            for sample in batch:
                for col, v in sample[self.labels].items():
                    lab[col].append(v)
            out[self.labels] = {k: torch.stack(v) for k, v in lab.items()}
        return out
