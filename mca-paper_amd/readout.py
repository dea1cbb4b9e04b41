"""Attention readout: where the rows of an attention looked, by key group, without the (b, h, N, N) matrix.

The reference's ``Attention.forward`` can return its probabilities (``return_attn=True``, model.py:87-103).  The native path
keeps ``o`` and the log-sum-exp only; ``mca_attn_readout`` (csrc/attention_readout.hip) rebuilds the probabilities tile by tile
from the saved q / k and that log-sum-exp and sums them per key group: modality ``m`` is group ``m``, fusion sub-block ``c`` is
group ``M + c`` (structure.py).  Imports without a GPU and without loading the library."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Optional

import numpy as np
import torch

from . import attention, hip
from .structure import FusionStructure


def group_names(model) -> List[object]:
    """One name per key group, in group-id order: the modality names, then one entry per fusion group - its combination of
    modality indices (a frozenset, as in ``output_slots()``) for a fusion-channel (fcl) structure, ``"fusion"`` otherwise."""
    st = model.structure
    M = len(model.modality_types)
    names: List[object] = list(model.modality_types)
    n_fusion_groups = st.n_groups - M
    if model.fcl and not model.zorro and n_fusion_groups == len(st.combos):
        names += list(st.combos)
    else:
        names += ["fusion"] * n_fusion_groups
    return names


def uniform_mass(st: FusionStructure) -> np.ndarray:
    """(G,) fp32: the group shares of a fully masked row.  The reference's softmax of such a row is uniform over ALL N keys,
    padded and blocked ones included, so a group's share is its key count over N."""
    counts = np.bincount(st.kgroup.astype(np.int64), minlength=st.n_groups)[:st.n_groups]
    return (counts.astype(np.float64) / float(len(st.kgroup))).astype(np.float32)


def slot_mass(pool_mass: torch.Tensor, slots: Dict[object, int]) -> Dict[object, torch.Tensor]:
    """{slot: (b, G)}: the head mean of the pooling row behind every output slot.  pool_mass: (b, H, R, G)."""
    return {k: pool_mass[:, :, row].mean(dim=1) for k, row in slots.items()}


def launch(engine, ops, ws, mass: torch.Tensor, um: torch.Tensor, probs: Optional[torch.Tensor] = None, row0: int = 0):
    """one mca_attn_readout launch on the operands of an attention whose forward has run (ops: attention.AttnOperands)"""
    if ops.hstride:
        raise hip.MCAHipError("mca_attn_readout reads row-major q | k: run the forward with engine.rows_only set (attention_readout does)")
    a = attention.readout_args(ops, engine.attn_keys(ws), um, mass, probs, row0)
    hip.call("mca_attn_readout", C.byref(a), hip.stream_ptr())


def attention_readout(model, batch, layers: Optional[Iterable[int]] = None, pool: bool = True, probs_rows: Optional[dict] = None) -> dict:
    """See ``MCA.attention_readout``."""
    if model.attn_pool is None:
        raise NotImplementedError("attention readout of an EAO model: its attention is block-diagonal by construction "
                                  "(every segment sees itself only)")
    eng = model.engine
    if eng.attn_dtype == "fp8":
        raise NotImplementedError("attention readout on an engine running fp8 attention: its log-sum-exp carries the fp8 forward's "
                                  "error (set_attention_dtype('bf16') first)")
    layers = list(range(eng.L)) if layers is None else [int(i) for i in layers]
    for i in layers:
        if not 0 <= i < eng.L:
            raise IndexError(f"layer {i} of {eng.L}")
    probs_rows = dict(probs_rows or {})
    for key, (row0, n) in probs_rows.items():
        nq = eng.R if key == "pool" else eng.N
        if not (key == "pool" and pool) and key not in layers:
            raise KeyError(f"probs_rows[{key!r}]: not among the requested attentions")
        if row0 < 0 or n <= 0 or row0 + n > nq:
            raise IndexError(f"probs_rows[{key!r}] = ({row0}, {n}) outside [0, {nq})")
    # (mca_attn_readout takes q | k as row-major matrices: this forward keeps them so at every batch size)
    rows_only, eng.rows_only = eng.rows_only, True
    try:
        with torch.no_grad():
            out = model(batch, no_loss=True)
    finally:
        eng.rows_only = rows_only
    b = next(iter(out["modality_sample_mask"].values())).shape[0]
    ws = eng.workspace(b)
    dev, H, N, R = eng.device, eng.H, eng.N, eng.R
    um = torch.from_numpy(uniform_mass(eng.st)).to(dev)
    G = um.numel()
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    res = {"groups": group_names(model), "layer_mass": {}, "pool_mass": None, "slot_mass": {},
           "modality_sample_mask": out["modality_sample_mask"]}
    probs = {}
    with hip.cached_stream():
        for i in layers:
            mass = f32(b, H, N, G)
            pr = f32(b, H, probs_rows[i][1], N) if i in probs_rows else None
            launch(eng, eng.layer_attention(ws, i)[0], ws, mass, um, pr, probs_rows[i][0] if pr is not None else 0)
            res["layer_mass"][i] = mass
            if pr is not None:
                probs[i] = pr
        if pool:
            mass = f32(b, H, R, G)
            pr = f32(b, H, probs_rows["pool"][1], N) if "pool" in probs_rows else None
            launch(eng, eng.pool_attention(ws)[0], ws, mass, um, pr, probs_rows["pool"][0] if pr is not None else 0)
            res["pool_mass"] = mass
            res["slot_mass"] = slot_mass(mass, model.output_slots())
            if pr is not None:
                probs["pool"] = pr
    if probs_rows:
        res["probs"] = probs
    return res
