"""A gradient-cached training step (GradCache): one optimizer step on a contrastive batch of B = n * micro_batch samples with the
activation memory of ONE micro-batch.

The objective is an all-pairs contrastive loss: every other sample of the batch is a negative, so the batch size is a modelling
choice.  The parameters reach the loss only through the pooled tokens and logit_scale, and the forward is bitwise reproducible, so
the step splits exactly:

  pass 1   chunks 0 .. n-1: forward to the pooled tokens; the (micro_batch, R, D) rows and the presence words go into a (B, R, D)
           bank, the activations are dropped (the last chunk's stay in the workspace);
  loss     ONE call over the bank as one rank of B rows: every row's negatives are all B rows, n_{t,r} counts over all B rows;
           it also returns d loss / d bank and d loss / d logit_scale;
  pass 2   chunks n-1 .. 0: forward again (not for chunk n-1), then the engine's backward with the chunk's rows of d loss / d bank,
           adding into the flat gradient buffer: 2n - 1 forwards and n backwards;
  then the gradient norm, the clip and the optimizer step, as graph.GraphedStep orders them.

The sum of the chunks' gradients is the gradient of the one step on B samples, up to the order of the additions; in deterministic
mode the chunk order and every sum inside a chunk are fixed, so a step repeats bit for bit.  The modality dropout draws chunk i at
sample0 = i * micro_batch with the step counter held, so both passes see the same masks and the n chunks draw the rows of the one
draw on B samples; the counter then advances once per step.  The finite and index flags of every chunk of both passes are OR-ed
into the engine's one device word, which nothing clears between chunks: FusedAdamW skips the update of a flagged step.

Not covered: data parallelism, capture as a hipGraph, torch encoders.  INTEGRATION.md section H."""
from __future__ import annotations

import os
from typing import List, Sequence, Tuple

import torch

from . import hip
from . import optim as _optim
from .engine import FLAG_CACHE_MISMATCH
from .hip import call, ptr, stream_ptr


def chunk_plan(B: int, micro_batch: int) -> List[Tuple[int, int]]:
    """[(first row, past-the-last row)] of the chunks of a batch of B rows; B must be a positive multiple of micro_batch"""
    if micro_batch <= 0:
        raise ValueError(f"micro_batch is {micro_batch}: it must be positive")
    if B <= 0 or B % micro_batch:
        raise ValueError(f"the batch has {B} rows, which is no positive multiple of micro_batch = {micro_batch}")
    return [(i, i + micro_batch) for i in range(0, B, micro_batch)]


def pass_plan(n: int) -> List[Tuple[str, int]]:
    """The launches of one step over n chunks, in order: ("forward", i) / ("loss", -1) / ("backward", i).  2n - 1 forwards: the last
    chunk of pass 1 is the first of pass 2 and is not run again."""
    plan = [("forward", i) for i in range(n)] + [("loss", -1)]
    for i in reversed(range(n)):
        if i != n - 1:
            plan.append(("forward", i))
        plan.append(("backward", i))
    return plan


def grad_cache_chunks(config) -> int:
    """the YAML key grad_cache_chunks (absent: 1); anything but a positive integer is an error"""
    n = config.get("grad_cache_chunks", 1)
    if n is None:
        return 1
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"grad_cache_chunks is {n!r}: it must be a positive integer")
    return n


def refuse_with(n: int, graph: bool, world: int):
    """train_accel_gpu.py: the options the gradient-cached step does not combine with, named together in the message"""
    if n > 1 and graph:
        raise SystemExit("grad_cache_chunks > 1 and --graph cannot be combined: the gradient-cached step is not captured as a hipGraph")
    if n > 1 and world > 1:
        raise SystemExit(f"grad_cache_chunks > 1 and more than one rank (WORLD_SIZE = {world}) cannot be combined: the gradient-cached step "
                         "has no data-parallel form")


def _leading(batch) -> int:
    return next(iter(next(iter(batch.values())).values())).shape[0]


def _rows(batch, lo: int, hi: int):
    """rows lo .. hi - 1 of every tensor of a batch dict, as views"""
    return {k: {kk: (vv[lo:hi] if torch.is_tensor(vv) else vv) for kk, vv in v.items()} for k, v in batch.items()}


class CachedStep:
    def __init__(self, model, optimizer, micro_batch: int, clip: float = 2.0, loss_kernel: str = "auto", verify: bool = False, dp=None):
        eng = model.engine
        if not eng.can_forward_backward():
            raise NotImplementedError("CachedStep needs native encoders: a torch encoder's backward runs under autograd "
                                      "(can_forward_backward() is false)")
        world = int(os.environ.get("WORLD_SIZE", 1))
        if dp is not None or world > 1 or eng.gather_hook is not None or eng.grad_bucket_hook is not None:
            raise NotImplementedError(f"CachedStep has no data-parallel form (dp object: {dp is not None or eng.gather_hook is not None}, "
                                      f"WORLD_SIZE = {world})")
        if len(eng._captured):
            raise RuntimeError("CachedStep: a GraphedStep of this engine is alive and would go on replaying the step it captured; delete it first")
        if loss_kernel not in ("auto", "dense", "stream"):
            raise ValueError(f"loss_kernel is '{loss_kernel}', not one of auto, dense, stream")
        if int(micro_batch) <= 0:
            raise ValueError(f"micro_batch is {micro_batch}: it must be positive")
        self.model, self.opt, self.micro_batch, self.clip = model, optimizer, int(micro_batch), float(clip or 0.0)
        self.loss_kernel, self.verify = loss_kernel, bool(verify)
        self.gnorm = None
        self.last_kernel = None          # the loss kernel the last step ran

    def _chunks(self, batch):
        mb = self.micro_batch
        if isinstance(batch, dict):
            plan = chunk_plan(_leading(batch), mb)
            return [_rows(batch, lo, hi) for lo, hi in plan]
        chunks = list(batch)
        for i, c in enumerate(chunks):
            if _leading(c) != mb:
                raise ValueError(f"micro-batch {i} has {_leading(c)} rows, not micro_batch = {mb}")
        if not chunks:
            raise ValueError("the batch has 0 rows, which is no positive multiple of micro_batch")
        return chunks

    def step(self, batch):
        """One optimizer step on the whole batch.  -> what model(batch) returns, for all B rows."""
        eng, m, mb = self.model.engine, self.model, self.micro_batch
        if len(eng._captured):
            raise RuntimeError("CachedStep.step: a GraphedStep of this engine is alive; delete it first")
        chunks = self._chunks(batch)          # (refuses a batch that is no multiple of micro_batch before anything is launched)
        n, B, R, D, dev = len(chunks), len(chunks) * mb, eng.R, eng.D, eng.device
        kernel = eng.loss_kernel_for(B, self.loss_kernel)
        with hip.cached_stream(), torch.no_grad():
            if eng.check_finite:
                eng.poll_finite()
            ls = m.loss.loss_fn
            ls.logit_scale.data.clamp_(ls.logit_scale_min, ls.logit_scale_max)
            # a fresh bank per step: the outputs handed to the caller are views of it
            bank = torch.empty(B, R, D, dtype=torch.float32, device=dev)
            present = torch.empty(B, dtype=torch.int32, device=dev)
            dropped = torch.empty(B, dtype=torch.int32, device=dev) if (eng._mdrop is not None and m.training) else None
            ws = None
            for i, ch in enumerate(chunks):
                ws, pooled, _ = eng.forward_chunk(ch, i * mb)
                call("mca_rows_copy_add", ptr(pooled), 0, bank.data_ptr() + i * mb * R * D * 4, 0, mb * R, D, 1, 0, stream_ptr())
                self._copy_words(ws["present_cur"], present, i)
                if dropped is not None:
                    self._copy_words(ws["dropped"], dropped, i)
            res = eng.loss_fwd_bwd_bank(bank, present, kernel)
            for k, i in enumerate(reversed(range(n))):
                if k:          # the last chunk's activations are still in the workspace
                    ws, pooled, _ = eng.forward_chunk(chunks[i], i * mb)
                    if self.verify:
                        differs = (pooled.view(torch.int32) != bank[i * mb:(i + 1) * mb].view(torch.int32)).any()
                        eng.finite_flag.bitwise_or_(differs.to(torch.int32) * FLAG_CACHE_MISMATCH)
                eng.backward(ws, res["d_pooled"][i * mb:(i + 1) * mb], res["d_logit"] if k == 0 else None, accumulate=k > 0)
            for p in eng.param_order:
                p.grad = eng.grad_of(p)
            self.gnorm = _optim.clip_grad_norm_(m, self.clip) if self.clip else None
            self.opt.step()
            eng.advance_modality_dropout()
            eng.publish_flags()
        self.last_kernel = kernel
        out = {k: bank[:, s] for k, s in m.output_slots().items()}
        terms = res["term_loss"]
        names = [t.name for t in m.loss_terms]
        out["losses"] = {nm: terms[i] for i, nm in enumerate(names)}
        if m.fcl and not m.zorro:
            fc = torch.tensor([1.0 if "fcl" in nm else 0.0 for nm in names], dtype=torch.float32, device=dev)
            w = torch.stack([fc / fc.sum().clamp(min=1), (1 - fc) / (1 - fc).sum().clamp(min=1)])
            both = (torch.nan_to_num(terms)[None, :] * w).sum(1)
            out["fcl_loss"], out["no-fcl_loss"] = both[0], both[1]
        out["loss"] = res["loss"].reshape(())
        bits = ((present[:, None] >> eng._mod_shifts) & 1).to(torch.bool)
        out["modality_sample_mask"] = {name: bits[:, mi] for mi, name in enumerate(m.modality_types)}
        if dropped is not None:
            out["modality_dropped"] = ((dropped[:, None] >> eng._mod_shifts) & 1).to(torch.bool)
        if eng.check_finite and eng.check_finite != "deferred":
            eng.assert_finite()
        return out

    def _copy_words(self, src, bank, i):
        """the chunk's micro_batch int32 words into their place in a (B,) bank: by the copy kernel where its 16-byte rule allows"""
        mb = self.micro_batch
        if mb % 4 == 0:
            call("mca_rows_copy_add", ptr(src), 0, bank.data_ptr() + i * mb * 4, 0, 1, mb, 1, 0, stream_ptr())
        else:
            bank[i * mb:(i + 1) * mb].copy_(src)
