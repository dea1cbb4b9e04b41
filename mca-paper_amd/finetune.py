"""Supervised fine-tuning: a linear task head over ONE slot of the pooled tokens, trained through the native step.

``FusionEngine.forward_chunk`` gives the pooled tokens (b, R, D) and keeps the activations, ``FusionEngine.backward`` takes the
gradient with respect to them; between the two, ONE kernel call (``mca_task_head_fwd_bwd``, csrc/task_head.hip) turns the pooled
tokens and the labels into the task loss, the head's gradients and d_pooled, added onto the contrastive loss's d_pooled when the
contrastive weight is positive (multi-task).  The objective is

    task_weight * mean element loss over the VALID rows  +  contrastive_weight * contrastive loss

A row is valid when the readout slot has something to read: a modality slot needs that modality present, the fusion slot (or a
combination slot) any of its members (``readout_plan``).  Invalid rows get a prediction but no loss and no gradient.  The head
keeps its own flat fp32 parameter / gradient / moment buffers (``probe.ProbeParams``) and its own AdamW launch; the clip uses ONE
norm over trunk and head gradients together.

``loss_type="CE"`` is softmax cross-entropy over ONE column of class indices (``task >= 0``) with a head of ``num_classes`` (2 .. 64)
outputs, optional ``class_weights`` and ``label_smoothing``: its own kernel call (``mca_class_head_fwd_bwd``, csrc/class_head.hip) in
the same place.  A negative label marks an unlabelled row: it gets a prediction and, with a positive contrastive weight, the
contrastive gradient, but no task loss; the mean is torch's weighted mean over the labelled valid rows.

Not covered: capture as a hipGraph, data parallelism, the gradient-cached form, MLP heads, probability (soft) targets, more than 64
classes, CE over several label columns, EAO models.  INTEGRATION.md section I."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Tuple

import torch
from torch import nn

from . import hip
from .hip import call, ptr, stream_ptr
from .optim import SQNORM_WORDS
from .probe import CE, LOSS_CODES, MAX_L, ProbeParams, check_binary_targets, check_class_targets

FINETUNE_DEFAULTS = {"loss_type": "MSE", "task": 0, "readout": "fusion", "head_lr": None, "task_weight": 1.0, "contrastive_weight": 0.0,
                     "head_warmup_steps": 0}
# the keys of loss_type CE alone; finetune_settings returns them with a CE loss and refuses them with any other
FINETUNE_CE_DEFAULTS = {"num_classes": None, "class_weights": None, "label_smoothing": 0.0}


class TaskHead(nn.Module):
    """``nn.Linear(dim, n_outputs)`` under the key ``head``, created from torch's CPU generator: a seed fixes it"""

    def __init__(self, dim: int, n_outputs: int):
        super().__init__()
        self.head = nn.Linear(dim, n_outputs)


def readout_plan(model, readout) -> Tuple[int, int]:
    """(slot, any_bits) of a readout key of ``model.output_slots()``: the pooled slot the head reads and the presence bits of which
    at least one must be set for a row to count.  A modality slot: that modality's bit.  "fusion" or a combination: the OR of its
    members' bits (the fusion token of a fusion-channel model is its first combination's; otherwise it sees every modality)."""
    slots = model.output_slots()
    if readout not in slots:
        raise KeyError(f"readout {readout!r} is no output slot of the model; known: {list(slots)}")
    names = list(model.modality_types)
    if readout in names:
        members = [names.index(readout)]
    elif readout == "fusion":
        members = sorted(model.fusion_combos[0]) if (model.fcl and not model.zorro) else range(len(names))
    else:
        members = sorted(readout)
    bits = 0
    for m in members:
        bits |= 1 << m
    return slots[readout], bits


def finetune_settings(config) -> Dict[str, object]:
    """The ``finetune:`` mapping of a training YAML over FINETUNE_DEFAULTS; an unknown key is an error that names it.  A ``readout``
    given as a list of modality names is a combination slot."""
    given = config.get("finetune", None) or {}
    if not isinstance(given, dict):
        raise ValueError(f"finetune: must be a mapping, found {type(given).__name__}")
    unknown = sorted(set(given) - set(FINETUNE_DEFAULTS) - set(FINETUNE_CE_DEFAULTS))
    if unknown:
        raise KeyError(f"finetune: unknown keys {unknown}; known: {sorted(FINETUNE_DEFAULTS) + sorted(FINETUNE_CE_DEFAULTS)}")
    out = dict(FINETUNE_DEFAULTS)
    out.update(given)
    if out["loss_type"] == CE:
        for k, v in FINETUNE_CE_DEFAULTS.items():
            out.setdefault(k, v)
        out["num_classes"], out["class_weights"], out["label_smoothing"] = class_settings(out["num_classes"], out["class_weights"],
                                                                                          out["label_smoothing"])
    else:
        stray = sorted(set(given) & set(FINETUNE_CE_DEFAULTS))
        if stray:
            raise ValueError(f"finetune: {stray} belong to loss_type CE, the loss is {out['loss_type']}")
    if isinstance(out["readout"], (list, tuple)):
        names = list((config.get("encoder_configs") or {}).keys())
        out["readout"] = frozenset(names.index(m) if m in names else int(m) for m in out["readout"])
    out["task"], out["head_warmup_steps"] = int(out["task"]), int(out["head_warmup_steps"])
    out["task_weight"], out["contrastive_weight"] = float(out["task_weight"]), float(out["contrastive_weight"])
    out["head_lr"] = None if out["head_lr"] is None else float(out["head_lr"])
    return out


def class_settings(num_classes, class_weights, label_smoothing):
    """(num_classes, class_weights or None, label_smoothing) of a CE head, validated: 2 .. 64 classes, num_classes finite
    non-negative weights that are not all zero, a smoothing in [0, 1)"""
    import math
    if num_classes is None or isinstance(num_classes, bool) or int(num_classes) != num_classes or not 2 <= int(num_classes) <= MAX_L:
        raise ValueError(f"loss_type CE needs num_classes in 2 .. {MAX_L}, found {num_classes!r}")
    num_classes = int(num_classes)
    if class_weights is not None:
        class_weights = [float(v) for v in (class_weights.tolist() if isinstance(class_weights, torch.Tensor) else class_weights)]
        if len(class_weights) != num_classes:
            raise ValueError(f"class_weights has {len(class_weights)} entries for num_classes = {num_classes}")
        if any(not math.isfinite(v) or v < 0 for v in class_weights) or not any(v > 0 for v in class_weights):
            raise ValueError(f"class_weights must be finite, non-negative and not all zero, found {class_weights}")
    label_smoothing = float(label_smoothing)
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"label_smoothing must lie in [0, 1), found {label_smoothing}")
    return num_classes, class_weights, label_smoothing


def refuse_with(n_chunks: int, graph: bool):
    """finetune_accel_gpu.py: the training options the fine-tune step does not combine with, both named in the message"""
    if n_chunks > 1 or graph:
        raise SystemExit("fine-tuning runs eager, one batch per step: grad_cache_chunks > 1 and --graph are not supported "
                         f"(grad_cache_chunks = {n_chunks}, --graph {'given' if graph else 'not given'})")


class FineTuneStep:
    def __init__(self, model, head: TaskHead, optimizer, readout="fusion", loss_type: str = "MSE", task: int = 0, task_weight: float = 1.0,
                 contrastive_weight: float = 0.0, head_lr: Optional[float] = None, clip: float = 2.0, head_warmup_steps: int = 0, dp=None,
                 num_classes: Optional[int] = None, class_weights=None, label_smoothing: float = 0.0):
        eng = model.engine
        if not eng.can_forward_backward():
            raise NotImplementedError("FineTuneStep needs native encoders: a torch encoder's backward runs under autograd "
                                      "(can_forward_backward() is false)")
        world = int(os.environ.get("WORLD_SIZE", 1))
        if dp is not None or world > 1 or eng.gather_hook is not None or eng.grad_bucket_hook is not None:
            raise NotImplementedError(f"FineTuneStep has no data-parallel form (dp object: {dp is not None or eng.gather_hook is not None}, "
                                      f"WORLD_SIZE = {world})")
        if len(eng._captured):
            raise RuntimeError("FineTuneStep: a GraphedStep of this engine is alive and would go on replaying the step it captured; delete it first")
        if eng.eao:
            raise NotImplementedError("FineTuneStep does not take an EAO model: it has no fusion slot and its slots are mean-pooled passes")
        if head.head.in_features != eng.D:
            raise ValueError(f"the head reads {head.head.in_features} features, the pooled tokens have D = {eng.D}")
        if head.head.out_features > MAX_L:
            raise ValueError(f"n_outputs is {head.head.out_features}: the task-head kernel takes at most {MAX_L}")
        if loss_type == CE:
            if head.head.out_features < 2:
                raise NotImplementedError("a one-output head supports L1, MSE and BCE; CE needs a head of num_classes >= 2 outputs")
            num_classes, class_weights, label_smoothing = class_settings(head.head.out_features if num_classes is None else num_classes,
                                                                         class_weights, label_smoothing)
            if head.head.out_features != num_classes:
                raise ValueError(f"num_classes is {num_classes}, the head has {head.head.out_features} outputs")
        elif loss_type not in LOSS_CODES:
            raise NotImplementedError(f"loss_type {loss_type!r}: the fine-tune step supports L1, MSE and BCE (one column or several) and CE")
        elif num_classes is not None or class_weights is not None or label_smoothing:
            raise ValueError(f"num_classes, class_weights and label_smoothing belong to loss_type CE, the loss is {loss_type}")
        task_weight, contrastive_weight = float(task_weight), float(contrastive_weight)
        if task_weight < 0 or contrastive_weight < 0 or not (task_weight == task_weight and contrastive_weight == contrastive_weight):
            raise ValueError(f"task_weight = {task_weight} and contrastive_weight = {contrastive_weight} must not be negative")
        if task_weight == 0 and contrastive_weight == 0:
            raise ValueError("task_weight and contrastive_weight are both 0: the step would have no objective")
        task = int(task)
        if task < -1:
            raise ValueError(f"task is {task}: a label column (>= 0) or -1 for all columns")
        if loss_type == CE and task < 0:
            raise ValueError("loss_type CE with task -1: CE reads one column of class indices (task >= 0)")
        if loss_type != CE and task >= 0 and head.head.out_features != 1:
            raise ValueError(f"task = {task} selects one label column, the head has {head.head.out_features} outputs")
        self.model, self.head, self.opt = model, head, optimizer
        self.slot, self.any_bits = readout_plan(model, readout)
        self.readout, self.loss_type, self.loss_code, self.task = readout, loss_type, LOSS_CODES.get(loss_type), task
        self.num_classes, self.label_smoothing = (num_classes, label_smoothing) if loss_type == CE else (None, 0.0)
        self.class_weights = None          # (C,) fp32 on the device, or None for all ones
        if loss_type == CE and class_weights is not None:
            self.class_weights = torch.tensor(class_weights, dtype=torch.float32, device=eng.device)
        self.task_weight, self.contrastive_weight = task_weight, contrastive_weight
        self.head_lr = None if head_lr is None else float(head_lr)
        self.clip, self.head_warmup_steps = float(clip or 0.0), int(head_warmup_steps)
        self.L, self.D = head.head.out_features, eng.D
        dev = eng.device
        self.params = ProbeParams(head.head, dev)          # flat [weight, bias]; the module's parameters become views of it
        head.head.weight.data, head.head.bias.data = self.params.views[0], self.params.views[1]
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.params.flat), torch.zeros_like(self.params.flat)
        self.sqnorm = torch.zeros(SQNORM_WORDS, dtype=torch.float32, device=dev)
        self.step_count = 0
        self.gnorm = None
        self._ws: Dict[int, torch.Tensor] = {}

    # ---- labels ----------------------------------------------------------------------------------------------------------
    def _label_window(self, labels: torch.Tensor):
        """(fp32 device matrix, byte offset of the window's first column, its row stride): no copy of the columns"""
        y = labels.detach().to(device=self.model.engine.device, dtype=torch.float32)
        y = (y.reshape(-1, 1) if y.dim() < 2 else y.reshape(y.shape[0], -1)).contiguous()
        if self.task >= 0:          # (CE too: its window is the one column of class indices)
            if self.task >= y.shape[1]:
                raise IndexError(f"task = {self.task}: the labels have {y.shape[1]} columns")
            return y, 4 * self.task, y.shape[1]
        if y.shape[1] != self.L:
            raise ValueError(f"task = -1: the labels have {y.shape[1]} columns, the head has {self.L} outputs")
        return y, 0, y.shape[1]

    def check_labels(self, *labels: torch.Tensor):
        """before training: BCE targets must be 0 or 1 in the columns the head is trained on (probe.check_binary_targets), CE targets
        class indices below num_classes or negative for an unlabelled row (probe.check_class_targets)"""
        if self.loss_type == CE:
            cols = []
            for y in labels:
                y = y.reshape(-1, 1) if y.dim() < 2 else y.reshape(y.shape[0], -1)
                cols.append(y[:, self.task])
            check_class_targets(*cols, n_classes=self.num_classes, allow_unlabelled=True)
        if self.loss_type == "BCE":
            cols = []
            for y in labels:
                y = y.reshape(-1, 1) if y.dim() < 2 else y.reshape(y.shape[0], -1)
                cols.append(y[:, self.task] if self.task >= 0 else y)
            check_binary_targets(*cols)

    # ---- the kernel call -------------------------------------------------------------------------------------------------
    def _class_kernel(self, pooled, present, b, y, y_off, ld, d_in, base):
        """mca_class_head_fwd_bwd -> (logits (b, C), loss [mean CE, counted rows, W], d_pooled)"""
        eng, dev = self.model.engine, self.model.engine.device
        if b not in self._ws:
            self._ws[b] = torch.empty(hip.lib().mca_class_head_workspace_bytes(b, self.L, self.D), dtype=torch.uint8, device=dev)
        pred = torch.empty(b, self.L, dtype=torch.float32, device=dev)
        loss = torch.empty(3, dtype=torch.float32, device=dev)
        d_pooled = d_in if d_in is not None else torch.empty(b, eng.R, self.D, dtype=torch.float32, device=dev)
        a = hip.ClassHeadArgs()
        a.pooled, a.present, a.any_bits = ptr(pooled), ptr(present), self.any_bits
        a.b, a.R, a.D, a.slot = b, eng.R, self.D, self.slot
        a.w, a.bias, a.C = ptr(self.params.views[0]), ptr(self.params.views[1]), self.L
        a.labels, a.ld_labels = y.data_ptr() + y_off, ld
        a.class_weights, a.label_smoothing = ptr(self.class_weights), self.label_smoothing
        a.task_weight, a.base_weight = self.task_weight, base
        a.d_pooled_in, a.pred, a.loss, a.d_pooled = ptr(d_in), ptr(pred), ptr(loss), ptr(d_pooled)
        a.gw, a.gb, a.accumulate = ptr(self.params.gviews[0]), ptr(self.params.gviews[1]), 0
        a.workspace, a.workspace_bytes = ptr(self._ws[b]), self._ws[b].numel()
        call("mca_class_head_fwd_bwd", C.byref(a), stream_ptr())
        return pred, loss, d_pooled

    def _task_kernel(self, pooled, present, b, y, y_off, ld, d_in, base):
        if self.loss_type == CE:
            return self._class_kernel(pooled, present, b, y, y_off, ld, d_in, base)
        eng, dev = self.model.engine, self.model.engine.device
        if b not in self._ws:
            self._ws[b] = torch.empty(hip.lib().mca_task_head_workspace_bytes(b, self.L, self.D), dtype=torch.uint8, device=dev)
        pred = torch.empty(b, self.L, dtype=torch.float32, device=dev)
        loss = torch.empty(2, dtype=torch.float32, device=dev)
        d_pooled = d_in if d_in is not None else torch.empty(b, eng.R, self.D, dtype=torch.float32, device=dev)
        a = hip.TaskHeadArgs()
        a.pooled, a.present, a.any_bits = ptr(pooled), ptr(present), self.any_bits
        a.b, a.R, a.D, a.slot = b, eng.R, self.D, self.slot
        a.w, a.bias, a.L = ptr(self.params.views[0]), ptr(self.params.views[1]), self.L
        a.labels, a.ld_labels, a.loss_type = y.data_ptr() + y_off, ld, self.loss_code
        a.task_weight, a.base_weight = self.task_weight, base
        a.d_pooled_in, a.pred, a.loss, a.d_pooled = ptr(d_in), ptr(pred), ptr(loss), ptr(d_pooled)
        a.gw, a.gb, a.accumulate = ptr(self.params.gviews[0]), ptr(self.params.gviews[1]), 0
        a.workspace, a.workspace_bytes = ptr(self._ws[b]), self._ws[b].numel()
        call("mca_task_head_fwd_bwd", C.byref(a), stream_ptr())
        return pred, loss, d_pooled

    # ---- one optimizer step ----------------------------------------------------------------------------------------------
    def step(self, batch, labels):
        """One optimizer step on a batch and its labels ((b,) or (b, columns)).  -> {"loss", "task_loss", "pred", "n_valid",
        "modality_sample_mask"} (+ "contrastive_loss", "losses" with a positive contrastive weight, "modality_dropped" when drawn).
        CE: "pred" holds the logits (b, C) and "n_valid" the counted rows (valid and labelled)."""
        m, eng = self.model, self.model.engine
        if len(eng._captured):
            raise RuntimeError("FineTuneStep.step: a GraphedStep of this engine is alive; delete it first")
        y, y_off, ld = self._label_window(labels)
        cw = self.contrastive_weight
        trunk = self.step_count >= self.head_warmup_steps          # the first head_warmup_steps steps train the head alone
        with hip.cached_stream(), torch.no_grad():
            if eng.check_finite:
                eng.poll_finite()
            if cw > 0:
                ls = m.loss.loss_fn
                ls.logit_scale.data.clamp_(ls.logit_scale_min, ls.logit_scale_max)
            ws, pooled, sample_mask = eng.forward_chunk(batch, 0)
            b = pooled.shape[0]
            if y.shape[0] != b:
                raise ValueError(f"the batch has {b} rows, the labels {y.shape[0]}")
            res = eng.loss_fwd_bwd(pooled, ws["present_cur"], b, 0) if cw > 0 else None
            pred, tl, d_pooled = self._task_kernel(pooled, ws["present_cur"], b, y, y_off, ld, res["d_pooled"] if res else None, cw)
            if eng.check_finite:
                eng._flag_tensors([pred, tl], 2)          # a non-finite label or prediction: the update is skipped, the next poll raises
            skip = ptr(eng.finite_flag) if eng.check_finite else None
            sq = eng._ws.setdefault("sqnorm", torch.zeros(SQNORM_WORDS, dtype=torch.float32, device=eng.device))
            if trunk:
                eng.backward(ws, d_pooled, cw * res["d_logit"] if res else None)
                for p in eng.param_order:
                    p.grad = eng.grad_of(p)
            if self.clip:          # ONE norm over trunk and head: the sum of the two squared norms, formed on the device
                call("mca_grad_sqnorm", ptr(self.params.gflat), self.params.numel, ptr(self.sqnorm), stream_ptr())
                if trunk:
                    call("mca_grad_sqnorm", ptr(eng.gflat), eng.n_params, ptr(sq), stream_ptr())
                    sq[0:1].add_(self.sqnorm[0:1])
                else:
                    sq[0:1].copy_(self.sqnorm[0:1])
                torch.sqrt(sq[0:1], out=sq[SQNORM_WORDS - 1:])
                self.gnorm = sq[SQNORM_WORDS - 1].reshape(())
            else:
                self.gnorm = None
            if trunk:
                eng._pending_clip = self.clip
                self.opt.step()
            g = self.opt.param_groups[0]
            t = self.step_count + 1
            lr = g["lr"] if self.head_lr is None else self.head_lr
            call("mca_adamw_step", ptr(self.params.flat), ptr(self.params.gflat), ptr(self.exp_avg), ptr(self.exp_avg_sq), self.params.numel,
                 float(lr), 0.9, 0.999, 1e-8, 0.01, 1.0 - 0.9 ** t, 1.0 - 0.999 ** t, self.clip, ptr(sq) if self.clip else None, skip, None,
                 stream_ptr())
            self.step_count = t
            eng.advance_modality_dropout()
            eng.publish_flags()
        out = {"task_loss": tl[0], "n_valid": tl[1], "pred": pred, "modality_sample_mask": sample_mask}
        if res is not None:
            terms = res["term_loss"]
            out["contrastive_loss"] = res["loss"].reshape(())
            out["losses"] = {t.name: terms[i] for i, t in enumerate(m.loss_terms)}
            out["loss"] = self.task_weight * tl[0] + cw * out["contrastive_loss"]
        else:
            out["loss"] = self.task_weight * tl[0]
        if ws["dropped_cur"] is not None:
            out["modality_dropped"] = ws["dropped_cur"]
        if eng.check_finite and eng.check_finite != "deferred":
            eng.assert_finite()
        return out

    # ---- evaluation ------------------------------------------------------------------------------------------------------
    def predict(self, batch):
        """-> (pred (b, L), valid (b,) bool): the head (mca_probe_nt_f32 on the readout slot) on the eval-mode forward; no gradients, no
        modality dropout"""
        m, eng = self.model, self.model.engine
        was_training = m.training
        m.eval()
        try:
            with hip.cached_stream(), torch.no_grad():
                ws, pooled, _ = eng.forward_chunk(batch, 0)
                b = pooled.shape[0]
                pred = torch.empty(b, self.L, dtype=torch.float32, device=eng.device)
                call("mca_probe_nt_f32", pooled.data_ptr() + 4 * self.slot * self.D, eng.R * self.D, None, ptr(self.params.views[0]), self.D,
                     ptr(self.params.views[1]), ptr(pred), self.L, b, self.L, self.D, 0, 0.0, 0, 0, stream_ptr())
                valid = (ws["present_cur"] & self.any_bits) != 0 if self.any_bits else torch.ones(b, dtype=torch.bool, device=eng.device)
        finally:
            if was_training:
                m.train()
        return pred, valid

    # ---- state -----------------------------------------------------------------------------------------------------------
    def state_dict(self):
        return {"head": {k: v.detach().clone() for k, v in self.head.state_dict().items()}, "exp_avg": self.exp_avg.clone(),
                "exp_avg_sq": self.exp_avg_sq.clone(), "step": self.step_count}

    def load_state_dict(self, sd):
        self.params.views[0].copy_(sd["head"]["head.weight"]); self.params.views[1].copy_(sd["head"]["head.bias"])
        self.exp_avg.copy_(sd["exp_avg"]); self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.step_count = int(sd["step"])


__all__ = ["TaskHead", "FineTuneStep", "readout_plan", "finetune_settings", "class_settings", "refuse_with", "FINETUNE_DEFAULTS",
           "FINETUNE_CE_DEFAULTS"]
