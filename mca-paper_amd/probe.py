"""The linear / MLP probe of the reference's lp_accel_gpu.py (lines 117-186) on HIP kernels (csrc/evaluate.hip).

Parameters live in ONE flat fp32 buffer (gradients in a second one) in ``nn`` order: ``nn.Linear(D, L)`` is [weight, bias],
the MLP ``Linear(D, H) -> Dropout -> ReLU -> Linear(H, L)`` is [W1, b1, W2, b2].  ``parameters()`` gives views of it whose
``.grad`` are views of the gradient buffer, so the ``utils.training`` norms work unchanged.  A step is: the layer kernels
(gather of the batch rows through the epoch's permutation, logits, loss, its gradient, predictions into an epoch buffer),
the weight gradients as per-chunk partials added in a fixed order, the batch loss added to a device accumulator, then the
existing ``mca_grad_sqnorm`` + ``mca_adamw_step`` (clip_grad_norm_ + AdamW with torch's defaults) reading the step's LR and
bias corrections from a device table written once.  Nothing inside an epoch reads the device from the host.
``loss_type="CE"`` (softmax cross-entropy over one column of class indices, a head of ``n_classes`` outputs) swaps the head kernel
for ``mca_probe_head_ce_f32`` (csrc/class_head.hip) and the metrics for ``metrics.multiclass_metrics``; the rest of the step is shared.

Host RNG: the permutations come from torch's own DataLoader over row indices (``EpochSampler``), drawn from the global CPU
generator in the reference's order, and the initial weights are ``nn.Linear``'s own.  The dropout mask is a counter-based
hash of (seed, optimizer step, row in the batch, hidden unit): torch's device generator cannot be reproduced."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional

import torch
from torch import nn

from . import metrics as M
from .hip import call, lib, ptr, stream_ptr
from .optim import SQNORM_WORDS

LOSS_CODES = {"L1": 0, "MSE": 1, "BCE": 2}
CE = "CE"          # softmax cross-entropy over class-index labels: its own kernel (mca_probe_head_ce_f32), no code of the above
MAX_D, MAX_L, MAX_H, MAX_B = 1024, 64, 1024, 4096


def build_module(model_type: str, d: int, hidden: int, n_labels: int, dropout: float) -> Optional[nn.Module]:
    """lp_accel_gpu.py:125-133: the probe as the reference builds it (on the CPU generator); None for any other model type
    (the reference exits there)."""
    if model_type == "linear":
        return nn.Linear(d, n_labels)
    if model_type.lower() == "mlp":
        return nn.Sequential(nn.Linear(d, hidden), nn.Dropout(dropout), nn.ReLU(), nn.Linear(hidden, n_labels))
    return None


class EpochSampler:
    """The reference's two loaders over row indices (lp_accel_gpu.py:117-118): ``draw()`` runs one epoch's shuffled train
    iterator to the end (one base-seed draw at iterator creation, one sampler seed at its first advance) and creates the eval
    iterator (one more base-seed draw).  ``first_batch()`` is the ``next(iter(train_dl))`` made before the model is built."""

    def __init__(self, n_train: int, n_eval: int, batch_size: int):
        from torch.utils.data import DataLoader
        self.train_dl = DataLoader(range(n_train), batch_size=batch_size, shuffle=True)
        self.eval_dl = DataLoader(range(n_eval), batch_size=batch_size)

    def first_batch(self) -> torch.Tensor:
        return next(iter(self.train_dl))

    def draw(self) -> torch.Tensor:
        perm = torch.cat(list(self.train_dl))
        iter(self.eval_dl)
        return perm


class ProbeParams:
    """Flat fp32 parameter / gradient buffers with ``nn``-ordered views (see the module docstring)."""

    def __init__(self, module: nn.Module, device):
        ts = [p.detach().float().cpu() for p in module.parameters()]
        self.numel = sum(t.numel() for t in ts)
        self.flat = torch.zeros(self.numel, dtype=torch.float32, device=device)
        self.gflat = torch.zeros_like(self.flat)
        self.views: List[torch.Tensor] = []
        self.gviews: List[torch.Tensor] = []
        self._params: List[nn.Parameter] = []
        o = 0
        for t in ts:
            v, g = self.flat[o:o + t.numel()].view(t.shape), self.gflat[o:o + t.numel()].view(t.shape)
            v.copy_(t)
            p = nn.Parameter(v, requires_grad=False)
            p.grad = g
            self.views.append(v); self.gviews.append(g); self._params.append(p)
            o += t.numel()

    def parameters(self):
        return iter(self._params)


class Probe:
    """One probe run: ``train_epoch`` / ``eval_epoch`` enqueue an epoch's kernels, ``epoch_record`` reads the log record back
    with one device-to-host copy."""

    def __init__(self, module: nn.Module, model_type: str, loss_type: str, x_train, y_train, x_eval, y_eval, batch_size: int,
                 lr: float, lr_at: Callable[[int], float], total_steps: int, clip: float, dropout: float, seed: int, device):
        if loss_type not in LOSS_CODES and loss_type != CE:
            raise NotImplementedError(f"loss_type {loss_type!r}: the probe supports L1, MSE, BCE and CE")
        self.kind = "linear" if model_type == "linear" else "mlp"
        self.loss_type, self.loss_code = loss_type, LOSS_CODES.get(loss_type)
        self.device = device
        self.x_train, self.x_eval = self._rows(x_train), self._rows(x_eval)
        self.y_train, self.y_eval = self._rows(y_train), self._rows(y_eval)
        self.B = int(batch_size)
        self.params = ProbeParams(module, device)
        # L is the head's width: the label columns, or for CE the classes (the module's outputs) over ONE column of class indices
        self.D, self.L = self.x_train.shape[1], (self.params.views[-1].shape[0] if loss_type == CE else self.y_train.shape[1])
        if loss_type == CE and (self.y_train.shape[1] != 1 or self.L < 2):
            raise ValueError(f"CE probe: one column of class indices and a head of >= 2 classes, found {self.y_train.shape[1]} columns and "
                             f"{self.L} outputs")
        self.H = self.params.views[0].shape[0] if self.kind == "mlp" else 0
        if self.D > MAX_D or self.L > MAX_L or self.H > MAX_H or self.B > MAX_B or self.B < 1:
            raise ValueError(f"probe sizes D={self.D} (<= {MAX_D}), L={self.L} (<= {MAX_L}), H={self.H} (<= {MAX_H}), "
                             f"batch {self.B} (1 .. {MAX_B}) out of range")
        self.n_out = 1 if loss_type == CE else self.L          # loss elements a row: the mean's divisor is b * n_out
        self.clip, self.dropout, self.seed = float(clip), float(dropout), int(seed)
        self.n_train, self.n_eval = self.x_train.shape[0], self.x_eval.shape[0]
        self.steps_per_epoch = (self.n_train + self.B - 1) // self.B
        self.eval_steps = (self.n_eval + self.B - 1) // self.B
        self.step = 0
        f32 = dict(dtype=torch.float32, device=device)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.params.flat), torch.zeros_like(self.params.flat)
        self.sqnorm = torch.zeros(SQNORM_WORDS, **f32)
        # {lr, 1 - b1^t, 1 - b2^t} of every optimizer step, written once (the scheduler steps after every optimizer step)
        table = torch.tensor([[lr * lr_at(s), 1.0 - 0.9 ** (s + 1), 1.0 - 0.999 ** (s + 1)] for s in range(total_steps)],
                             dtype=torch.float32).reshape(-1, 3)
        self.hyper = table.to(device)
        self.acc = torch.zeros(2, **f32)                                # train / eval sum of the batch mean losses
        self.pred_train = torch.zeros(self.n_train, self.L, **f32)
        self.pred_eval = torch.zeros(self.n_eval, self.L, **f32)
        self.dz = torch.zeros(self.B, self.L, **f32)
        self.part = torch.zeros(lib().mca_probe_head_blocks(self.B), **f32)
        if self.kind == "mlp":
            self.hid = torch.zeros(self.B, self.H, **f32)
            self.dhid = torch.zeros(self.B, self.H, **f32)
            ws = max(lib().mca_probe_tn_workspace(self.B, self.H, self.D), lib().mca_probe_tn_workspace(self.B, self.L, self.H))
        else:
            ws = lib().mca_probe_tn_workspace(self.B, self.L, self.D)
        self.ws = torch.zeros(ws, **f32)
        self.perm_host = torch.zeros(self.n_train, dtype=torch.int32).pin_memory()
        self.perm = torch.zeros(self.n_train, dtype=torch.int32, device=device)
        self.perm_long: Optional[torch.Tensor] = None

    def _rows(self, t: torch.Tensor) -> torch.Tensor:
        t = t.detach().to(device=self.device, dtype=torch.float32)
        return (t.reshape(-1, 1) if t.dim() < 2 else t).contiguous()

    def parameters(self):
        return self.params.parameters()

    # ---- one epoch -------------------------------------------------------------------------------------------------------
    def _forward(self, x, xidx, labels, yidx, b, pred, train: bool):
        """the layer kernels of one batch of b rows; returns the number of loss partials written"""
        st = stream_ptr()
        v = self.params.views
        if self.loss_type == CE:
            a, lda, aidx, k, w, bias, da, scale = x.data_ptr(), self.D, xidx, self.D, ptr(v[0]), ptr(v[1]), None, 0.0
            if self.kind == "mlp":
                call("mca_probe_nt_f32", x.data_ptr(), self.D, xidx, ptr(v[0]), self.D, ptr(v[1]), ptr(self.hid), self.H, b, self.H, self.D,
                     2 if train else 1, self.dropout, self.seed & 0xFFFFFFFFFFFFFFFF, self.step, st)
                scale = 1.0 / (1.0 - self.dropout) if self.dropout < 1.0 else 0.0
                a, lda, aidx, k, w, bias, da = ptr(self.hid), self.H, None, self.H, ptr(v[2]), ptr(v[3]), ptr(self.dhid) if train else None
            call("mca_probe_head_ce_f32", a, lda, aidx, k, w, bias, self.L, labels.data_ptr(), 1, yidx, b, pred,
                 ptr(self.dz) if train else None, da, scale, ptr(self.part), st)
        elif self.kind == "linear":
            call("mca_probe_head_f32", x.data_ptr(), self.D, xidx, self.D, ptr(v[0]), ptr(v[1]), self.L, labels.data_ptr(), yidx, b,
                 self.loss_code, pred, ptr(self.dz) if train else None, None, 0.0, ptr(self.part), st)
        else:
            call("mca_probe_nt_f32", x.data_ptr(), self.D, xidx, ptr(v[0]), self.D, ptr(v[1]), ptr(self.hid), self.H, b, self.H, self.D,
                 2 if train else 1, self.dropout, self.seed & 0xFFFFFFFFFFFFFFFF, self.step, st)
            scale = 1.0 / (1.0 - self.dropout) if self.dropout < 1.0 else 0.0
            call("mca_probe_head_f32", ptr(self.hid), self.H, None, self.H, ptr(v[2]), ptr(v[3]), self.L, labels.data_ptr(), yidx, b,
                 self.loss_code, pred, ptr(self.dz) if train else None, ptr(self.dhid) if train else None, scale, ptr(self.part), st)
        return lib().mca_probe_head_blocks(b)

    def train_epoch(self, perm: torch.Tensor):
        """perm: this epoch's row order (the shuffled train loader's indices)."""
        st = stream_ptr()
        self.perm_host.copy_(perm.to(torch.int32))          # the previous epoch's copy completed before its record was read
        self.perm.copy_(self.perm_host, non_blocking=True)
        self.perm_long = None
        self.acc.zero_()
        g = self.params.gviews
        for s in range(self.steps_per_epoch):
            r0 = s * self.B
            b = min(self.B, self.n_train - r0)
            rows = self.perm.data_ptr() + 4 * r0
            nb = self._forward(self.x_train, rows, self.y_train, rows, b, self.pred_train.data_ptr() + 4 * r0 * self.L, True)
            if self.kind == "linear":
                call("mca_probe_tn_f32", ptr(self.dz), self.L, self.x_train.data_ptr(), self.D, rows, b, self.L, self.D, ptr(self.ws),
                     self.ws.numel(), ptr(g[0]), ptr(g[1]), st)
            else:
                call("mca_probe_tn_f32", ptr(self.dz), self.L, ptr(self.hid), self.H, None, b, self.L, self.H, ptr(self.ws),
                     self.ws.numel(), ptr(g[2]), ptr(g[3]), st)
                call("mca_probe_tn_f32", ptr(self.dhid), self.H, self.x_train.data_ptr(), self.D, rows, b, self.H, self.D, ptr(self.ws),
                     self.ws.numel(), ptr(g[0]), ptr(g[1]), st)
            call("mca_probe_loss_accum", ptr(self.part), nb, b * self.n_out, ptr(self.acc), st)
            self._optimizer_step()

    def _optimizer_step(self):
        st = stream_ptr()
        n = self.params.numel
        if self.clip > 0:
            call("mca_grad_sqnorm", ptr(self.params.gflat), n, ptr(self.sqnorm), st)
        h = self.hyper[self.step]
        call("mca_adamw_step", ptr(self.params.flat), ptr(self.params.gflat), ptr(self.exp_avg), ptr(self.exp_avg_sq), n,
             0.0, 0.9, 0.999, 1e-8, 0.01, 1.0, 1.0, self.clip if self.clip > 0 else 0.0, ptr(self.sqnorm) if self.clip > 0 else None,
             None, h.data_ptr(), st)
        self.step += 1

    def eval_epoch(self):
        """the eval rows in order, no dropout, no gradients"""
        for s in range(self.eval_steps):
            r0 = s * self.B
            b = min(self.B, self.n_eval - r0)
            nb = self._forward(self.x_eval[r0:], None, self.y_eval[r0:], None, b, self.pred_eval.data_ptr() + 4 * r0 * self.L, False)
            call("mca_probe_loss_accum", ptr(self.part), nb, b * self.n_out, self.acc.data_ptr() + 4, stream_ptr())

    # ---- the log record --------------------------------------------------------------------------------------------------
    def _metrics(self, pred, labels) -> Dict[str, torch.Tensor]:
        if self.loss_type == "BCE":
            return M.binary_metrics(M.binary_format(pred, self.B, self.L), labels)
        if self.loss_type == CE:
            return M.multiclass_metrics(torch.softmax(pred.double(), 1), labels.reshape(-1))
        return {"PCC": M.pearson(pred, labels)}

    def epoch_device_values(self) -> Dict[str, torch.Tensor]:
        """every value of the epoch's record as device tensors (no sync)"""
        from utils.training import get_grad_norm, get_param_norm
        if self.perm_long is None:
            self.perm_long = self.perm.long()
        vals = {"train_loss": self.acc[0] / self.steps_per_epoch, "eval_loss": self.acc[1] / self.eval_steps,
                "param_norm": get_param_norm(self).reshape(()), "grad_norm": get_grad_norm(self).reshape(())}
        if self.clip > 0:          # torch scales the gradients in place by the clip coefficient; the fused AdamW applies it on the fly
            coef = torch.clamp(self.clip / (self.sqnorm[0].sqrt() + 1e-6), max=1.0)
            vals["grad_norm"] = vals["grad_norm"] * coef
        for k, v in self._metrics(self.pred_train, self.y_train[self.perm_long]).items():
            vals[f"train_{k}"] = v
        for k, v in self._metrics(self.pred_eval, self.y_eval).items():
            vals[f"eval_{k}"] = v
        return vals

    @staticmethod
    def read(vals: Dict[str, torch.Tensor]) -> Dict[str, object]:
        """ONE device-to-host copy of the whole record"""
        flat = torch.cat([v.reshape(-1).double() for v in vals.values()]).cpu().tolist()
        out, o = {}, 0
        for k, v in vals.items():
            n = v.numel()
            if k.endswith("_cm"):
                side = v.shape[0]          # (2, 2) binary, (C, C) multiclass
                out[k] = [[int(flat[o + i * side + j]) for j in range(side)] for i in range(side)]
            else:
                out[k] = flat[o]
            o += n
        return out


def check_binary_targets(*labels: torch.Tensor):
    """BCE targets must be 0 or 1 (torchmetrics' binary metrics reject anything else at the first update); raises before the
    first step, naming the offending values."""
    for y in labels:
        bad = torch.unique(y[(y != 0) & (y != 1)])
        if bad.numel():
            raise ValueError(f"BCE probe: targets must be 0 or 1, found {bad[:8].tolist()}"
                             f"{' ...' if bad.numel() > 8 else ''} (binarise the labels first)")


def check_class_targets(*labels: torch.Tensor, n_classes: int, allow_unlabelled: bool = False):
    """CE targets must be class indices: integer values in [0, n_classes) (a negative value marks an unlabelled row where
    ``allow_unlabelled``); raises before the first step, naming up to 8 offending values."""
    for y in labels:
        y = y.detach().reshape(-1).double()
        bad = ~(y == y.floor()) | (y >= n_classes)          # (NaN is no integer)
        if not allow_unlabelled:
            bad |= y < 0
        vals = torch.unique(y[bad])
        if vals.numel():
            raise ValueError(f"CE targets must be class indices 0 .. {n_classes - 1}"
                             f"{' (or negative: unlabelled)' if allow_unlabelled else ''}, found {vals[:8].tolist()}"
                             f"{' ...' if vals.numel() > 8 else ''}")


def plan(cfg, n_labels_all: Optional[int] = None, n_classes: Optional[int] = None) -> Optional[Dict[str, object]]:
    """What the probe does for a config: None when only the rank block runs (model types other than linear / mlp), else
    {model, loss, metrics, L} (L needs the labels' width when task == -1).  CE (softmax cross-entropy over ONE column of class
    indices) is planned when the caller passes ``n_classes``, which becomes L; without it CE raises NotImplementedError, and with
    task == -1 ValueError.  NotImplementedError also for L1 / MSE with task == -1, whose metric (PCC) is 1-D."""
    mt = cfg["model_type"]
    if not (mt == "linear" or mt.lower() == "mlp"):
        return None
    loss = cfg["loss_type"]
    if loss == CE:
        if n_classes is None:
            raise NotImplementedError("loss_type CE: needs the class count (plan(cfg, n_classes=...))")
        if cfg["task"] == -1:
            raise ValueError("loss_type CE with task -1: CE reads one column of class indices")
        if not 2 <= int(n_classes) <= MAX_L:
            raise ValueError(f"loss_type CE: {n_classes} classes, the head kernel takes 2 .. {MAX_L}")
        return {"model": "linear" if mt == "linear" else "mlp", "loss": CE, "L": int(n_classes), "metrics": list(M.MULTICLASS_METRICS)}
    if loss not in LOSS_CODES:
        raise Exception("Didn't recognize config.metric")
    if loss in ("L1", "MSE") and cfg["task"] == -1:
        raise NotImplementedError(f"loss_type {loss} with task -1: its metric (PCC) is 1-D")
    L = n_labels_all if cfg["task"] == -1 else 1
    return {"model": "linear" if mt == "linear" else "mlp", "loss": loss, "L": L,
            "metrics": list(M.BINARY_METRICS) if loss == "BCE" else ["PCC"]}


def lr_schedule(name: str, lr: float, warmup: int, total: int) -> Callable[[int], float]:
    """transformers.get_scheduler(name, warmup, total) as a multiplier of the base LR (train_accel_gpu.lr_factor)"""
    import importlib
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    lr_factor = importlib.import_module("train_accel_gpu").lr_factor
    return lambda step: lr_factor(name, step, warmup, total)


__all__ = ["Probe", "ProbeParams", "EpochSampler", "build_module", "plan", "check_binary_targets", "check_class_targets", "lr_schedule"]
