"""Embedding-space metrics of the reference's eval loop (utils/metrics.py:20-70, Wang & Isola 2020): alignment of
positive pairs and uniformity on the hypersphere, accumulated over batches like the reference's torchmetrics classes
(``update`` / ``compute(norm=...)`` / ``reset``).  Plain torch; evaluation only, not on the timed step.

The probe stage (lp_accel_gpu.py) adds: the retrieval rank metrics of the reference (utils/metrics.py:72-98:
``compute_cosines``, ``get_rank``, ``get_rank_metrics``) on the HIP rank kernel, ``uniformity`` (``lunif`` on the HIP pair
kernel), ``__call__`` on the two accumulators (torchmetrics' forward), and the per-epoch formulas of the probe's torchmetrics
(binary classification scores, Pearson correlation) as device tensor code without host syncs."""
from __future__ import annotations

from typing import Dict, List

import torch
from torch.nn.functional import normalize


def lalign(x: torch.Tensor, y: torch.Tensor, alpha: float = 2, norm: bool = True) -> torch.Tensor:
    if norm:
        x, y = normalize(x), normalize(y)
    return (x - y).norm(dim=1).pow(alpha).mean()


def lunif(x: torch.Tensor, t: float = 2, norm: bool = True) -> torch.Tensor:
    if norm:
        x = normalize(x)
    return torch.pdist(x, p=2).pow(2).mul(-t).exp().mean().log()


def _gather_cat(parts: List[torch.Tensor], group=None) -> torch.Tensor:
    """this rank's accumulated rows, then every other rank's, rank-major: what torchmetrics does for a list state with
    ``dist_reduce_fx="cat"`` when ``compute()`` synchronises (utils/metrics.py:40-41,60)"""
    import torch.distributed as dist
    local = torch.cat(parts) if parts else torch.zeros(0)
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return local
    out = [None] * dist.get_world_size(group)
    dist.all_gather_object(out, local, group=group)
    return torch.cat([o for o in out if o.numel()])


class Alignment:
    def __init__(self, alpha: float = 2):
        self.alpha = alpha
        self.preds: List[torch.Tensor] = []
        self.target: List[torch.Tensor] = []

    def update(self, preds: torch.Tensor, target: torch.Tensor):
        if preds.shape != target.shape:
            raise ValueError("preds and target must have the same shape")
        self.preds.append(preds.detach().float().cpu())
        self.target.append(target.detach().float().cpu())

    def compute(self, norm: bool = False, sync: bool = False, group=None) -> torch.Tensor:
        """sync: gather every rank's rows first (a collective: every rank must call it), as the reference's torchmetrics do"""
        if sync:
            return lalign(_gather_cat(self.preds, group), _gather_cat(self.target, group), self.alpha, norm)
        return lalign(torch.cat(self.preds), torch.cat(self.target), self.alpha, norm)

    def __call__(self, preds: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """torchmetrics' forward: the rows are accumulated, and the value of THIS call's rows is returned (norm=False)."""
        self.update(preds, target)
        return lalign(preds.float(), target.float(), self.alpha, False)

    def reset(self):
        self.preds, self.target = [], []


class Uniformity:
    def __init__(self, t: float = 2):
        self.t = t
        self.preds: List[torch.Tensor] = []

    def update(self, preds: torch.Tensor):
        self.preds.append(preds.detach().float().cpu())

    def compute(self, norm: bool = False, sync: bool = False, group=None) -> torch.Tensor:
        if sync:
            return lunif(_gather_cat(self.preds, group), self.t, norm)
        return lunif(torch.cat(self.preds), self.t, norm)

    def __call__(self, preds: torch.Tensor) -> torch.Tensor:
        """torchmetrics' forward: the rows are accumulated, and the value of THIS call's rows is returned (norm=False), on the
        HIP pair kernel (``uniformity``)."""
        self.update(preds)
        return uniformity(preds, self.t, False)

    def reset(self):
        self.preds = []


# ---- HIP-backed retrieval and uniformity (csrc/evaluate.hip) --------------------------------------------------------------
def _hip():
    import importlib
    return importlib.import_module("mca-paper_amd.hip")


def _hip_device(device=None) -> torch.device:
    """The HIP device the kernels below run on: the current one (``device``, when given, must name it).  The library reads
    device memory only, so a request it cannot serve raises ValueError here, before anything is launched."""
    if device is not None:
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"the evaluation kernels run on a HIP device, not on {dev}")
    if not torch.cuda.is_available():
        raise ValueError("the evaluation kernels need a HIP device and none is available (the inputs stay on the cpu)")
    cur = torch.device("cuda", torch.cuda.current_device())
    if device is not None and dev.index is not None and dev.index != cur.index:
        raise ValueError(f"device {dev} is not the current HIP device {cur}: the kernels launch on its current stream")
    return cur


def _device_f32(x: torch.Tensor, device: torch.device) -> torch.Tensor:
    """x as a contiguous fp32 (rows, features) tensor on ``device`` (a ``_hip_device``): cpu inputs are copied there."""
    if x.dim() != 2:
        raise ValueError(f"expected a 2-D (rows, features) tensor, got {tuple(x.shape)}")
    return x.detach().to(device=device, dtype=torch.float32).contiguous()


def normalize_rows(x: torch.Tensor) -> torch.Tensor:
    """x / max(||x||_2, 1e-8) per row, fp32 on the current HIP device (cpu inputs are copied there): the first half of
    torch's cosine_similarity."""
    h = _hip()
    x = _device_f32(x, _hip_device())
    y = torch.empty_like(x)
    h.call("mca_rows_normalize_f32", x.data_ptr(), x.shape[1], y.data_ptr(), x.shape[1], x.shape[0], x.shape[1], h.stream_ptr())
    return y


def uniformity(x: torch.Tensor, t: float = 2, norm: bool = True) -> torch.Tensor:
    """``lunif`` of the same rows on the HIP pair kernel: log of the mean over pairs i < j of exp(-t ||x_i - x_j||^2), the
    squared distance taken as a direct-difference fmaf chain (no pdist sqrt then square), exp in fp32, the sum in fp64.
    A 0-d fp32 tensor on the current HIP device (cpu inputs are copied there): NaN for fewer than two rows, -inf when every
    pair underflows (as the pdist form)."""
    h = _hip()
    x = _device_f32(x, _hip_device())
    if norm:
        x = normalize_rows(x)
    n, d = x.shape
    ws = torch.empty(h.lib().mca_pair_gauss_workspace(n), dtype=torch.float64, device=x.device)
    out = torch.empty((), dtype=torch.float32, device=x.device)
    h.call("mca_pair_gauss_sum_f32", x.data_ptr(), d, n, max(d, 1), float(t), ws.data_ptr(), ws.numel(), None, out.data_ptr(),
           h.stream_ptr())
    return out


def cosine_ranks(queries: torch.Tensor, targets: torch.Tensor, index: torch.Tensor, device=None) -> torch.Tensor:
    """ranks[r] = #{j : cos(q_i, t_j) > cos(q_i, t_i)}, i = index[r]: the rank of the true target (row i of targets) among
    all targets, strict > as the reference's get_rank.  int32 on the HIP device (``_hip_device(device)``; cpu inputs are
    copied there); cosines as torch's cosine_similarity takes them (rows normalised, then one fmaf chain per dot product;
    the true target's value is bitwise the matrix's)."""
    h = _hip()
    dev = _hip_device(device)
    q, t = normalize_rows(_device_f32(queries, dev)), normalize_rows(_device_f32(targets, dev))
    if q.shape[1] != t.shape[1]:
        raise ValueError(f"queries have {q.shape[1]} features, targets {t.shape[1]}")
    idx = index.detach().to(device="cpu", dtype=torch.int64)
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= min(q.shape[0], t.shape[0])):
        raise IndexError("every selected query needs its true target: row i of queries pairs with row i of targets")
    idx = idx.to(device=dev, dtype=torch.int32)
    s_true = torch.empty(idx.numel(), dtype=torch.float32, device=dev)
    ranks = torch.empty(idx.numel(), dtype=torch.int32, device=dev)
    h.call("mca_cosine_rank_f32", q.data_ptr(), q.shape[1], idx.data_ptr(), idx.numel(), t.data_ptr(), t.shape[1], t.shape[0], t.shape[1],
           s_true.data_ptr(), ranks.data_ptr(), h.stream_ptr())
    return ranks


TOPK_MAX = 64          # include/mca_hip.h MCA_TOPK_MAX


def _topk_arguments(queries, targets, k, query_index, target_mask, exclude):
    """cosine_topk's argument checks, on shapes and host values only (they raise with or without a HIP device): the selected
    query rows as a cpu int64 tensor or None, the target mask as cpu bool or None, the exclusions as cpu int64 or None."""
    if queries.dim() != 2 or targets.dim() != 2:
        raise ValueError(f"expected 2-D (rows, features) tensors, got {tuple(queries.shape)} and {tuple(targets.shape)}")
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= TOPK_MAX:
        raise ValueError(f"k must be an integer in 1..{TOPK_MAX}, got {k!r}")
    if queries.shape[1] != targets.shape[1]:
        raise ValueError(f"queries have {queries.shape[1]} features, targets {targets.shape[1]}")
    if queries.shape[1] < 1:
        raise ValueError("the rows have no features")
    idx = None
    if query_index is not None:
        idx = torch.as_tensor(query_index).detach().reshape(-1).to(device="cpu", dtype=torch.int64)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= queries.shape[0]):
            raise IndexError(f"query_index selects a row outside the {queries.shape[0]} query rows")
    n = queries.shape[0] if idx is None else idx.numel()
    mask = None
    if target_mask is not None:
        mask = torch.as_tensor(target_mask).detach().reshape(-1).to("cpu")
        if mask.numel() != targets.shape[0]:
            raise ValueError(f"target_mask has {mask.numel()} entries for {targets.shape[0]} targets")
        mask = mask != 0
    ex = None
    if exclude is not None:
        ex = torch.as_tensor(exclude).detach().reshape(-1).to(device="cpu", dtype=torch.int64)
        if ex.numel() != n:
            raise ValueError(f"exclude has {ex.numel()} entries for {n} queries")
        ex = ex.clamp(min=-1, max=2 ** 31 - 1)          # anything below 0 or past the last target excludes nothing
    return idx, mask, ex


def cosine_topk(queries: torch.Tensor, targets: torch.Tensor, k: int, query_index=None, target_mask=None, exclude=None, device=None):
    """The k nearest targets of every query by cosine, on the HIP top-k kernel: (scores (n, k) float32, indices (n, k) int64)
    on the HIP device (``_hip_device(device)``; cpu inputs are copied there), n = the rows ``query_index`` selects (all when
    None).  Rows are normalised as in ``cosine_ranks`` and a score is the same fmaf chain, so it is bitwise the value the rank
    kernel compares.  ``target_mask`` (true = the target may be returned) and ``exclude`` (per query one target index that may
    not, -1 for none) narrow the candidates; a NaN score is never returned.  Order: the higher score first, equal scores by
    the lower index.  Columns past the number of candidates hold index -1 and score -inf.  The (n, targets) matrix is never
    formed.  ValueError for k outside 1..64, a feature mismatch, a mask or exclusion of the wrong length, or no usable HIP
    device; IndexError for a query_index outside the query rows: all before anything is launched."""
    idx, mask, ex = _topk_arguments(queries, targets, k, query_index, target_mask, exclude)
    k = int(k)
    h = _hip()
    dev = _hip_device(device)
    q, t = normalize_rows(_device_f32(queries, dev)), normalize_rows(_device_f32(targets, dev))
    n = q.shape[0] if idx is None else idx.numel()
    idx = None if idx is None else idx.to(device=dev, dtype=torch.int32)
    mask = None if mask is None else mask.to(device=dev, dtype=torch.uint8)
    ex = None if ex is None else ex.to(device=dev, dtype=torch.int32)
    need = h.lib().mca_cosine_topk_workspace(n, t.shape[0], k)
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
    score = torch.empty(n, k, dtype=torch.float32, device=dev)
    index = torch.empty(n, k, dtype=torch.int32, device=dev)
    h.call("mca_cosine_topk_f32", q.data_ptr(), q.shape[1], h.ptr(idx), n, t.data_ptr(), t.shape[1], t.shape[0], t.shape[1], h.ptr(mask),
           h.ptr(ex), k, ws.data_ptr(), ws.numel(), score.data_ptr(), k, index.data_ptr(), k, h.stream_ptr())
    return score, index.long()


def knn_predict(scores: torch.Tensor, indices: torch.Tensor, labels: torch.Tensor, weighted: bool = False) -> torch.Tensor:
    """The kNN readout of ``cosine_topk``'s result: per query the mean of ``labels[indices]`` over the valid neighbours
    (index >= 0), weighted by ``scores.clamp_min(0)`` when ``weighted``.  labels (n,) -> (queries,), labels (n, L) ->
    (queries, L), float32.  NaN where a row has no valid neighbour, and where ``weighted`` and all its weights are 0.
    Plain torch on the device of ``indices``."""
    valid = indices >= 0
    w = valid.to(torch.float32)
    if weighted:
        w = w * scores.to(torch.float32).clamp_min(0)          # padding: 0 * max(-inf, 0) = 0
    lab = labels.to(device=indices.device, dtype=torch.float32)
    flat = lab.reshape(lab.shape[0], -1)
    picked = flat[indices.clamp_min(0).long()]                             # (queries, k, L); padding picks row 0 ...
    picked = torch.where(valid[..., None], picked, torch.zeros_like(picked))          # ... and drops it
    total = w.sum(1, keepdim=True)
    out = (picked * w[..., None]).sum(1) / total
    out = torch.where(total > 0, out, torch.full_like(out, float("nan")))
    return out.reshape(-1) if lab.dim() == 1 else out


def hits_at(indices: torch.Tensor, positives: torch.Tensor, m: int) -> torch.Tensor:
    """hit[r] = ``positives[r]`` is among the first ``m`` returned indices of row r: presence in the top-m list.  With the
    reference's rank (the number of targets scoring STRICTLY higher than the true one) this equals ``rank < m`` except on exact
    score ties: a true target tied with m or more lower-indexed targets has rank < m but no place among the first m."""
    pos = torch.as_tensor(positives, device=indices.device).reshape(-1, 1).to(indices.dtype)
    return ((indices[:, :m] == pos) & (pos >= 0)).any(1)


def compute_cosines(embedding: torch.Tensor, embeddings: torch.Tensor) -> torch.Tensor:
    """utils/metrics.py:73-76: cosine of one vector against every row, (rows,) fp32 on the current HIP device, without the
    reference's (rows, D) repeat: normalised rows times the normalised vector on the HIP probe layer kernel."""
    h = _hip()
    dev = _hip_device()
    t = normalize_rows(_device_f32(embeddings, dev))
    q = normalize_rows(_device_f32(embedding.reshape(1, -1), dev))
    out = torch.empty(t.shape[0], 1, dtype=torch.float32, device=dev)
    h.call("mca_probe_nt_f32", t.data_ptr(), t.shape[1], None, q.data_ptr(), q.shape[1], None, out.data_ptr(), 1, t.shape[0], 1, t.shape[1],
           0, 0.0, 0, 0, h.stream_ptr())
    return out.reshape(-1)


def get_rank(x: torch.Tensor, indices) -> torch.Tensor:
    """utils/metrics.py:78-80: per row of a (queries, targets) similarity matrix, how many entries exceed the true one."""
    idx = torch.as_tensor(indices, device=x.device, dtype=torch.long)
    vals = x[torch.arange(len(x), device=x.device), idx]
    return (x > vals[:, None]).long().sum(1)


def get_rank_metrics(embeddings: torch.Tensor, mask: torch.Tensor, targets: torch.Tensor, fusion: str = "fusion", device="cuda"):
    """utils/metrics.py:82-98: (median rank, R@1, R@5, R@10) over the queries the mask selects, query i's positive being row
    i of ``targets``.  0-d tensors on the HIP device: the median is torch.median's (the lower middle value), the recalls
    fractions.  No selected query raises RuntimeError; a ``device`` that is not the current HIP device raises ValueError
    (cpu inputs are copied to it)."""
    _hip_device(device)                                 # a device the kernels cannot run on raises before any work
    sel = torch.nonzero(torch.as_tensor(mask).reshape(-1).to("cpu").bool()).reshape(-1)
    if sel.numel() == 0:
        raise RuntimeError("get_rank_metrics: the mask selects no query")
    ranks = cosine_ranks(embeddings, targets, sel, device).long()
    n = float(ranks.numel())
    return ranks.median(), (ranks == 0).sum() / n, (ranks < 5).sum() / n, (ranks < 10).sum() / n


# ---- the probe's torchmetrics, per epoch on device tensors ------------------------------------------------------------------
BINARY_METRICS = ("precision", "recall", "accuracy", "cm", "f1", "specificity", "auroc", "auprc")


def binary_format(preds: torch.Tensor, batch_rows: int, row_width: int) -> torch.Tensor:
    """torchmetrics' binary input rule, per update: a batch (``batch_rows`` rows of ``row_width`` predictions, the last batch
    possibly shorter) any of whose predictions lies outside [0, 1] is taken as logits and goes through a sigmoid."""
    p = preds.reshape(-1).float()
    per = batch_rows * row_width
    bid = torch.arange(p.numel(), device=p.device) // per
    nb = (p.numel() + per - 1) // per
    bad = torch.zeros(nb, device=p.device).scatter_reduce(0, bid, ((p < 0) | (p > 1)).float(), reduce="amax", include_self=True)
    return torch.where(bad[bid] > 0, torch.sigmoid(p), p)


def _safe_div(a, b):
    return torch.where(b > 0, a / b.clamp_min(1), torch.zeros_like(a))


def binary_metrics(probs: torch.Tensor, target: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The eight binary torchmetrics of the probe (lp_accel_gpu.py:105-115) from formatted predictions (``binary_format``)
    and 0/1 targets, flattened: threshold 0.5 (pred = p > 0.5), zero division -> 0, cm = [[TN, FP], [FN, TP]].  auroc and
    auprc are exact (no binning; sklearn's roc_auc_score / average_precision_score, ties as one threshold).  An epoch of a
    single class returns auroc 0 and, with no positive, auprc 0 (with only positives auprc is 1)."""
    p = probs.reshape(-1).double()
    y = target.reshape(-1).long()
    hard = (p > 0.5).long()
    tp = ((hard == 1) & (y == 1)).sum().double()
    fp = ((hard == 1) & (y == 0)).sum().double()
    fn = ((hard == 0) & (y == 1)).sum().double()
    tn = ((hard == 0) & (y == 0)).sum().double()
    out = {"precision": _safe_div(tp, tp + fp), "recall": _safe_div(tp, tp + fn),
           "accuracy": _safe_div(tp + tn, tp + tn + fp + fn), "f1": _safe_div(2 * tp, 2 * tp + fp + fn),
           "specificity": _safe_div(tn, tn + fp),
           "cm": torch.stack([torch.stack([tn, fp]), torch.stack([fn, tp])]).long()}
    out["auroc"], out["auprc"], _, _ = _exact_curves(p, y)
    return {k: (v if k == "cm" else v.float()) for k, v in out.items()}


def _exact_curves(p: torch.Tensor, y: torch.Tensor):
    """(auroc, auprc, positives, negatives) of fp64 scores p and 0/1 targets y, both 1-d: the exact curves, scores in descending
    order, one point per distinct score (the last index of each run of ties); a zero division gives 0"""
    order = torch.argsort(p, descending=True, stable=True)
    ps, ys = p[order], y[order].double()
    n = ps.numel()
    pos = torch.arange(1, n + 1, device=p.device, dtype=torch.float64)
    tps = torch.cumsum(ys, 0)
    fps = pos - tps
    last = torch.ones(n, dtype=torch.bool, device=p.device)
    last[:-1] = ps[1:] != ps[:-1]
    first = torch.ones(n, dtype=torch.bool, device=p.device)
    first[1:] = ps[1:] != ps[:-1]
    start = torch.cummax(torch.where(first, torch.arange(n, device=p.device), torch.zeros(n, dtype=torch.long, device=p.device)), 0).values
    prev = start - 1                                            # the previous distinct score's last index (-1: the origin)
    tp_prev = torch.where(prev >= 0, tps[prev.clamp_min(0)], torch.zeros_like(tps))
    fp_prev = torch.where(prev >= 0, fps[prev.clamp_min(0)], torch.zeros_like(fps))
    P, N = tps[-1], fps[-1]
    lastf = last.double()
    area = ((fps - fp_prev) * (tps + tp_prev) * 0.5 * lastf).sum()
    return _safe_div(area, P * N), _safe_div(((tps - tp_prev) * (tps / pos) * lastf).sum(), P), P, N


MULTICLASS_METRICS = BINARY_METRICS


def multiclass_metrics(probs: torch.Tensor, target: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The eight ``task='multiclass'`` metrics the reference's CE branch names (lp_accel_gpu.py), from class probabilities
    (n, C) and class-index targets (n,), as device tensor code.  The prediction is the argmax, a tie going to the LOWEST class
    index; cm[true, pred] is (C, C) int64; accuracy is micro (trace / n); precision, recall, f1 and specificity are macro means
    over the classes with tp + fp + fn > 0 (a zero division gives 0); auroc is the macro mean of the exact one-vs-rest AUROC
    (``binary_metrics``' curve code) over the classes with at least one positive and one negative, 0 when there is none; auprc
    the macro mean of the exact average precision over the classes with at least one positive.

    These are torchmetrics' multiclass defaults as far as can be told without it: torchmetrics is not installed where this
    was written, and the reference's CE branch cannot run (it takes the class count from the label width and hands
    torchmetrics a target of the predictions' shape), so no reference numbers exist to pin these against."""
    n, C = probs.shape
    p = probs.double()
    y = target.reshape(-1).long()
    top = p.max(1, keepdim=True).values
    classes = torch.arange(C, device=p.device)
    pred = torch.where(p == top, classes[None, :], torch.full((1, 1), C, device=p.device)).min(1).values          # the lowest index among ties
    pred = pred.clamp_max(C - 1)                                                                                  # (a row of NaN)
    cm = torch.zeros(C * C, dtype=torch.long, device=p.device).scatter_add_(0, y * C + pred, torch.ones(n, dtype=torch.long, device=p.device))
    cm = cm.view(C, C)
    cmd = cm.double()
    tp = cmd.diagonal()
    fp, fn = cmd.sum(0) - tp, cmd.sum(1) - tp
    tn = cmd.sum() - tp - fp - fn
    seen = ((tp + fp + fn) > 0).double()
    k = seen.sum()
    macro = lambda v: _safe_div((v * seen).sum(), k)
    out = {"precision": macro(_safe_div(tp, tp + fp)), "recall": macro(_safe_div(tp, tp + fn)), "accuracy": _safe_div(tp.sum(), cmd.sum()),
           "cm": cm, "f1": macro(_safe_div(2 * tp, 2 * tp + fp + fn)), "specificity": macro(_safe_div(tn, tn + fp))}
    roc, ap, has_roc, has_ap = [], [], [], []
    for c in range(C):
        a, r, P, N = _exact_curves(p[:, c].contiguous(), (y == c).long())
        roc.append(a); ap.append(r); has_roc.append(((P > 0) & (N > 0)).double()); has_ap.append((P > 0).double())
    roc, ap, has_roc, has_ap = torch.stack(roc), torch.stack(ap), torch.stack(has_roc), torch.stack(has_ap)
    out["auroc"] = _safe_div((roc * has_roc).sum(), has_roc.sum())
    out["auprc"] = _safe_div((ap * has_ap).sum(), has_ap.sum())
    return {k: (v if k == "cm" else v.float()) for k, v in out.items()}


def pearson(preds: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Pearson correlation of the flattened predictions and targets over the epoch (fp64 moments, an fp32 0-d result)."""
    x, y = preds.reshape(-1).double(), target.reshape(-1).double()
    xc, yc = x - x.mean(), y - y.mean()
    return ((xc * yc).sum() / ((xc * xc).sum().sqrt() * (yc * yc).sum().sqrt())).float()
