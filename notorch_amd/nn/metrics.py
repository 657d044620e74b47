"""Metrics (reference ``notorch.nn.metrics``): same class names, constructor arguments and call signature
``metric(preds, targets, *, mask=None, sample_weights=None)``; no ``torchmetrics``.

``MAE``, ``RMSE`` and their Bounded forms are element losses reduced like the losses of
:mod:`notorch_amd.nn.loss.loss` and take the same two routes (``nt_task_loss`` or torch ops).  ``RMSE`` keeps
the reference's literal definition, the mean of ``sqrt((preds - targets)^2)``, which equals ``MAE``.

``AUROC`` and ``AUPRC`` rank by sort and scan.  With ``task="binary"`` every unmasked ``(b, t)`` entry is pooled
into one ranking; with ``task="multilabel"`` every column is ranked and the result is the mean over the
columns that have both classes (NaN when none has).  An entry is positive where ``int(target) == 1``,
negative where it is 0, ignored otherwise or where ``mask`` is False; ``mask=None`` means all true.
AUROC is the trapezoid over distinct thresholds (Mann-Whitney, ties counted half), AUPRC the average
precision ``sum_g (tp_g - tp_{g-1}) / P * tp_g / (tp_g + fp_g)`` over the groups ``g`` of equal scores.

* **kernel**: fp32 / bf16 / fp16 scores on a ROCm device.  Up to ``kernels.rank_metric_max_n()`` (4096) ranked
  rows: ``nt_rank_metric``, one workgroup per column.  Above that, up to ``RANK_LONG_DEFAULT_MAX_N`` rows
  (with ``NT_LOSS=kernel``: up to ``kernels.rank_metric_long_max_n()`` = 2^24): ``nt_rank_metric_long``, sorted
  runs of 4096 rows, merge passes and a tiled scan over several workgroups per column.  Metrics carry no
  gradient.
* **torch ops**: a sort, cumulative sums and the group ends (never ``O(n^2)``), on any device and dtype:
  CPU, fp64, more rows than the above, or ``NT_LOSS=torch`` in the environment (read per call).

``R2``, ``Accuracy`` and ``F1`` are torch ops on every device.
"""
from __future__ import annotations

import os
from typing import Literal

import torch
import torch.nn as nn
from torch import Tensor

from notorch_amd import kernels as K
from notorch_amd.nn.loss.loss import _as_bool, _BoundedMixin, _LossFunctionBase

__all__ = ["MAE", "RMSE", "BoundedMAE", "BoundedRMSE", "R2", "AUROC", "AUPRC", "Accuracy", "F1",
           "rank_metric_torch", "RANK_LONG_DEFAULT_MAX_N"]

# Rankings of more than kernels.rank_metric_max_n() and at most this many rows take nt_rank_metric_long without
# being asked to (NT_LOSS=kernel: up to kernels.rank_metric_long_max_n()).  The largest n timed such that the
# kernel is not slower than the torch route there and at every smaller n timed: DESIGN.md section 4.
RANK_LONG_DEFAULT_MAX_N = 1 << 20


class MAE(_LossFunctionBase):
    KIND = "mae"

    def _element(self, preds, targets):
        return (preds - targets).abs()


class RMSE(_LossFunctionBase):
    KIND = "rmse"

    def _element(self, preds, targets):
        return (preds - targets).square().sqrt()


class BoundedMAE(_BoundedMixin, MAE):
    pass


class BoundedRMSE(_BoundedMixin, RMSE):
    pass


class R2(_LossFunctionBase):
    """Mean over the columns of ``1 - rss / tss``; ``None`` weights and mask mean ones, and the weights scale
    rows.  Otherwise literal: the column means are ``(w * targets).mean(0)`` over all rows, masked or not."""

    def forward(self, preds, targets, *, mask=None, sample_weights=None):
        w = 1.0 if sample_weights is None else sample_weights.unsqueeze(1)
        m = 1.0 if mask is None else mask
        target_means = (w * targets).mean(0, keepdim=True)
        rss = torch.sum(w * (preds - targets).square() * m, dim=0)
        tss = torch.sum(w * (targets - target_means).square() * m, dim=0)

        return (1 - rss / tss).mean(0)


def rank_metric_torch(scores: Tensor, targets: Tensor, mask: Tensor | None = None) -> Tensor:
    """AUROC, AP, P and N of every column of ``n x t`` scores (a ``t x 4`` tensor in the dtype of ``scores``,
    fp32 for half-precision scores): the sort-and-scan formulation of ``nt_rank_metric`` in torch ops."""
    n, t = scores.shape
    dev = scores.device
    dt = scores.dtype if scores.dtype in (torch.float32, torch.float64) else torch.float32
    cls = targets.trunc()
    keep = torch.ones_like(cls, dtype=torch.bool) if mask is None else _as_bool(mask)
    pos, neg = keep & (cls == 1), keep & (cls == 0)
    if n == 0:
        zero = torch.zeros(t, dtype=dt, device=dev)
        return torch.stack([zero / 0, zero / 0, zero, zero], 1)
    # ignored entries go behind every score; in a group of -inf scores they count nothing
    s, order = scores.detach().masked_fill(~(pos | neg), float("-inf")).sort(0, descending=True)
    tp = pos.gather(0, order).long().cumsum(0)
    fp = neg.gather(0, order).long().cumsum(0)
    ends = torch.ones(n, t, dtype=torch.bool, device=dev)
    ends[:-1] = s[1:] != s[:-1]
    # the counts at the group end before each position: they never decrease, so the latest is the largest
    zeros = torch.zeros(1, t, dtype=torch.long, device=dev)
    tp_prev = torch.cat([zeros, torch.where(ends, tp, 0).cummax(0).values[:-1]])
    fp_prev = torch.cat([zeros, torch.where(ends, fp, 0).cummax(0).values[:-1]])
    P, N = tp[-1], fp[-1]
    area = torch.where(ends, (fp - fp_prev) * (tp + tp_prev), 0).sum(0)  # exact integers
    auroc = area.to(dt) / (2 * P * N).to(dt)
    prec = tp.to(dt) / (tp + fp).clamp_min(1).to(dt)
    ap = torch.where(ends, (tp - tp_prev).to(dt) * prec, 0).sum(0) / P.to(dt)
    nan = torch.full_like(auroc, float("nan"))
    both = (P > 0) & (N > 0)
    return torch.stack([torch.where(both, auroc, nan), torch.where(both, ap, nan), P.to(dt),
                        N.to(dt)], 1)


class _ClassificationMetricBase(nn.Module):
    def __init__(self, task: Literal["binary", "multilabel"]) -> None:
        super().__init__()

        self.task = task

    def extra_repr(self) -> str:
        return f"task={self.task}"


class _RankMetric(_ClassificationMetricBase):
    COLUMN = 0  # of rank_metric's (AUROC, AP, P, N)

    def forward(self, preds: Tensor, targets: Tensor, *, mask: Tensor | None = None,
                sample_weights: Tensor | None = None) -> Tensor:
        if preds.shape != targets.shape:
            raise ValueError(f"preds and targets must have one shape, got {tuple(preds.shape)} and "
                             f"{tuple(targets.shape)}")
        if self.task == "binary":  # one ranking of every entry
            preds, targets = preds.reshape(-1, 1), targets.reshape(-1, 1)
            mask = None if mask is None else mask.reshape(-1, 1)
        elif preds.dim() != 2:
            raise ValueError(f"task={self.task} ranks the columns of b x t scores, got {tuple(preds.shape)}")
        if self._kernel_route(preds, targets, mask):
            mk = None if mask is None else _as_bool(mask).contiguous()
            kernel = K.rank_metric if preds.shape[0] <= K.rank_metric_max_n() else K.rank_metric_long
            res = kernel(preds.detach().float().contiguous(), targets.detach().float().contiguous(), mk)
        else:
            res = rank_metric_torch(preds, targets, mask)
        vals = res[:, self.COLUMN]
        both = (res[:, 2] > 0) & (res[:, 3] > 0)
        # the mean over the columns with both classes; 0 / 0 = NaN when there is none
        return torch.where(both, vals, torch.zeros_like(vals)).sum() / both.sum()

    @staticmethod
    def _kernel_route(preds: Tensor, targets: Tensor, mask: Tensor | None) -> bool:
        if not preds.is_cuda or preds.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            return False
        if any(x is not None and x.device != preds.device for x in (targets, mask)):
            return False
        knob = os.environ.get("NT_LOSS", "")
        if knob == "torch":
            return False
        n = preds.shape[0]
        if n <= K.rank_metric_max_n():
            return True
        return n <= (K.rank_metric_long_max_n() if knob == "kernel" else RANK_LONG_DEFAULT_MAX_N)


class AUROC(_RankMetric):
    COLUMN = 0


class AUPRC(_RankMetric):
    COLUMN = 1


class Accuracy(_LossFunctionBase):
    def __init__(self, task: Literal["binary", "multilabel"], threshold: float = 0.5):
        super().__init__()

        self.task = task
        self.threshold = threshold

    def _element(self, preds, targets):
        hard = preds > self.threshold if self.task == "binary" else preds.argmax(-1)
        return (hard == targets).to(preds.dtype)

    def extra_repr(self) -> str:
        return f"task={self.task}, threshold={self.threshold:0.1f}"


class F1(nn.Module):
    """F1 of the thresholded predictions from the masked TP, FP and FN counts: of all entries with
    ``task="binary"``, else per column and averaged over the columns.  No positives anywhere
    (``2 TP + FP + FN == 0``) gives 0."""

    def __init__(self, task: Literal["binary", "multilabel"], threshold: float = 0.5):
        super().__init__()

        self.task = task
        self.threshold = threshold

    def forward(self, preds: Tensor, targets: Tensor, *, mask: Tensor | None = None,
                sample_weights: Tensor | None = None) -> Tensor:
        keep = torch.ones_like(targets, dtype=torch.bool) if mask is None else _as_bool(mask)
        hard, truth = preds > self.threshold, targets.trunc() == 1
        dims = None if self.task == "binary" else 0
        dt = preds.dtype if preds.is_floating_point() else torch.get_default_dtype()
        tp = (keep & hard & truth).sum(dims).to(dt)
        fp = (keep & hard & ~truth).sum(dims).to(dt)
        fn = (keep & ~hard & truth).sum(dims).to(dt)
        den = 2 * tp + fp + fn
        f1 = torch.where(den > 0, 2 * tp / den.clamp_min(1), torch.zeros_like(den))

        return f1 if self.task == "binary" else f1.mean()

    def extra_repr(self) -> str:
        return f"task={self.task}, threshold={self.threshold:0.1f}"
