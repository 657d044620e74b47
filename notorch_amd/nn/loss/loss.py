"""Task losses (reference ``notorch.nn.loss.loss``): same class names, constructor arguments and aliases.

Every loss is an element loss ``L[i, j]`` of ``preds[i, j]`` (``b x t``, or ``b x t x c`` for MVE, Evidential,
CrossEntropy and Dirichlet) and ``targets[i, j]``, reduced as the reference evidently means to:

    loss = sum_ij L[i, j] w[i] m[i, j] / sum_ij m[i, j]        (mask m; without one: the mean over b t)

``sample_weights`` (``b``) scale rows for every ``t`` (the reference multiplies by ``unsqueeze(0)``, which
raises unless ``t`` is ``b`` or 1 and yields a ``b x b`` matrix at ``t == 1``).  An all-false mask gives NaN,
as ``0 / 0`` does there.  The Bounded losses run (the reference passes keyword-only arguments positionally
and raises ``TypeError``); an element clamped to its target has zero loss and zero gradient.

Two routes, chosen from devices, dtypes and ``requires_grad`` alone (nothing is read back from the device):

* **kernel**: ``preds`` in fp32 or bf16 on a ROCm device, every other tensor on that device, no gradient
  wanted for ``targets`` or ``sample_weights``: ``nt_task_loss`` through :class:`TaskLossFunction`, one
  launch that returns the fp32 loss and, when ``preds`` needs a gradient, ``dLoss/dpreds`` in its dtype.
* **torch ops**: the same math on any device and dtype (CPU, fp64, fp16), differentiated by autograd.

``NT_LOSS`` in the environment, read per call, overrides the choice on device tensors: ``torch`` forces
torch ops, ``kernel`` forces the kernel.  Without it a kind takes the kernel unless it is listed in
``TORCH_BY_DEFAULT`` (the kinds whose training step measured slower on the kernel: DESIGN.md section 4).
``Dirichlet`` is torch ops only (its gradient needs a trigamma).
"""
from __future__ import annotations

import math
import os
from abc import abstractmethod

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from notorch_amd import kernels as K

__all__ = [
    "SelfSupervisedLoss",
    "MSE",
    "BoundedMSE",
    "MeanVarianceEstimation",
    "MVE",
    "Evidential",
    "BinaryCrossEntropy",
    "BCE",
    "CrossEntropy",
    "XENT",
    "Dirichlet",
    "TaskLossFunction",
]

# kinds that take torch ops on device tensors unless NT_LOSS=kernel (see the module docstring)
TORCH_BY_DEFAULT: frozenset[str] = frozenset()


class SelfSupervisedLoss(nn.Module):
    """A pass-through module to backpropagate self-supervised loss terms: an ``nn.Identity`` that checks
    that its input is a scalar and has an idiomatic name in config files."""

    def forward(self, inputs: Tensor) -> Tensor:
        if inputs.ndim != 0:
            raise ValueError(f"input must be a scalar! received input with shape: {inputs.shape}")

        return inputs


class TaskLossFunction(torch.autograd.Function):
    """The reduced loss on the kernel: one launch returns the loss and, with ``need_grad``, ``dLoss/dpreds``
    for a unit upstream gradient; backward is one multiply.  Only ``preds`` gets a gradient."""

    @staticmethod
    def forward(ctx, preds, targets, mask, sample_weights, lt_mask, gt_mask, kind, v_kl, eps, need_grad):
        # need_grad is the caller's torch.is_grad_enabled() and preds.requires_grad: needs_input_grad does
        # not see no_grad, and without a gradient no buffer is allocated
        loss, dpreds = K.task_loss(preds, targets, kind, mask, sample_weights, lt_mask, gt_mask, v_kl, eps,
                                   need_grad)
        ctx.save_for_backward(dpreds)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        (dpreds,) = ctx.saved_tensors
        return (dpreds * grad_out.to(dpreds.dtype),) + (None,) * 9


def _as_bool(m: Tensor | None) -> Tensor | None:
    if m is None or m.dtype == torch.bool:
        return m
    return m != 0


class _LossFunctionBase(nn.Module):
    KIND: str | None = None  # the kernel's element loss; None: torch ops only

    def forward(self, preds: Tensor, targets: Tensor, *, mask: Tensor | None = None,
                sample_weights: Tensor | None = None) -> Tensor:
        return self._forward(preds, targets, mask, sample_weights)

    @abstractmethod
    def _element(self, preds: Tensor, targets: Tensor) -> Tensor:
        """The ``b x t`` element loss in torch ops."""

    def _kernel_params(self) -> tuple[float, float]:
        return 0.0, 0.0

    def _forward(self, preds, targets, mask, sample_weights, lt_mask=None, gt_mask=None) -> Tensor:
        if self._kernel_route(preds, targets, mask, sample_weights, lt_mask, gt_mask):
            v_kl, eps = self._kernel_params()
            sw = None if sample_weights is None else sample_weights.detach().float().contiguous()
            mk, lt, gt = (None if m is None else _as_bool(m).contiguous() for m in (mask, lt_mask, gt_mask))
            return TaskLossFunction.apply(preds.contiguous(), targets.detach().float().contiguous(), mk, sw, lt, gt,
                                          self.KIND, v_kl, eps, torch.is_grad_enabled() and preds.requires_grad)
        if lt_mask is not None:
            preds = torch.where((preds < targets) & _as_bool(lt_mask), targets, preds)
        if gt_mask is not None:
            preds = torch.where((preds > targets) & _as_bool(gt_mask), targets, preds)
        return self._reduce(self._element(preds, targets), mask, sample_weights)

    def _kernel_route(self, preds, targets, mask=None, sample_weights=None, lt_mask=None, gt_mask=None) -> bool:
        if self.KIND is None or not preds.is_cuda or preds.dtype not in (torch.float32, torch.bfloat16):
            return False
        others = (targets, mask, sample_weights, lt_mask, gt_mask)
        if any(x is not None and x.device != preds.device for x in others):
            return False
        if targets.dim() != 2 or preds.dim() not in (2, 3) or preds.shape[:2] != targets.shape:
            return False  # torch ops raise their own error
        sw = sample_weights
        if targets.requires_grad or (sw is not None and sw.requires_grad):
            return False
        knob = os.environ.get("NT_LOSS", "")
        if knob in ("torch", "kernel"):
            return knob == "kernel"
        return self.KIND not in TORCH_BY_DEFAULT

    def _reduce(self, loss: Tensor, mask: Tensor | None = None, sample_weights: Tensor | None = None) -> Tensor:
        if not loss.is_floating_point():
            loss = loss.to(torch.get_default_dtype())
        if sample_weights is not None:
            loss = loss * sample_weights.unsqueeze(1)

        return loss.mean() if mask is None else (loss * mask).sum() / mask.sum()


class _BoundedMixin:
    def forward(self, preds: Tensor, targets: Tensor, *, mask: Tensor | None = None,
                sample_weights: Tensor | None = None, lt_mask: Tensor, gt_mask: Tensor) -> Tensor:
        return self._forward(preds, targets, mask, sample_weights, lt_mask, gt_mask)


class MSE(_LossFunctionBase):
    KIND = "mse"

    def _element(self, preds, targets):
        return F.mse_loss(preds, targets, reduction="none")


class BoundedMSE(_BoundedMixin, MSE):
    pass


class MeanVarianceEstimation(_LossFunctionBase):
    """Eq. 9 of Nix and Weigend, "Estimating the mean and variance of the target probability distribution",
    ICNN 1994: ``preds[..., 0]`` is the mean, ``preds[..., 1]`` the variance."""

    KIND = "mve"

    def forward(self, preds, targets, *, mask=None, sample_weights=None, **kwargs):
        return self._forward(preds, targets, mask, sample_weights)

    def _element(self, preds, targets):
        m, v = preds.unbind(-1)
        return (m - targets).square() / (2 * v) + torch.log(2 * math.pi * v) / 2


class Evidential(_LossFunctionBase):
    """The evidential regression loss of Soleimany et al., ACS Cent. Sci. 2021, 7, 1356:
    ``preds[..., :]`` is ``(mean, v, alpha, beta)``."""

    KIND = "evidential"

    def __init__(self, v_kl: float = 0.2, eps: float = 1e-8):
        super().__init__()

        self.v_kl = v_kl
        self.eps = eps

    def _kernel_params(self):
        return float(self.v_kl), float(self.eps)

    def _element(self, preds, targets):
        m, v, a, be = preds.unbind(-1)
        r = targets - m
        B = 2 * be * (1 + v)  # 2 beta (1 + v)
        nll = (0.5 * torch.log(math.pi / v) - a * B.log() + (a + 0.5) * (v * r.square() + B).log()
               + torch.lgamma(a) - torch.lgamma(a + 0.5))
        reg = (2 * v + a) * r.abs()
        return nll + self.v_kl * (reg - self.eps)

    def extra_repr(self) -> str:
        return f"v_kl={self.v_kl:0.1f}, eps={self.eps:0.1e}"


class BinaryCrossEntropy(_LossFunctionBase):
    KIND = "bce"

    def _element(self, preds, targets):
        return F.binary_cross_entropy_with_logits(preds, targets, reduction="none")


class CrossEntropy(_LossFunctionBase):
    KIND = "xent"

    def _element(self, preds, targets):
        return F.cross_entropy(preds.transpose(1, 2), targets.long(), reduction="none")


class Dirichlet(_LossFunctionBase):
    """The loss of Sensoy et al., "Evidential deep learning to quantify classification uncertainty", NeurIPS
    2018, for ``alphas.shape[-1]`` classes (the reference hard-codes two).  Torch ops on every device."""

    def __init__(self, v_kl: float = 0.2) -> None:
        super().__init__()

        self.v_kl = v_kl

    def forward(self, alphas, targets, *, mask=None, sample_weights=None, **kwargs):
        return self._forward(alphas, targets, mask, sample_weights)

    def _element(self, alphas, targets):
        al = F.softplus(alphas) + 1
        k = al.shape[-1]
        y = F.one_hot(targets.long(), num_classes=k).to(al.dtype)
        S = al.sum(-1, keepdim=True)
        p = al / S
        mse = (y - p).square().sum(-1) + (p * (1 - p) / (S + 1)).sum(-1)
        # KL(Dir(at) || Dir(1)) with the evidence of the true class removed: at = y + (1 - y) al
        at = y + (1 - y) * al
        St = at.sum(-1)
        kl = (St.lgamma() - at.lgamma().sum(-1) - math.lgamma(k)
              + ((at - 1) * (torch.digamma(at) - torch.digamma(St).unsqueeze(-1))).sum(-1))
        return mse + self.v_kl * kl

    def extra_repr(self) -> str:
        return f"v_kl={self.v_kl:0.1f}"


BCE = BinaryCrossEntropy
XENT = CrossEntropy
MVE = MeanVarianceEstimation
