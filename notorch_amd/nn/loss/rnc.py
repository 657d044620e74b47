"""Rank-N-Contrast loss (reference ``notorch.nn.loss.RankNContrastLoss``, notorch/nn/loss/rnc.py).

With ``D = distance(targets)``, ``Sim = similarity(inputs)`` (both ``N x N``) and ``s = exp(Sim / temp)``:

    denom_ij = EPS + sum_{k : D[i,k] >= D[i,j]} s[i,k]          (k over all of 0..N-1)
    loss     = mean_{i != j} ( log denom_ij - Sim_ij / temp )

The reference materialises the ``N x N x N`` mask of the comparison.  Here every row is sorted by its
label distances (descending): the ``>=`` set of ``j`` is then the prefix of the row that ends where j's
group of equal distances ends, so one prefix sum of ``s`` per row serves every ``j``: O(N^2) memory.

Three routes, chosen by ``rnc_route`` without a device-to-host copy (``N`` comes from the shape):

* fp32 (or bf16 / fp16, widened) ``Sim`` and ``D`` on a ROCm device with ``N <= kernels.rnc_max_n()``:
  the HIP kernel ``nt_rnc_rank``, one workgroup per row, which under grad also writes ``dLoss/dSim``;
* the same tensors with ``N`` above that and up to ``RNC_LONG_DEFAULT_MAX_N`` (set from
  ``tools/rnc_bench.py``; up to ``kernels.rnc_long_max_n()`` with ``NT_RNC=kernel``): ``nt_rnc_rank_long``,
  the same kernel with 8 or 16 sorted positions per thread;
* anything else (CPU tensors, fp64, larger ``N``, or ``NT_RNC=torch``): the same sorted formulation in
  torch ops, differentiated by autograd.

``NT_RNC`` is read from the environment per call.

``k = i`` is inside the sum exactly when ``D[i,j] <= D[i,i]`` (duplicated targets), as in the reference.
One deliberate difference: the loss is evaluated as ``log denom - Sim / temp``, which stays finite where
the reference's ``log(s / denom)`` returns ``inf`` because ``s`` underflowed.  Non-finite entries of
``D`` or ``Sim`` are not checked (a check would need a device-to-host copy).
"""
from __future__ import annotations

import os
from abc import abstractmethod

import torch
import torch.nn as nn
from torch import Tensor

from notorch_amd import kernels as K

__all__ = ["RankNContrastLoss", "CDist", "PNorm", "RnCRankFunction", "RnCRankLongFunction", "rnc_route",
           "RNC_LONG_DEFAULT_MAX_N"]

# Largest N that takes nt_rnc_rank_long without NT_RNC=kernel: the largest N timed by tools/rnc_bench.py at
# which, as at every smaller timed N, the kernel's median is below the torch route's by more than the torch
# route's spread over the rounds; 0 would mean no N.  Measured: the kernel is 5 to 11 times
# ahead at every timed N up to kernels.rnc_long_max_n().
RNC_LONG_DEFAULT_MAX_N = 16384


class CDist(nn.Module):
    """Pairwise map: rows of ``A`` (``n x d``) against rows of ``B`` (default ``A``) -> ``n x m``."""

    @abstractmethod
    def forward(self, A: Tensor, B: Tensor | None = None) -> Tensor:
        pass


# torch.cdist with p != 2 launches one 256-thread block per (row of A, row of B) pair, and a HIP launch
# holds fewer than 2^32 threads: 4096 x 4096 pairs are refused ("invalid configuration argument").
# Row blocks of A below that many pairs keep every launch legal; the values are the same.
_CDIST_PAIRS = 1 << 23


class PNorm(CDist):
    def __init__(self, p: float = 2.0, negate: bool = False) -> None:
        super().__init__()

        self.p = p
        self.negate = negate

    def forward(self, A: Tensor, B: Tensor | None = None) -> Tensor:
        B = A if B is None else B
        rows = max(1, _CDIST_PAIRS // max(1, B.shape[-2]))
        if self.p != 2 and A.is_cuda and A.dim() == 2 and A.shape[0] > rows:
            X = torch.cat([torch.cdist(a, B, p=self.p) for a in A.split(rows)])
        else:
            X = torch.cdist(A, B, p=self.p)

        return X.neg() if self.negate else X

    def extra_repr(self) -> str:
        return f"p={self.p:0.1f}, negate={self.negate}"


class RnCRankFunction(torch.autograd.Function):
    """mean_{i != j} (log denom_ij - Sim_ij / temp) on the kernel: one launch returns the row sums and,
    when ``Sim`` needs a gradient, ``dLoss/dSim``; ``D`` gets no gradient (it is only compared)."""

    @staticmethod
    def forward(ctx, sim: Tensor, dist: Tensor, temp: float, eps: float, need_grad: bool) -> Tensor:
        # need_grad is the caller's torch.is_grad_enabled() and sim.requires_grad: needs_input_grad does
        # not see no_grad, and without a gradient no n x n buffer is allocated
        n = sim.shape[0]
        row_nll, dsim = K.rnc_rank(sim, dist, temp, eps, need_grad)
        ctx.save_for_backward(dsim)
        return row_nll.sum() / (n * (n - 1))

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        (dsim,) = ctx.saved_tensors
        return grad_out * dsim, None, None, None, None


class RnCRankLongFunction(RnCRankFunction):
    """``RnCRankFunction`` on ``K.rnc_rank_long``: N above ``K.rnc_max_n()``, up to ``K.rnc_long_max_n()``."""

    @staticmethod
    def forward(ctx, sim: Tensor, dist: Tensor, temp: float, eps: float, need_grad: bool) -> Tensor:
        n = sim.shape[0]
        row_nll, dsim = K.rnc_rank_long(sim, dist, temp, eps, need_grad)
        ctx.save_for_backward(dsim)
        return row_nll.sum() / (n * (n - 1))


def rank_loss_torch(sim: Tensor, dist: Tensor, temp: float, eps: float) -> Tensor:
    """The sorted formulation in torch ops (any device and dtype; autograd differentiates it)."""
    n = sim.shape[0]
    logits = sim / temp
    d_sorted, order = torch.sort(dist.detach(), dim=1, descending=True, stable=True)
    csum = logits.exp().gather(1, order).cumsum(1)
    # the last position of each group of equal distances; other positions take the next one to their right
    pos = torch.arange(n, device=sim.device).expand(n, n)
    ends = torch.ones(n, n, dtype=torch.bool, device=sim.device)
    ends[:, :-1] = d_sorted[:, 1:] != d_sorted[:, :-1]
    group_end = torch.where(ends, pos, n - 1).flip(1).cummin(1).values.flip(1)
    denom = torch.empty_like(csum).scatter(1, order, csum.gather(1, group_end) + eps)
    nll = denom.log() - logits
    diag = torch.eye(n, dtype=torch.bool, device=sim.device)
    return nll.masked_fill(diag, 0.0).sum() / (n * (n - 1))


_NARROW = (torch.float32, torch.bfloat16, torch.float16)


def rnc_route(n: int, device_type: str, sim_dtype: torch.dtype, dist_dtype: torch.dtype, knob: str) -> str:
    """Which route an N x N problem takes: ``"kernel"`` (``nt_rnc_rank``), ``"long"`` (``nt_rnc_rank_long``)
    or ``"torch"``.  ``knob`` is the value of ``NT_RNC``: ``"torch"`` forces torch, ``"kernel"`` takes the
    kernels as far as they reach instead of as far as they were measured to win."""
    if device_type != "cuda" or sim_dtype not in _NARROW or dist_dtype not in _NARROW or knob == "torch":
        return "torch"
    if n <= K.rnc_max_n():
        return "kernel"
    if n <= (K.rnc_long_max_n() if knob == "kernel" else RNC_LONG_DEFAULT_MAX_N):
        return "long"
    return "torch"


class RankNContrastLoss(nn.Module):
    EPS: float = 1e-6

    def __init__(self, distance: CDist | None = None, similarity: CDist | None = None, temp: float = 2.0):
        super().__init__()

        self.distance = distance or PNorm(p=1)
        self.similarity = similarity or PNorm(p=2, negate=True)
        self.temp = temp

    def forward(self, inputs: Tensor, targets: Tensor) -> Tensor:
        N = len(targets)
        dists = self.distance(targets)
        sims = self.similarity(inputs)
        if N < 2:  # the mean over no pairs
            return torch.full((), float("nan"), dtype=sims.dtype, device=sims.device)
        device = "cuda" if sims.is_cuda and dists.is_cuda else "cpu"
        route = rnc_route(N, device, sims.dtype, dists.dtype, os.environ.get("NT_RNC", ""))
        if route == "torch":
            return rank_loss_torch(sims, dists, self.temp, self.EPS)
        function = RnCRankLongFunction if route == "long" else RnCRankFunction
        sims = sims.float().contiguous()
        return function.apply(sims, dists.detach().float().contiguous(), float(self.temp), self.EPS,
                              torch.is_grad_enabled() and sims.requires_grad)

    def extra_repr(self) -> str:
        return f"(temp): {self.temp:0.1f}"
