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

``PNorm`` (the default distance, p = 1, and similarity, p = 2 negated) is ``torch.cdist``, or for 2-D fp32 /
bf16 ROCm tensors the direct-form HIP kernels ``nt_pairwise_pnorm`` / ``nt_pairwise_pnorm_backward``
(``PairwisePNormFunction``): for the p in ``PNORM_KERNEL_P``, or for p = 1 and 2 with ``NT_PNORM=kernel``;
``NT_PNORM=torch`` never takes them (``pnorm_route``; read per call).

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
           "RNC_LONG_DEFAULT_MAX_N", "PairwisePNormFunction", "pnorm_route", "PNORM_KERNEL_P"]

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


# The p that take the pairwise kernels (csrc/pairwise.hip) without NT_PNORM=kernel: a p is listed only if, at
# every shape tools/pnorm_bench.py times for it, the kernel's median is below the torch.cdist route's by more
# than that route's spread, forward and forward + backward (DESIGN.md §4 has the table).
PNORM_KERNEL_P: tuple = ()


class PairwisePNormFunction(torch.autograd.Function):
    """``K.pairwise_pnorm`` with ``K.pairwise_pnorm_backward`` as its gradient.  ``B = None`` is ``B = A`` (one
    backward pass gives A both of its uses).  X is fp32; each gradient comes back in its input's dtype."""

    @staticmethod
    def forward(ctx, A: Tensor, B: Tensor | None, p: int, negate: bool) -> Tensor:
        X = K.pairwise_pnorm(A, B, p=p, negate=negate)
        ctx.p, ctx.negate = p, negate
        ctx.save_for_backward(A, B, X)  # kept only when a gradient is recorded
        return X

    @staticmethod
    def backward(ctx, G: Tensor):
        A, B, X = ctx.saved_tensors
        want = tuple(name for name, t, need in (("A", A, ctx.needs_input_grad[0]), ("B", B, ctx.needs_input_grad[1]))
                     if t is not None and need)
        dA, dB = K.pairwise_pnorm_backward(A, B, X, G.float().contiguous(), p=ctx.p, negate=ctx.negate, want=want)
        return (None if dA is None else dA.to(A.dtype)), (None if dB is None else dB.to(B.dtype)), None, None


def pnorm_route(p: float, device_type: str, dtype_a: torch.dtype, dtype_b: torch.dtype, dims_ok: bool,
                knob: str) -> str:
    """Which route a PNorm call takes: ``"kernel"`` (``PairwisePNormFunction``) or ``"torch"`` (``torch.cdist``).
    ``dims_ok``: both operands 2-D with the same number of columns.  ``knob`` is the value of ``NT_PNORM``:
    ``"torch"`` never takes the kernel, ``"kernel"`` takes it for p = 1 and p = 2 whatever ``PNORM_KERNEL_P``
    lists."""
    if device_type != "cuda" or not dims_ok or dtype_a != dtype_b or dtype_a not in (torch.float32, torch.bfloat16):
        return "torch"
    if knob == "torch" or p not in (1, 2):
        return "torch"
    return "kernel" if knob == "kernel" or p in PNORM_KERNEL_P else "torch"


class PNorm(CDist):
    def __init__(self, p: float = 2.0, negate: bool = False) -> None:
        super().__init__()

        self.p = p
        self.negate = negate

    def forward(self, A: Tensor, B: Tensor | None = None) -> Tensor:
        other = A if B is None else B
        dims_ok = A.dim() == 2 and other.dim() == 2 and A.shape[1] == other.shape[1]
        device = "cuda" if A.is_cuda and other.is_cuda else "cpu"
        if pnorm_route(self.p, device, A.dtype, other.dtype, dims_ok, os.environ.get("NT_PNORM", "")) == "kernel":
            X = PairwisePNormFunction.apply(A.contiguous(), None if other is A else other.contiguous(),
                                            int(self.p), self.negate)
            # torch.cdist answers bf16 operands in bf16, and in fp32 under autocast
            return X if A.dtype == torch.float32 or torch.is_autocast_enabled() else X.to(A.dtype)
        B = other
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
