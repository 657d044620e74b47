"""``MLP`` head (reference ``notorch/nn/mlp.py:9-68``), SURVEY §8(f) row 4.

The module tree is the reference's: ``Linear, act, Dropout, Linear, ..., Linear`` (the dropout before the
first layer and the activation after the last one are left out), optionally followed by ``nn.Unflatten``, so
the ``state_dict`` keys (``0.weight``, ``3.weight``, ...) and the output shape match.  ``MLP(...)`` returns an
``nn.Sequential`` subclass, :class:`MLPHead`, whose ``forward`` has two routes (``mlp_route``) and, for a forward
that needs an autograd graph, an opt-in third (``mlp_train_route``, below):

* ``"kernel"``: the inference forward of the whole chain in ONE launch of ``nt_mlp_head_forward``
  (``csrc/mlp_head.hip``): 16 rows per workgroup, their activations in LDS from layer to layer, weights read
  in ``nn.Linear``'s own layout.  fp32 throughout runs the exact fp32 MFMA chain; under
  ``torch.autocast("cuda", dtype=torch.bfloat16)`` the bf16 instance rounds where autocast's ``nn.Linear``
  and activation round, and returns bf16.  ``Unflatten`` stays a view of the kernel's output.
* ``"torch"``: ``nn.Sequential.forward``, bit for bit what it was.  Training through the head (an autograd
  graph is needed, or dropout is active) takes it unless ``NT_MLP_TRAIN=kernel`` is set: the inference kernel
  keeps no activations for a backward.  So does anything the kernel route does not state: an edited child list,
  hooks on a child, other dtypes, an autocast of another dtype, widths beyond ``nt_mlp_head_supported``, a CPU
  input.

Knob ``NT_MLP`` (read per call): ``kernel`` takes the kernel wherever the route allows, ``torch`` never;
unset, the kernel runs where ``tools/mlp_bench.py`` measured it ahead of the torch route in every run by
more than that route's spread: 1 to 4096 rows, widths up to 300, two or three linear layers
(``MLP_KERNEL_ROWS`` / ``MLP_KERNEL_MAX_WIDTH`` / ``MLP_KERNEL_LAYERS``; DESIGN.md §4 has the table).  At 32768
rows the library GEMMs are ahead, so large batches stay on them.

Training on the kernels (knob ``NT_MLP_TRAIN``, read per call; opt-in).  With ``NT_MLP_TRAIN=kernel`` a forward that
needs an autograd graph runs ``nt_mlp_head_forward_train`` (the same chain in one launch, which also stores every
hidden layer's pre-activation) under a ``torch.autograd.Function`` whose backward is ``nt_mlp_head_backward``
(``csrc/mlp_head_train.hip``): the dX chain in one launch, every ``dW`` / ``db`` in a second over one work list, and
a fixed-order reduce of the row chunks' partials when there are several; at most three launches whatever the
depth, bit-reproducible, no double backward.  ``mlp_train_route`` takes it only for a CUDA input, an intact chain
without hooks, no active dropout (``p > 0`` in training stays on torch), fp32 throughout or bf16 autocast,
``nt_mlp_head_train_supported`` and parameters that all require grad.  Unset, ``NT_MLP_TRAIN=torch`` or
``NT_MLP=torch``: training is bit for bit what it was.  ``NT_MLP`` and ``mlp_route`` do not change meaning.
"""
from __future__ import annotations

import os
from collections.abc import Sequence
from math import prod

import torch
import torch.nn as nn

from notorch_amd import kernels as K
from notorch_amd.nn.gnn import _engine

DEFAULT_HIDDEN_DIM = 256  # notorch/conf.py:11

# Where the kernel is the default (NT_MLP unset): row counts lo <= rows <= hi, for fp32 and for bf16 autocast,
# the widest layer (input included) and the numbers of linear layers it was measured at.  (0, 0): nowhere.
# From tools/mlp_bench.py (profiles/mlp_head/mlp_bench.jsonl): ahead of the torch route at 64, 512 and 4096
# rows in every run (1.2x to 1.8x), behind it at 32768 (0.4x to 0.65x: a 16-row tile re-reads W per tile).
MLP_KERNEL_ROWS: dict = {"fp32": (1, 4096), "bf16": (1, 4096)}
MLP_KERNEL_MAX_WIDTH = 300
MLP_KERNEL_LAYERS = (2, 3)

__all__ = ["MLP", "MLPHead", "mlp_route", "mlp_train_route", "DEFAULT_HIDDEN_DIM", "MLP_KERNEL_ROWS",
           "MLP_KERNEL_MAX_WIDTH", "MLP_KERNEL_LAYERS"]


def mlp_route(device_type: str, chain_ok: bool, hooks: bool, dropout_active: bool, needs_grad: bool,
              x_dtype: torch.dtype, param_dtype: torch.dtype | None, autocast: str, supported: bool,
              rows: int, widest: int, nlayers: int, knob: str = "") -> str:
    """``"kernel"`` or ``"torch"`` for one forward of the head; pure, so it is tested without a GPU.
    ``chain_ok``: the children are still ``Linear, (act, Dropout, Linear)*, [Unflatten]`` with one shared
    activation that has a kernel code.  ``param_dtype``: the dtype all parameters share, None if they differ.
    ``autocast``: ``""`` (off), ``"bf16"`` or ``"other"``.  ``supported``: ``nt_mlp_head_supported``.
    ``rows``, ``widest`` (the widest layer, input included) and ``nlayers`` (linear layers) only matter to the
    measured default.  ``knob`` is the value of ``NT_MLP``."""
    if knob == "torch" or device_type != "cuda" or not chain_ok or hooks or dropout_active or needs_grad:
        return "torch"
    if autocast == "bf16":
        mode = "bf16"
        if x_dtype not in (torch.float32, torch.bfloat16) or param_dtype not in (torch.float32, torch.bfloat16):
            return "torch"
    elif autocast == "" and x_dtype == param_dtype == torch.float32:
        mode = "fp32"
    else:
        return "torch"
    if not supported:
        return "torch"
    if knob == "kernel":
        return "kernel"
    lo, hi = MLP_KERNEL_ROWS[mode]
    measured = lo <= rows <= hi and rows > 0 and widest <= MLP_KERNEL_MAX_WIDTH and nlayers in MLP_KERNEL_LAYERS
    return "kernel" if measured else "torch"


def mlp_train_route(device_type: str, chain_ok: bool, hooks: bool, dropout_active: bool, needs_grad: bool,
                    all_params_grad: bool, x_dtype: torch.dtype, param_dtype: torch.dtype | None, autocast: str,
                    supported: bool, train_knob: str = "", knob: str = "") -> str:
    """``"kernel"`` (the training kernels) or ``"torch"`` for one forward that may need an autograd graph; pure.
    Arguments as ``mlp_route``; ``all_params_grad``: every parameter requires grad; ``supported``:
    ``nt_mlp_head_train_supported``; ``train_knob`` / ``knob``: the values of ``NT_MLP_TRAIN`` / ``NT_MLP``."""
    if train_knob != "kernel" or knob == "torch" or not needs_grad or not all_params_grad:
        return "torch"
    if device_type != "cuda" or not chain_ok or hooks or dropout_active or not supported:
        return "torch"
    if autocast == "bf16":
        ok = x_dtype in (torch.float32, torch.bfloat16) and param_dtype in (torch.float32, torch.bfloat16)
    else:
        ok = autocast == "" and x_dtype == param_dtype == torch.float32
    return "kernel" if ok else "torch"


def _kernel_rows(x: torch.Tensor, width: int) -> torch.Tensor:
    """x as the kernels take it: rows a whole number of 16-byte pieces apart go as they are (a column slice);
    anything else is copied once."""
    if not (x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= width and x.stride(0) * x.element_size() % 16 == 0):
        x = x.contiguous()
    return x


class _MLPHeadTrain(torch.autograd.Function):
    """The head's chain on the training kernels: forward(x, act, out_dtype, n, W_1..W_n, b_1..b_n (or None))."""

    @staticmethod
    def forward(ctx, x, act, out_dtype, n, *params):
        weights, biases = params[:n], params[n:]
        xk = _kernel_rows(x.detach(), weights[0].shape[1])
        y, saved = K.mlp_head_train_forward(xk, [w.detach() for w in weights],
                                            [None if b is None else b.detach() for b in biases], act, out_dtype)
        ctx.save_for_backward(xk, *weights, *saved)
        ctx.act, ctx.n, ctx.has_bias = act, n, [b is not None for b in biases]
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        n = ctx.n
        xk, weights, saved = ctx.saved_tensors[0], ctx.saved_tensors[1:1 + n], ctx.saved_tensors[1 + n:]
        dx, dWs, dbs = K.mlp_head_backward(dy.contiguous(), xk, saved, weights, ctx.has_bias, ctx.act,
                                           need_dx=ctx.needs_input_grad[0])
        return (dx, None, None, None, *dWs, *dbs)


class MLPHead(nn.Sequential):
    """The ``nn.Sequential`` that ``MLP`` builds, with the fused inference route and the opt-in training route
    (module docstring)."""

    def _chain(self):
        """(linears, activation code) if the children are still the chain ``MLP`` built, else None."""
        mods = list(self)
        if mods and type(mods[-1]) is nn.Unflatten:
            mods.pop()
        if len(mods) % 3 != 1 or any(type(m) is not nn.Linear for m in mods[0::3]):
            return None
        acts, drops = mods[1::3], mods[2::3]
        if any(a is not acts[0] for a in acts) or any(type(d) is not nn.Dropout for d in drops):
            return None
        try:
            code = K.act_code(acts[0]) if acts else (0, 0.0)
        except NotImplementedError:
            return None
        return mods[0::3], code

    def forward(self, input):
        knob = os.environ.get("NT_MLP", "")
        if knob == "torch" or not isinstance(input, torch.Tensor) or input.device.type != "cuda" or input.dim() < 1:
            return super().forward(input)
        chain = self._chain()
        linears = chain[0] if chain else []
        params = [p for m in linears for p in (m.weight, m.bias) if p is not None]
        dtypes = {p.dtype for p in params}
        pdt = dtypes.pop() if len(dtypes) == 1 else None
        dims = [linears[0].in_features, *(m.out_features for m in linears)] if linears else [0, 0]
        if torch.is_autocast_enabled("cuda"):
            autocast = "bf16" if _engine.autocast_bf16(input.device) else "other"
        else:
            autocast = ""
        chain_ok = chain is not None and input.shape[-1] == dims[0]
        hooks = any(m._forward_hooks or m._forward_pre_hooks for m in self)
        dropout_active = self.training and any(type(m) is nn.Dropout and m.p > 0 for m in self)
        needs_grad = torch.is_grad_enabled() and (input.requires_grad or any(p.requires_grad for p in params))
        out_dtype = torch.bfloat16 if autocast == "bf16" else torch.float32
        train_knob = os.environ.get("NT_MLP_TRAIN", "")
        if needs_grad and train_knob == "kernel" and mlp_train_route(
                input.device.type, chain_ok, hooks, dropout_active, needs_grad,
                all(p.requires_grad for p in params), input.dtype, pdt, autocast,
                chain_ok and pdt is not None and K.mlp_head_train_supported(input.dtype, pdt, dims),
                train_knob, knob) == "kernel":
            out = _MLPHeadTrain.apply(input, chain[1], out_dtype, len(linears), *(m.weight for m in linears),
                                      *(m.bias for m in linears))
        else:
            route = mlp_route(
                input.device.type, chain_ok, hooks, dropout_active, needs_grad, input.dtype, pdt, autocast,
                chain is not None and pdt is not None and K.mlp_head_supported(input.dtype, pdt, dims),
                input.numel() // max(input.shape[-1], 1), max(dims), len(linears), knob)
            if route != "kernel":
                return super().forward(input)
            out = K.mlp_head(_kernel_rows(input, dims[0]), [m.weight for m in linears], [m.bias for m in linears],
                             chain[1], out_dtype=out_dtype)
        last = self[len(self) - 1]
        return last(out) if type(last) is nn.Unflatten else out


def MLP(
    input_dim: int,
    output_size: int | Sequence[int],
    hidden_dim: int = DEFAULT_HIDDEN_DIM,
    num_layers: int = 1,
    dropout: float = 0.0,
    activation: type[nn.Module] = nn.ReLU,
) -> nn.Sequential:
    """input_dim -> num_layers hidden layers of hidden_dim -> output_size (an int, or a shape the last
    dimension is unflattened into).  One activation and one dropout module, shared by every block,
    as in the reference (neither holds parameters)."""
    shape = None if isinstance(output_size, int) else tuple(output_size)
    out_dim = output_size if shape is None else prod(shape)
    act, drop = activation(), nn.Dropout(dropout)
    widths = [input_dim, *([hidden_dim] * num_layers), out_dim]
    mods: list[nn.Module] = []
    for k, (d_in, d_out) in enumerate(zip(widths[:-1], widths[1:])):
        if k > 0:  # between two linear layers: activation, then dropout
            mods += [act, drop]
        mods.append(nn.Linear(d_in, d_out))
    mlp = MLPHead(*mods)
    if shape is not None:
        mlp.append(nn.Unflatten(-1, shape))
    return mlp
