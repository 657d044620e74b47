"""GPU: training through the fused MLP head (csrc/mlp_head.hip's training forward, csrc/mlp_head_train.hip's
backward, kernels.mlp_head_train_forward / mlp_head_backward, nn/mlp.py's NT_MLP_TRAIN route) against the same
modules' forward and backward on the CPU in fp64.  The error of y, dx, every dW and every db is helpers.norm_err.

fp32: every case runs the row counts 1, 15, 17, 33 as four launches on the blocks of one 66-row input (dW / db
summed over the launches in fp64) and one launch of MULTI rows that spans three row chunks of the weight-gradient
split; every tensor <= 1e-5, and tensors of >= 64 elements no further from fp64 than 4 x torch's fp32 CPU backward.
bf16 autocast: no further from fp64 than 2 x torch's own bf16-autocast backward on the same device.
Run with -s to see the figures.  Measured on an MI355X (worst tensor of a case, kernel / the comparison):
fp32 [300, 64, 1] 3.5e-7 / 5.3e-7, [300, 5] 3.1e-7 / 3.4e-7, [36, 8, 8, 17] 4.5e-7 / 6.7e-7, [300, 300, 300, 6]
7.1e-7 / 6.0e-7, [36, 512, 512, 3] 8.6e-7 / 6.3e-7, [300, 256, 1] strided 5.0e-7 / 4.6e-7; bf16 autocast
[300, 256, 64] up to 4.3e-3 / 4.6e-3, [304, 512, 512, 64] up to 6.5e-3 / 6.3e-3 (worst ratio 1.07)."""
import copy

import pytest
import torch
import torch.nn as nn

from helpers import FP32_NORM_TOL, norm_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = (1, 15, 17, 33)
# chunk_rule (csrc/mlp_head_train.hip): ceil(293 / 128) = 3 chunks of ceil(293 / 3) = 98 -> 128 rows: 128, 128, 37
MULTI = 293


def _last_kernel():
    from notorch_amd import _lib

    return _lib.load().nt_last_kernel().decode()


def _chain(dims, act, null_bias=None, seed=0):
    torch.manual_seed(seed)
    lins = [nn.Linear(i, o, bias=k != null_bias) for k, (i, o) in enumerate(zip(dims[:-1], dims[1:]))]
    mods = [lins[0]]
    for lin in lins[1:]:
        mods += [act, lin]
    return nn.Sequential(*mods)


def _cpu(seq, x, dy, dtype):
    """y, the hidden pre-activations and {name: gradient} of a copy of seq in dtype on the CPU."""
    m = copy.deepcopy(seq).cpu().to(dtype)
    xr = x.detach().cpu().to(dtype).requires_grad_()
    zs, v = [], xr
    for mod in m:
        v = mod(v)
        if type(mod) is nn.Linear:
            zs.append(v.detach())
    v.backward(dy.detach().cpu().to(dtype))
    return v.detach(), zs[:-1], {"dx": xr.grad, **{n: p.grad for n, p in m.named_parameters()}}


def _kernel(seq, act, x, dy, splits):
    """y and {name: gradient} of the training kernels, one forward and backward per row block."""
    from notorch_amd import kernels as K

    lins = [m for m in seq if type(m) is nn.Linear]
    names = [n for n, _ in seq.named_parameters()]
    Ws = [m.weight.detach().to(DEV) for m in lins]
    bs = [None if m.bias is None else m.bias.detach().to(DEV) for m in lins]
    code = K.act_code(act)
    ys, dxs, sums = [], [], None
    for xb, dyb in zip(torch.split(x, splits), torch.split(dy, splits)):
        y, saved = K.mlp_head_train_forward(xb, Ws, bs, code)
        assert _last_kernel() == "mlp_head_train_f32" and len(saved) == len(lins) - 1
        dx, dWs, dbs = K.mlp_head_backward(dyb.contiguous(), xb, saved, Ws, [b is not None for b in bs], code)
        assert _last_kernel() == "mlp_head_backward_f32"
        grads = [g.double().cpu() for pair in zip(dWs, dbs) for g in pair if g is not None]
        sums = grads if sums is None else [a + b for a, b in zip(sums, grads)]
        ys.append(y), dxs.append(dx)
    return torch.cat(ys), {"dx": torch.cat(dxs), **dict(zip(names, sums))}


CASES = [
    ([300, 64, 1], nn.ReLU(), None, False, 0),
    ([300, 5], nn.ReLU(), None, False, 0),                 # one layer: nothing saved, no LDS tile
    ([36, 8, 8, 17], nn.SiLU(), None, False, 0),           # the ping-pong returns to its first tile; widths < 16
    ([36, 8, 8, 17], nn.LeakyReLU(0.1), 1, False, 0),      # no bias on the middle layer
    ([300, 300, 300, 6], nn.GELU(), None, False, 0),
    ([36, 512, 512, 3], nn.Tanh(), None, False, 0),
    ([300, 256, 1], nn.ELU(), None, True, 0),              # x is a column slice of a wider tensor
]
IDS = ["relu", "one-layer", "narrow", "null-bias", "h300", "h512", "strided"]


def _fp32_case(dims, act, null_bias, strided, seed, rows):
    seq = _chain(dims, act, null_bias, seed)
    x = torch.randn(rows, dims[0] + 8)[:, 4:4 + dims[0]] if strided else torch.randn(rows, dims[0])
    dy = torch.randn(rows, dims[-1])
    ref_y, zs, ref = _cpu(seq, x, dy, torch.float64)
    if isinstance(act, (nn.ReLU, nn.LeakyReLU)):  # a condition on the input: no derivative hangs on rounding
        assert all(z.abs().min() > 1e-5 * z.abs().max() for z in zs)
    xd = x.to(DEV) if not strided else torch.zeros(rows, dims[0] + 8).to(DEV)[:, 4:4 + dims[0]].copy_(x)
    return seq, xd, dy.to(DEV), ref_y, ref, _cpu(seq, x, dy, torch.float32)[2]


@pytest.mark.parametrize("rows, splits", [(sum(ROWS), ROWS), (MULTI, MULTI)], ids=["seams", "chunks"])
@pytest.mark.parametrize("dims, act, null_bias, strided, seed", CASES, ids=IDS)
def test_fp32_kernels_against_fp64(dims, act, null_bias, strided, seed, rows, splits):
    seq, xd, dyd, ref_y, ref, cpu32 = _fp32_case(dims, act, null_bias, strided, seed, rows)
    y, got = _kernel(seq, act, xd, dyd, splits)
    assert not strided or not xd.is_contiguous()
    assert norm_err(y, ref_y) <= FP32_NORM_TOL
    assert set(got) == set(ref)
    for name, r in ref.items():
        e_dev, e_cpu = norm_err(got[name], r), norm_err(cpu32[name], r)
        print(f"{dims} {rows} rows {name}: kernel vs fp64 {e_dev:.3e}, fp32 CPU vs fp64 {e_cpu:.3e}")
        assert got[name].shape == r.shape and e_dev <= FP32_NORM_TOL, name
        assert r.numel() < 64 or e_dev <= 4 * e_cpu, name


def test_two_runs_give_the_same_bits():
    from notorch_amd import kernels as K

    dims, act = [300, 300, 300, 6], nn.GELU()
    seq, xd, dyd = _fp32_case(dims, act, None, False, 0, MULTI)[:3]
    lins = [m for m in seq if type(m) is nn.Linear]
    Ws, bs = [m.weight.detach().to(DEV) for m in lins], [m.bias.detach().to(DEV) for m in lins]
    y, saved = K.mlp_head_train_forward(xd, Ws, bs, K.act_code(act))
    runs = [K.mlp_head_backward(dyd, xd, saved, Ws, [True] * 3, K.act_code(act)) for _ in range(2)]
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16], ids=["x-fp32", "x-bf16"])
@pytest.mark.parametrize("in_dim, hidden, layers, act", [(300, 256, 1, nn.SiLU), (304, 512, 2, nn.GELU)],
                         ids=["300-256-64-silu", "304-512-512-64-gelu"])
def test_bf16_autocast_module_against_fp64(monkeypatch, in_dim, hidden, layers, act, x_dtype):
    from notorch_amd.nn import MLP

    torch.manual_seed(1)
    head = MLP(in_dim, 64, hidden_dim=hidden, num_layers=layers, activation=act).train()
    x = torch.randn(sum(ROWS), in_dim).to(x_dtype)
    dy = torch.randn(sum(ROWS), 64).bfloat16()
    ref = _cpu(nn.Sequential(*head), x, dy, torch.float64)[2]
    head = head.to(DEV)
    got = {}
    for knob in ("torch", "kernel"):
        monkeypatch.setenv("NT_MLP_TRAIN", knob)
        head.zero_grad()
        xd = x.to(DEV).requires_grad_()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = head(xd)
        assert y.dtype == torch.bfloat16
        y.backward(dy.to(DEV))
        got[knob] = {"dx": xd.grad, **{n: p.grad.clone() for n, p in head.named_parameters()}}
        assert xd.grad.dtype == x_dtype
    assert _last_kernel() == "mlp_head_train_bf16"  # the backward's name stays with the autograd thread
    for name, r in ref.items():
        e_dev, e_torch = norm_err(got["kernel"][name], r), norm_err(got["torch"][name], r)
        print(f"{in_dim}-{hidden}x{layers}-64 {x_dtype} {name}: kernel vs fp64 {e_dev:.3e}, torch {e_torch:.3e}")
        assert r.numel() >= 64 and e_dev <= 2 * e_torch, name


def test_bf16_relu_in_exact_arithmetic():
    """Inputs for which every product, sum and rounding of the bf16 instance is exact, so the derivative mask and
    the rounding points are tested without a tolerance.  First-layer pre-activations are odd multiples of 0.5;
    a second-layer one can be exactly 0, where torch and the kernel both take the derivative 0."""
    from notorch_amd import kernels as K

    torch.manual_seed(3)
    dims, rows, act = [8, 8, 8, 4], 33, nn.ReLU()
    seq = _chain(dims, act)
    with torch.no_grad():
        for p in seq.parameters():
            p.copy_(torch.randint(-1, 2, p.shape) if p.dim() == 2 else torch.randint(0, 2, p.shape) - 0.5)
    x, dy = torch.randint(-1, 2, (rows, 8)).float(), torch.randint(-1, 2, (rows, 4)).float()
    ref_y, zs, ref = _cpu(seq, x, dy, torch.float64)
    assert zs[0].abs().min() > 0 and all(z.abs().max() <= 68.5 for z in zs)  # conditions on the input
    assert torch.equal(ref_y.bfloat16().double(), ref_y)
    lins = [m for m in seq if type(m) is nn.Linear]
    Ws, bs = [m.weight.detach().to(DEV) for m in lins], [m.bias.detach().to(DEV) for m in lins]
    y, saved = K.mlp_head_train_forward(x.to(DEV), Ws, bs, K.act_code(act), torch.bfloat16)
    assert _last_kernel() == "mlp_head_train_bf16" and y.dtype == saved[0].dtype == torch.bfloat16
    dx, dWs, dbs = K.mlp_head_backward(dy.to(DEV).bfloat16(), x.to(DEV), saved, Ws, [True] * 3, K.act_code(act))
    got = {"dx": dx, **dict(zip([n for n, _ in seq.named_parameters()], [g for p in zip(dWs, dbs) for g in p]))}
    assert torch.equal(y.double().cpu(), ref_y)
    for name, r in ref.items():
        assert torch.equal(got[name].double().cpu(), r), name


@pytest.mark.parametrize("case, expect", [
    ("train", "mlp_head_train_f32"), ("unset", None), ("dropout", None), ("frozen", None), ("knob-torch", None),
    ("no-grad", "mlp_head_f32")])
def test_module_routes(monkeypatch, case, expect):
    """The kernel routes are proved by nt_last_kernel (per thread: the training forward's name, the backward runs
    on the autograd thread and is proved by its gradients); the torch route by its absence: a one-layer bf16 launch
    ahead of the step leaves its own name there."""
    from notorch_amd import kernels as K
    from notorch_amd.nn import MLP

    monkeypatch.setenv("NT_MLP", "torch" if case == "knob-torch" else "kernel")
    if case == "unset":
        monkeypatch.delenv("NT_MLP_TRAIN", raising=False)
    else:
        monkeypatch.setenv("NT_MLP_TRAIN", "kernel")
    torch.manual_seed(2)
    head = MLP(300, (2, 3), hidden_dim=64, num_layers=2, dropout=0.1 if case == "dropout" else 0.0,
               activation=nn.SiLU).to(DEV).train()
    if case == "frozen":
        head[0].bias.requires_grad_(False)
    x = torch.randn(33, 300, device=DEV, requires_grad=True)
    K.mlp_head(torch.zeros(1, 4, device=DEV), [torch.zeros(2, 4, device=DEV)], [None], (0, 0.0), torch.bfloat16)
    if case == "no-grad":
        with torch.no_grad():
            assert head(x).shape == (33, 2, 3)
    else:
        y = head(x)
        assert y.shape == (33, 2, 3)
        assert _last_kernel() == ("mlp_head_train_f32" if case == "train" else "mlp_head_bf16")
        y.backward(torch.ones_like(y))
        assert all(p.grad is not None for p in head.parameters() if p.requires_grad) and x.grad is not None
    assert _last_kernel() == (expect or "mlp_head_bf16")
    if case == "train":
        ref = _cpu(nn.Sequential(*head), x, torch.ones(33, 2, 3), torch.float64)[2]
        got = {"dx": x.grad, **{n: p.grad for n, p in head.named_parameters()}}
        assert all(norm_err(got[n], r) <= FP32_NORM_TOL for n, r in ref.items())
