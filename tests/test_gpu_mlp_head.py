"""GPU: the fused MLP head (csrc/mlp_head.hip, kernels.mlp_head, nn/mlp.py's kernel route) against the same
modules evaluated by torch on the CPU in fp64.

R = 16 rows per workgroup.  Every case runs the four row counts 1, R - 1, R + 1, 2R + 1 as four launches on
consecutive row blocks of one 66-row input; its error is the normalised max error (helpers.norm_err: max |y - ref|
/ max |ref|) over those 66 rows.  fp32: <= 1e-5 and no further from fp64 than 4 x torch's fp32 CPU evaluation.
bf16 autocast: no further from fp64 than 2 x torch's own bf16-autocast evaluation on the same device.
Run with -s to see the figures."""
import pytest
import torch
import torch.nn as nn

from helpers import FP32_NORM_TOL, norm_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
R = 16
ROWS = (1, R - 1, R + 1, 2 * R + 1)
BOUND = 1264  # the stated width bound (nt_mlp_head_supported)


def _last_kernel():
    from notorch_amd import _lib

    return _lib.load().nt_last_kernel().decode()


def _blocks(x):
    return torch.split(x, ROWS)


def _chain(dims, act, null_bias=None, seed=0):
    torch.manual_seed(seed)
    lins = [nn.Linear(i, o, bias=k != null_bias) for k, (i, o) in enumerate(zip(dims[:-1], dims[1:]))]
    mods = [lins[0]]
    for lin in lins[1:]:
        mods += [act, lin]
    return lins, nn.Sequential(*mods)


@pytest.mark.parametrize("dims, act, null_bias, strided", [
    ([300, 256, 1], nn.ReLU(), None, False),           # the default head: out = 1
    ([300, 5], nn.ReLU(), None, False),                # num_layers = 0: no LDS tile at all
    ([36, 8, 8, 17], nn.SiLU(), None, False),          # the ping-pong returns to its first tile; widths < 16
    ([36, 8, 8, 17], nn.LeakyReLU(0.1), 1, False),     # no bias on the middle layer
    ([300, 300, 300, 6], nn.LeakyReLU(0.1), None, False),
    ([36, BOUND, BOUND, 3], nn.ReLU(), None, False),   # the hidden-width bound: 159 KiB of LDS
    ([300, 256, 1], nn.SiLU(), None, True),            # x is a column slice of a wider tensor
], ids=["default", "one-layer", "narrow", "null-bias", "h300", "bound", "strided"])
def test_fp32_kernel_against_fp64(dims, act, null_bias, strided):
    from notorch_amd import kernels as K

    lins, seq = _chain(dims, act, null_bias)
    x = torch.randn(sum(ROWS), dims[0] + 8)[:, 4:4 + dims[0]] if strided else torch.randn(sum(ROWS), dims[0])
    with torch.no_grad():
        ref = seq.double()(x.double())
        cpu32 = seq.float()(x)
    xd = x.to(DEV) if not strided else torch.zeros(sum(ROWS), dims[0] + 8).to(DEV)[:, 4:4 + dims[0]].copy_(x)
    Ws = [m.weight.detach().to(DEV) for m in lins]
    bs = [None if m.bias is None else m.bias.detach().to(DEV) for m in lins]
    outs = [K.mlp_head(xb, Ws, bs, K.act_code(act)) for xb in _blocks(xd)]
    assert _last_kernel() == "mlp_head_f32"
    assert not strided or not _blocks(xd)[-1].is_contiguous()
    out = torch.cat(outs).cpu()
    assert out.dtype == torch.float32 and out.shape == ref.shape
    e_dev, e_cpu = norm_err(out, ref), norm_err(cpu32, ref)
    print(f"{dims}: kernel vs fp64 {e_dev:.3e}, fp32 CPU vs fp64 {e_cpu:.3e}")
    assert e_dev <= FP32_NORM_TOL
    assert e_dev <= 4 * e_cpu


@pytest.mark.parametrize("x_dtype", [torch.float32, torch.bfloat16], ids=["x-fp32", "x-bf16"])
@pytest.mark.parametrize("in_dim, hidden, layers, out_dim", [(300, 256, 1, 1), (304, 512, 2, 3)],
                         ids=["300-256-1", "304-512-512-3"])
def test_bf16_autocast_module_against_fp64(monkeypatch, in_dim, hidden, layers, out_dim, x_dtype):
    from notorch_amd.nn import MLP

    torch.manual_seed(1)
    head = MLP(in_dim, out_dim, hidden_dim=hidden, num_layers=layers).eval()
    x = torch.randn(sum(ROWS), in_dim).to(x_dtype)
    with torch.no_grad():
        ref = nn.Sequential(*head).double()(x.double())
    head = head.float().to(DEV)
    got = {}
    for knob in ("torch", "kernel"):
        monkeypatch.setenv("NT_MLP", knob)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            got[knob] = torch.cat([head(xb) for xb in _blocks(x.to(DEV))])
        assert got[knob].dtype == torch.bfloat16 and got[knob].shape == ref.shape
    assert _last_kernel() == "mlp_head_bf16"
    e_dev, e_torch = norm_err(got["kernel"], ref), norm_err(got["torch"], ref)
    print(f"{in_dim}-{hidden}x{layers}-{out_dim} {x_dtype}: kernel vs fp64 {e_dev:.3e}, torch autocast {e_torch:.3e}")
    assert e_dev <= 2 * e_torch


@pytest.mark.parametrize("case", ["eval", "train", "input-grad", "appended", "knob-torch"])
def test_module_routes(monkeypatch, case):
    """The kernel route is proved by nt_last_kernel naming the fp32 instance; the torch route by its absence:
    a one-layer bf16 launch ahead of the forward leaves its own name there."""
    from notorch_amd import kernels as K
    from notorch_amd.nn import MLP

    monkeypatch.setenv("NT_MLP", "torch" if case == "knob-torch" else "kernel")
    torch.manual_seed(2)
    head = MLP(300, (2, 3), hidden_dim=64, num_layers=2, dropout=0.1, activation=nn.SiLU).to(DEV).eval()
    x = torch.randn(2 * R + 1, 300, device=DEV)
    if case == "train":
        head.train()
    if case == "appended":
        head.append(nn.Sigmoid())
    if case == "input-grad":
        x.requires_grad_()
    K.mlp_head(torch.zeros(1, 4, device=DEV), [torch.zeros(2, 4, device=DEV)], [None], (0, 0.0), torch.bfloat16)
    assert _last_kernel() == "mlp_head_bf16"
    if case in ("train", "input-grad"):
        y = head(x)
        assert y.requires_grad
    else:
        with torch.no_grad():
            y = head(x)
    assert y.shape == (2 * R + 1, 2, 3)
    assert _last_kernel() == ("mlp_head_f32" if case == "eval" else "mlp_head_bf16")
    if case == "eval":
        with torch.no_grad():
            ref = nn.Sequential(*head).cpu().double()(x.cpu().double())
        assert norm_err(y, ref) <= FP32_NORM_TOL
