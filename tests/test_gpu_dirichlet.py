"""GPU: the Dirichlet loss on nt_dirichlet_loss (csrc/dirichlet_loss.hip), through K.dirichlet_loss and the module,
with the yardstick, criterion and helpers of tests/test_gpu_task_loss.py (the fp64 CPU route; 1e-5 on loss and
gradient; bf16 gradient within 2^-8 + 1e-5).  Logits are 3 randn: about one class in twenty reaches a >= 6, the
series side of dirichlet_math.hpp."""
import functools

import pytest
import torch

from test_gpu_task_loss import DEV, TOL, _check, _K, _run

pytestmark = pytest.mark.gpu

# (b, t, k): the smallest case; many elements at W = 2; W = 4 with an idle lane; W = 8 with three; a full W = 64
# group; a lane's second and third class trip; exactly 8192 lane slots (one launch); 8194 and 8200 (three launches)
SHAPES = ((1, 1, 2), (65, 3, 2), (64, 1, 3), (33, 2, 5), (7, 1, 64), (5, 1, 65), (3, 1, 130), (4096, 1, 2),
          (4097, 1, 2), (1025, 2, 4))


def _module():
    from notorch_amd.nn.loss import Dirichlet

    return Dirichlet()


@functools.lru_cache(maxsize=None)
def _inputs(b, t, k):
    """fp32 CPU tensors: logits, targets, the random mask, weights."""
    gen = torch.Generator().manual_seed(10000 * b + 100 * t + k)
    x, y = 3 * torch.randn(b, t, k, generator=gen), torch.randint(0, k, (b, t), generator=gen).float()
    return x.contiguous(), y, torch.rand(b, t, generator=gen) < 0.6, torch.rand(b, generator=gen) + 0.5


@pytest.mark.parametrize("b,t,k", SHAPES)
def test_kernel_matches_the_fp64_torch_route(b, t, k, monkeypatch):
    monkeypatch.setenv("NT_LOSS", "kernel")
    x, y, rnd, w_rnd = _inputs(b, t, k)
    for which, mask in (("none", None), ("random", rnd), ("all-false", torch.zeros(b, t, dtype=torch.bool))):
        for w in (None, w_rnd):
            want = _run(_module(), x.double(), y, mask, w, {}, "cpu", torch.float64)
            _check("dirichlet", f"b={b} t={t} k={k} mask={which} weights={w is not None}",
                   _run(_module(), x, y, mask, w, {}, DEV, torch.float32), want)


@pytest.mark.parametrize("b,t,k", ((33, 2, 5), (1025, 2, 4)))
def test_bf16_logits(b, t, k, monkeypatch):
    monkeypatch.setenv("NT_LOSS", "kernel")
    x, y, rnd, w = _inputs(b, t, k)
    got = _run(_module(), x.bfloat16(), y, rnd, w, {}, DEV, torch.bfloat16)
    assert got[1].dtype == torch.bfloat16
    want = _run(_module(), x.bfloat16().double(), y, rnd, w, {}, "cpu", torch.float64)
    _check("dirichlet_bf16", f"b={b} t={t} k={k}", got, want, gtol=2.0 ** -8 + TOL)


@pytest.mark.parametrize("b,t,k", ((65, 3, 2), (4097, 1, 2)))
def test_two_calls_return_the_same_bits(b, t, k):
    x, y, rnd, w = _inputs(b, t, k)
    args = (x.to(DEV), y.to(DEV), rnd.to(DEV), w.to(DEV), 0.2, True)
    (a_loss, a_g), (b_loss, b_g) = _K().dirichlet_loss(*args), _K().dirichlet_loss(*args)
    assert torch.equal(a_loss, b_loss) and torch.equal(a_g, b_g) and torch.isfinite(a_g).all().item()


@pytest.mark.parametrize("bad", (-1.0, 5.0, float("nan")))
def test_a_target_that_is_no_class_is_nan_in_its_element_alone(bad):
    x, y, _, _ = _inputs(33, 2, 5)
    y = y.clone()
    y[7, 1] = bad
    loss, g = _K().dirichlet_loss(x.to(DEV), y.to(DEV), None, None, 0.2, True)
    nan = torch.isnan(g).cpu()
    assert torch.isnan(loss).item() and nan[7, 1].all().item() and nan.sum().item() == 5


def test_gradient_reaches_an_upstream_linear(monkeypatch):
    gen = torch.Generator().manual_seed(3)
    x, y = torch.randn(257, 16, generator=gen).to(DEV), torch.randint(0, 3, (257, 2), generator=gen).to(DEV)
    mask = (torch.rand(257, 2, generator=gen) < 0.7).to(DEV)
    torch.manual_seed(0)
    head, res = torch.nn.Linear(16, 6).to(DEV), []
    for knob in ("kernel", "torch"):
        monkeypatch.setenv("NT_LOSS", knob)
        head.zero_grad(set_to_none=True)
        loss = _module()(head(x).view(257, 2, 3), y, mask=mask)
        loss.backward()
        res.append((loss.detach(), torch.cat([head.weight.grad.flatten(), head.bias.grad])))
    _check("dirichlet", "head gradient vs the device torch route", res[0], (res[1][0].double(), res[1][1].double().cpu()))


def test_routing(monkeypatch):
    K, seen = _K(), []
    real = K.dirichlet_loss
    monkeypatch.setattr(K, "dirichlet_loss", lambda *a: seen.append(a[-1]) or real(*a))
    x, y, mod = _inputs(65, 3, 2)[0].to(DEV), _inputs(65, 3, 2)[1].to(DEV), _module()
    monkeypatch.setenv("NT_LOSS", "kernel")
    on_kernel = mod(x, y)
    with torch.no_grad():
        mod(x.clone().requires_grad_(), y.long())  # class indices as integers; no gradient buffer
    assert seen == [False, False] and mod.KIND is None
    assert mod(x.double(), y.double()).dtype == torch.float64 and mod(x.cpu(), y.cpu()).device.type == "cpu"
    monkeypatch.setenv("NT_LOSS", "torch")  # the knob, read per call
    assert abs(on_kernel.item() - mod(x, y).item()) <= TOL * max(1.0, on_kernel.item()) and len(seen) == 2
