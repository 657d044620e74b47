"""GPU: the task losses and regression metrics on nt_task_loss (csrc/task_loss.hip).

Inputs: the mean channel and the targets are randn; v and beta are softplus(randn) + 0.1; alpha is
softplus(randn) + 1; BCE targets are 0 / 1, XENT has 5 classes.  The yardstick is the module's torch route on
the same values in fp64 on the CPU (tests/test_task_loss.py ties that route to the literal formulas).  The
criterion is the fp32 contract:
    |L - L64| <= 1e-5 max(1, |L64|)        max|g - g64| <= 1e-5 max|g64|
(torch's own fp32 evaluation stays at or below 2.3e-7 on both, so the bound has room for a device lgammaf and
the hand-written digamma).  Under an all-false mask loss and gradient are NaN on both sides.  bf16 preds are
compared on the same rounded values; their gradient is stored in bf16, one rounding to nearest of the fp32
value: bf16 has 8 significand bits, so an ulp is 2^-7 of the element's binade and the rounding moves an
element by at most half of it, 2^-8 |g| <= 2^-8 max|g64|; the bound is that plus the fp32 contract's 1e-5.
Every case prints
``LOSSERR <kind> <value> <case>``."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-5
KINDS = ("mse", "mae", "rmse", "bce", "mve", "evidential", "xent")
# one element; the wave edge; several waves and t > 1; more than one element per thread; the bench batch; one
# element past the one-launch size (two workgroups, finalize, gradient launch), with t = 3
SIZES = ((1, 1), (63, 1), (64, 1), (65, 3), (1025, 2), (4096, 1), (2731, 3))
MASKS = ("none", "random", "all-false", "one-true")


def _K():
    from notorch_amd import kernels

    return kernels


def _module(kind):
    from notorch_amd.nn import loss as L
    from notorch_amd.nn import metrics as M

    return {"mse": L.MSE, "mae": M.MAE, "rmse": M.RMSE, "bce": L.BCE, "mve": L.MVE, "evidential": L.Evidential,
            "xent": L.XENT}[kind]()


def _sp(gen, b, t):
    return F.softplus(torch.randn(b, t, generator=gen))


@functools.lru_cache(maxsize=None)
def _inputs(kind, b, t):
    """fp32 CPU tensors: preds, targets, the random mask, the one-true mask, weights, lt, gt."""
    gen = torch.Generator().manual_seed(100 * b + 10 * t + len(kind))
    mean, y = torch.randn(b, t, generator=gen), torch.randn(b, t, generator=gen)
    if kind == "bce":
        y = (y > 0).float()
    if kind == "mve":
        p = torch.stack([mean, _sp(gen, b, t) + 0.1], -1)
    elif kind == "evidential":
        p = torch.stack([mean, _sp(gen, b, t) + 0.1, _sp(gen, b, t) + 1, _sp(gen, b, t) + 0.1], -1)
    elif kind == "xent":
        p, y = torch.randn(b, t, 5, generator=gen), torch.randint(0, 5, (b, t), generator=gen).float()
    else:
        p = mean
    rnd = torch.rand(b, t, generator=gen) < 0.6
    one = torch.zeros(b, t, dtype=torch.bool)
    one[b // 2, t - 1] = True
    w = torch.rand(b, generator=gen) + 0.5
    lt, gt = torch.rand(b, t, generator=gen) < 0.5, torch.rand(b, t, generator=gen) < 0.5
    return p.contiguous(), y, rnd, one, w, lt, gt


def _mask(kind, b, t, which):
    _, _, rnd, one, _, _, _ = _inputs(kind, b, t)
    return {"none": None, "random": rnd, "all-false": torch.zeros(b, t, dtype=torch.bool), "one-true": one}[which]


def _run(mod, p, y, mask, w, bounds, dev, dtype):
    """(loss, preds.grad) of mod on dev, all inputs moved there; preds in dtype."""
    q = p.to(dev, dtype).clone().requires_grad_()  # the cached inputs stay as they are
    side = torch.float64 if dtype == torch.float64 else torch.float32  # targets and weights
    kw = {k: v.to(dev) for k, v in bounds.items()}
    loss = mod(q, y.to(dev, side), mask=None if mask is None else mask.to(dev),
               sample_weights=None if w is None else w.to(dev, side), **kw)
    loss.backward()
    return loss.detach(), q.grad


def _check(kind, case, got, want, gtol=TOL):
    (loss, g), (l64, g64) = got, want
    assert loss.dtype == torch.float32 and loss.dim() == 0 and g.dtype != torch.float64
    l64, g64, g = l64.item(), g64, g.double().cpu()
    if l64 != l64:  # the all-false mask: 0 / 0 on both sides
        assert torch.isnan(loss).item() and torch.isnan(g64).all().item() and torch.isnan(g).all().item()
        print(f"LOSSERR {kind} nan {case}")
        return
    e_loss = abs(loss.item() - l64) / max(1.0, abs(l64))
    if g64.abs().max().item() == 0.0:  # every element clamped to its target: exact zeros
        assert g.abs().max().item() == 0.0
        e_grad = 0.0
    else:
        e_grad = (g - g64).abs().max().item() / g64.abs().max().item()
    print(f"LOSSERR {kind} {e_loss:.3e} loss {case} L64={l64:.6f}")
    print(f"LOSSERR {kind} {e_grad:.3e} grad {case} max|g64|={g64.abs().max().item():.3e}")
    assert e_loss <= TOL
    assert e_grad <= gtol


@pytest.mark.parametrize("b,t", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_matches_the_fp64_torch_route(kind, b, t, monkeypatch):
    monkeypatch.setenv("NT_LOSS", "kernel")
    mod = _module(kind)
    p, y, _, _, w_rnd, _, _ = _inputs(kind, b, t)
    for which in MASKS:
        mask = _mask(kind, b, t, which)
        for w in (None, w_rnd):
            want = _run(mod, p.double(), y, mask, w, {}, "cpu", torch.float64)
            got = _run(mod, p, y, mask, w, {}, DEV, torch.float32)
            _check(kind, f"b={b} t={t} mask={which} weights={'none' if w is None else 'random'}", got, want)


@pytest.mark.parametrize("b,t", SIZES)
@pytest.mark.parametrize("kind", ("mse", "mae"))
def test_bounds(kind, b, t, monkeypatch):
    from notorch_amd.nn.loss import BoundedMSE
    from notorch_amd.nn.metrics import BoundedMAE

    monkeypatch.setenv("NT_LOSS", "kernel")
    mod = BoundedMSE() if kind == "mse" else BoundedMAE()
    p, y, rnd, _, w, lt, gt = _inputs(kind, b, t)
    for bounds in (dict(lt_mask=lt, gt_mask=gt), dict(lt_mask=lt, gt_mask=torch.zeros_like(gt))):
        for mask in (None, rnd):
            want = _run(mod, p.double(), y, mask, w, bounds, "cpu", torch.float64)
            got = _run(mod, p, y, mask, w, bounds, DEV, torch.float32)
            _check("bounded_" + kind, f"b={b} t={t} mask={'none' if mask is None else 'random'}", got, want)
            clamped = ((p < y) & bounds["lt_mask"]) | ((p > y) & bounds["gt_mask"])
            assert (got[1].cpu()[clamped] == 0).all().item()


@pytest.mark.parametrize("b,t", ((65, 3), (4096, 1), (2731, 3)))
@pytest.mark.parametrize("kind", ("mse", "mve"))
def test_bf16_preds(kind, b, t, monkeypatch):
    monkeypatch.setenv("NT_LOSS", "kernel")
    mod = _module(kind)
    p, y, rnd, _, w, _, _ = _inputs(kind, b, t)
    pb = p.bfloat16()
    for mask in (None, rnd):
        want = _run(mod, pb.double(), y, mask, w, {}, "cpu", torch.float64)
        got = _run(mod, pb, y, mask, w, {}, DEV, torch.bfloat16)
        assert got[1].dtype == torch.bfloat16
        _check(kind + "_bf16", f"b={b} t={t} mask={'none' if mask is None else 'random'}", got, want,
               gtol=2.0 ** -8 + TOL)


def test_two_calls_return_the_same_bits():
    K = _K()
    for kind, (b, t) in (("evidential", (4096, 1)), ("xent", (2731, 3)), ("mse", (1025, 2))):
        p, y, rnd, _, w, _, _ = _inputs(kind, b, t)
        args = (p.to(DEV), y.to(DEV), kind, rnd.to(DEV), w.to(DEV), None, None, 0.2, 1e-8, True)
        a_loss, a_g = K.task_loss(*args)
        b_loss, b_g = K.task_loss(*args)
        assert torch.equal(a_loss, b_loss) and torch.equal(a_g, b_g)
        assert torch.isfinite(a_loss).item() and torch.isfinite(a_g).all().item()


@pytest.fixture
def calls(monkeypatch):
    """Record (kind, need_grad, dpreds is None) of every K.task_loss."""
    K = _K()
    real, seen = K.task_loss, []

    def counted(preds, targets, kind, *args):
        out = real(preds, targets, kind, *args)
        seen.append((kind, bool(args[-1]), out[1] is None))
        return out

    monkeypatch.setattr(K, "task_loss", counted)
    monkeypatch.delenv("NT_LOSS", raising=False)
    return seen


def test_no_grad_allocates_no_gradient(calls, monkeypatch):
    monkeypatch.setenv("NT_LOSS", "kernel")
    mod = _module("mve")
    p, y, rnd, _, w, _, _ = _inputs("mve", 65, 3)
    p, y = p.to(DEV), y.to(DEV)
    with_grad = mod(p.clone().requires_grad_(), y, mask=rnd.to(DEV))
    with torch.no_grad():
        without = mod(p.clone().requires_grad_(), y, mask=rnd.to(DEV))
    plain = mod(p, y, mask=rnd.to(DEV))  # nothing requires a gradient
    assert calls == [("mve", True, False), ("mve", False, True), ("mve", False, True)]
    assert torch.equal(with_grad, without) and torch.equal(with_grad, plain)
    assert with_grad.requires_grad and not without.requires_grad


def test_routing(calls, monkeypatch):
    from notorch_amd.nn.loss import loss as loss_mod
    from notorch_amd.nn.loss import Dirichlet

    p, y, rnd, _, w, _, _ = _inputs("mse", 65, 3)
    p, y = p.to(DEV), y.to(DEV)
    mod = _module("mse")
    monkeypatch.setenv("NT_LOSS", "kernel")
    on_kernel = mod(p, y)
    assert len(calls) == 1
    monkeypatch.setenv("NT_LOSS", "torch")  # the knob, read per call
    on_torch = mod(p, y)
    assert len(calls) == 1 and abs(on_kernel.item() - on_torch.item()) <= TOL * max(1.0, abs(on_torch.item()))
    monkeypatch.delenv("NT_LOSS")
    mod(p, y)
    assert len(calls) == (1 if "mse" in loss_mod.TORCH_BY_DEFAULT else 2)  # the measured default
    n = len(calls)
    monkeypatch.setenv("NT_LOSS", "kernel")
    assert mod(p.double(), y.double()).dtype == torch.float64 and len(calls) == n  # fp64: torch ops
    assert mod(p.half(), y.half()).dtype == torch.float16 and len(calls) == n
    mod(p, y.clone().requires_grad_())  # a gradient for the targets: autograd
    assert len(calls) == n
    alphas = torch.randn(65, 3, 4, device=DEV)
    assert torch.isfinite(Dirichlet()(alphas, torch.randint(0, 4, (65, 3), device=DEV))).item()
    assert len(calls) == n  # Dirichlet has no kernel


@pytest.mark.parametrize("kind", ("mse", "mve", "evidential"))
def test_gradient_reaches_an_upstream_linear(kind, monkeypatch):
    """head -> (softplus on the variance-like channels) -> loss, kernel route against the device torch route."""
    b, t, h = 257, 2, 16
    c = {"mse": 1, "mve": 2, "evidential": 4}[kind]
    gen = torch.Generator().manual_seed(c)
    x, y = torch.randn(b, h, generator=gen).to(DEV), torch.randn(b, t, generator=gen).to(DEV)
    mask = (torch.rand(b, t, generator=gen) < 0.7).to(DEV)
    torch.manual_seed(0)
    head = torch.nn.Linear(h, t * c).to(DEV)
    mod = _module(kind)
    res = []
    for knob in ("kernel", "torch"):
        monkeypatch.setenv("NT_LOSS", knob)
        head.zero_grad(set_to_none=True)
        out = head(x).view(b, t, c)
        if c == 1:
            out = out.squeeze(-1)
        else:
            shift = torch.tensor([0.0, 0.1, 1.0, 0.1][:c], device=DEV)
            out = torch.cat([out[..., :1], F.softplus(out[..., 1:]) + shift[1:]], -1)
        loss = mod(out, y, mask=mask)
        loss.backward()
        res.append((loss.item(), head.weight.grad.double().cpu(), head.bias.grad.double().cpu()))
    (lk, wk, bk), (lt_, wt, bt) = res
    e_loss = abs(lk - lt_) / max(1.0, abs(lt_))
    e_w = (wk - wt).abs().max().item() / wt.abs().max().item()
    e_b = (bk - bt).abs().max().item() / bt.abs().max().item()
    print(f"LOSSERR {kind} {e_loss:.3e} loss_e2e vs the device torch route")
    print(f"LOSSERR {kind} {max(e_w, e_b):.3e} head_grad vs the device torch route")
    assert e_loss <= TOL and e_w <= TOL and e_b <= TOL
