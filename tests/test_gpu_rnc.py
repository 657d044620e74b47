"""GPU: RankNContrastLoss on the sort-and-scan kernel nt_rnc_rank (csrc/rnc.hip).

Inputs are X = 0.5 randn(N, 8) at temp 2.0, so s = exp(Sim / temp) stays above ~0.1 and nothing
underflows.  The yardstick is the module's torch route on the same Sim and D, in fp64 on the CPU
(tests/test_rnc.py ties that route to the literal N x N x N form).  The criterion is the fp32 contract
of 1e-5 on scales that do not vanish:
    |L - L64| <= 1e-5 max(1, |L64|)
    max|dSim - dSim64| <= 1e-5 max(max|dSim64|, 1 / (temp N (N - 1)))
(at N = 2, and for each row's farthest j, loss term and gradient are ~EPS / s: plain relative error
means nothing there).  Every case prints ``RNCERR <class> <value> <case>``."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
TEMP, EPS, TOL = 2.0, 1e-6, 1e-5
# (N, targets): degenerate scans; the wave edge; power-of-two padding over several waves; tie groups of
# ~200 that cross waves; one group with k = i inside every sum; the largest N, once
CASES = ((2, "distinct"), (3, "distinct"), (63, "distinct"), (64, "distinct"), (65, "distinct"),
         (257, "distinct"), (1000, "five"), (1000, "equal"), (4096, "distinct"))


def _K():
    from notorch_amd import kernels

    return kernels


def _L():
    from notorch_amd.nn import loss

    return loss


def _report(cls, err, case):
    print(f"RNCERR {cls} {err:.3e} {case}")


def _inputs(n, kind):
    gen = torch.Generator().manual_seed(1000 * n + len(kind))
    x = 0.5 * torch.randn(n, 8, generator=gen)
    if kind == "distinct":
        t = torch.randn(n, 2, generator=gen)
    elif kind == "five":
        t = torch.randint(0, 5, (n, 1), generator=gen).float()
    else:
        t = torch.full((n, 1), 1.5)
    return x, t


@functools.lru_cache(maxsize=None)
def _case(n, kind):
    """Sim, D (fp32, on the device, from the default PNorms) and the fp64 CPU yardstick (L64, dSim64)."""
    from notorch_amd.nn.loss.rnc import rank_loss_torch

    x, t = _inputs(n, kind)
    crit = _L().RankNContrastLoss()
    with torch.no_grad():
        sim = crit.similarity(x.to(DEV)).contiguous()
        dist = crit.distance(t.to(DEV)).contiguous()
    s64 = sim.double().cpu().requires_grad_()
    l64 = rank_loss_torch(s64, dist.double().cpu(), TEMP, EPS)
    (g64,) = torch.autograd.grad(l64, s64)
    return sim, dist, l64.item(), g64


def _grad_floor(n):
    return 1.0 / (TEMP * n * (n - 1))


@pytest.mark.parametrize("n,kind", CASES)
def test_kernel_matches_the_fp64_torch_route(n, kind):
    from notorch_amd.nn.loss.rnc import RnCRankFunction

    sim, dist, l64, g64 = _case(n, kind)
    leaf = sim.clone().requires_grad_()
    loss = RnCRankFunction.apply(leaf, dist, TEMP, EPS, True)
    loss.backward()
    assert loss.dtype == torch.float32 and loss.dim() == 0
    e_loss = abs(loss.item() - l64) / max(1.0, abs(l64))
    e_grad = (leaf.grad.double().cpu() - g64).abs().max().item() / max(g64.abs().max().item(), _grad_floor(n))
    _report("loss", e_loss, f"N={n} {kind} L64={l64:.6f}")
    _report("dsim", e_grad, f"N={n} {kind} max|dSim64|={g64.abs().max().item():.3e}")
    assert e_loss <= TOL
    assert e_grad <= TOL
    if kind != "distinct":  # k = i is inside the sums of the anchor's duplicates
        assert leaf.grad.diagonal().abs().max().item() > 0.0


def test_end_to_end_gradient_matches_the_device_torch_route(monkeypatch):
    n = 257
    x, t = _inputs(n, "distinct")
    crit = _L().RankNContrastLoss().to(DEV)
    grads, losses = [], []
    for knob in (None, "torch"):
        if knob is None:
            monkeypatch.delenv("NT_RNC", raising=False)
        else:
            monkeypatch.setenv("NT_RNC", knob)
        xa = x.to(DEV).requires_grad_()
        loss = crit(xa, t.to(DEV))
        loss.backward()
        grads.append(xa.grad.double().cpu())
        losses.append(loss.item())
    e_loss = abs(losses[0] - losses[1]) / max(1.0, abs(losses[1]))
    e_grad = (grads[0] - grads[1]).abs().max().item() / max(grads[1].abs().max().item(), _grad_floor(n))
    _report("loss_e2e", e_loss, f"N={n} vs the device torch route")
    _report("dinputs", e_grad, f"N={n} vs the device torch route")
    assert e_loss <= TOL and e_grad <= TOL


def test_two_calls_return_the_same_bits():
    K = _K()
    for n, kind in ((1000, "five"), (257, "distinct")):
        sim, dist, _, _ = _case(n, kind)
        a_nll, a_g = K.rnc_rank(sim, dist, TEMP, EPS, True)
        b_nll, b_g = K.rnc_rank(sim, dist, TEMP, EPS, True)
        assert torch.equal(a_nll, b_nll) and torch.equal(a_g, b_g)
        assert torch.isfinite(a_nll).all().item() and torch.isfinite(a_g).all().item()


class _Identity(torch.nn.Module):
    def forward(self, A, B=None):
        return A


@pytest.fixture
def calls(monkeypatch):
    """Count the launches of K.rnc_rank and record (need_grad, dsim is None) of each."""
    K = _K()
    real, seen = K.rnc_rank, []

    def counted(sim, dist, temp, eps, need_grad):
        out = real(sim, dist, temp, eps, need_grad)
        seen.append((bool(need_grad), out[1] is None))
        return out

    monkeypatch.setattr(K, "rnc_rank", counted)
    monkeypatch.delenv("NT_RNC", raising=False)
    return seen


def test_routing(calls, monkeypatch):
    K = _K()
    x, t = _inputs(65, "distinct")
    x, t = x.to(DEV), t.to(DEV)
    crit = _L().RankNContrastLoss()
    on_kernel = crit(x, t)
    assert len(calls) == 1  # fp32 device tensors: the kernel
    monkeypatch.setenv("NT_RNC", "torch")
    on_torch = crit(x, t)
    assert len(calls) == 1  # the knob, read per call
    monkeypatch.delenv("NT_RNC")
    assert abs(on_kernel.item() - on_torch.item()) <= TOL * max(1.0, abs(on_torch.item()))
    out64 = crit(x.double(), t.double())
    assert len(calls) == 1 and out64.dtype == torch.float64  # fp64: torch
    # one above the kernel's limit: precomputed Sim / D through identity CDists, D of few distinct values
    n = K.rnc_max_n() + 1
    gen = torch.Generator().manual_seed(11)
    sim = -torch.rand(n, n, generator=gen).to(DEV)
    dist = torch.randint(0, 3, (n, n), generator=gen).float().to(DEV)
    big = _L().RankNContrastLoss(distance=_Identity(), similarity=_Identity())
    out = big(sim, dist)
    assert len(calls) == 1 and torch.isfinite(out).item()
    # and at the limit's side of the decision the same module takes the kernel
    big(sim[: n - 1, : n - 1], dist[: n - 1, : n - 1])
    assert len(calls) == 2


def test_no_grad_allocates_no_gradient_buffer(calls):
    x, t = _inputs(257, "distinct")
    x, t = x.to(DEV), t.to(DEV)
    crit = _L().RankNContrastLoss()
    with_grad = crit(x.clone().requires_grad_(), t)
    with torch.no_grad():
        without = crit(x.clone().requires_grad_(), t)
    plain = crit(x, t)  # nothing requires a gradient
    assert calls == [(True, False), (False, True), (False, True)]
    assert torch.equal(with_grad, without) and torch.equal(with_grad, plain)
    assert with_grad.requires_grad and not without.requires_grad


def test_bf16_autocast_takes_the_fp32_kernel(calls):
    x, t = _inputs(257, "distinct")
    xb, t = x.to(DEV).bfloat16(), t.to(DEV)
    crit = _L().RankNContrastLoss()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        sim = crit.similarity(xb)
        loss = crit(xb, t)
    # torch.cdist autocasts to fp32: the kernel sees the distances of the widened fingerprints
    assert sim.dtype == torch.float32
    wide = crit(xb.float(), t)
    assert len(calls) == 2
    assert loss.dtype == torch.float32 and torch.equal(loss, wide)
