"""GPU: the pairwise p-norm kernels nt_pairwise_pnorm / nt_pairwise_pnorm_backward (csrc/pairwise.hip) and
their route through PNorm and RankNContrastLoss, at the seams of the tiles, the k chunk and the j split.
The yardstick is the direct formula in fp64 on the CPU from the exactly widened values, and autograd's
gradient of it for a seeded G (sqrt guarded at 0: equal rows take the 0 gradient of torch's direct form).
Forward, per element: |X - X64| <= (d + 4) 2^-24 |X64|, the first-order rounding bound of a sum of d
non-negative terms (a subtract and a multiply each) and a square root, whatever the summation order.
Backward: max|dA - dA64| / max|dA64| <= 1e-5 and at most 4 x that figure of the formula in fp32 on the CPU."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
SHAPES = ((1, 1), (127, 129), (128, 128), (129, 257))


def _K():
    from notorch_amd import kernels

    return kernels


def _direct(A, B, p):
    diff = A[:, None] - B[None]
    if p == 1:
        return diff.abs().sum(-1)
    s = diff.square().sum(-1)
    return torch.where(s > 0, torch.where(s > 0, s, torch.ones_like(s)).sqrt(), torch.zeros_like(s))


@functools.lru_cache(maxsize=None)
def _inputs(n, m, d):
    gen = torch.Generator().manual_seed(7 + 1000 * n + 10 * m + d)
    return torch.randn(n, d, generator=gen), torch.randn(m, d, generator=gen), torch.randn(n, m, generator=gen)


def _check_forward(X, X64, d):
    excess = ((X.double().cpu() - X64).abs() - (d + 4) * U * X64.abs()).max().item()
    assert excess <= 0.0, f"per-element bound exceeded by {excess:.3e}"


@pytest.mark.parametrize("d", (1, 3, 17, 33, 300))
@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("self_mode", (False, True))
@pytest.mark.parametrize("p", (1, 2))
def test_forward_meets_the_per_element_bound(p, self_mode, n, m, d):
    A, B, _ = _inputs(n, m, d)
    if self_mode:
        X = _K().pairwise_pnorm(B.to(DEV), p=p)
        _check_forward(X, _direct(B.double(), B.double(), p), d)
        assert torch.equal(X, X.T) and not X.diagonal().any().item()
    else:
        X = _K().pairwise_pnorm(A.to(DEV), B.to(DEV), p=p, negate=True)
        _check_forward(-X, _direct(A.double(), B.double(), p), d)


@pytest.mark.parametrize("p", (1, 2))
def test_forward_unaligned_and_bf16(p):
    A, B, _ = _inputs(129, 257, 33)
    A, B = A[:, :32].contiguous(), B[:, :32].contiguous()
    flat = torch.empty(A.numel() + 1, device=DEV)
    odd = flat[1:].view_as(A).copy_(A)  # 4 bytes past a 16-byte boundary: rows load by element
    assert odd.data_ptr() % 16 == 4
    X64 = _direct(A.double(), B.double(), p)
    _check_forward(_K().pairwise_pnorm(odd, B.to(DEV), p=p), X64, 32)
    assert torch.equal(_K().pairwise_pnorm(odd, B.to(DEV), p=p), _K().pairwise_pnorm(A.to(DEV), B.to(DEV), p=p))
    Ab, Bb = A.bfloat16(), B.bfloat16()
    Xb = _K().pairwise_pnorm(Ab.to(DEV), Bb.to(DEV), p=p)
    assert Xb.dtype == torch.float32
    _check_forward(Xb, _direct(Ab.double(), Bb.double(), p), 32)


def test_offset_inputs_keep_near_pairs(monkeypatch):
    """A = 100 + 0.01 randn(129, 16): |a|^2 is ~1.6e5 and the squared distances ~3e-3.  The form
    |a|^2 + |b|^2 - 2ab that torch.cdist takes above 25 rows gave on this input (fp32, torch's CPU build, the
    same form as on the device): 62 % of the off-diagonal distances exactly 0, median relative error 1.0, worst
    6.5, diagonal entries up to 0.25, against a bound of 1.2e-6.  It is not asserted on.  The direct form
    meets the per-element bound, and through the module X is bitwise symmetric with an exactly zero diagonal."""
    from notorch_amd.nn.loss.rnc import PNorm

    gen = torch.Generator().manual_seed(5)
    A = 100 + 0.01 * torch.randn(129, 16, generator=gen)
    _check_forward(_K().pairwise_pnorm(A.to(DEV), p=2), _direct(A.double(), A.double(), 2), 16)
    monkeypatch.setenv("NT_PNORM", "kernel")
    X = PNorm(p=2, negate=True)(A.to(DEV))
    assert torch.equal(X, X.T) and not X.diagonal().any().item()
    _check_forward(-X, _direct(A.double(), A.double(), 2), 16)


def _grads(A, B, G, p, dtype):
    a = A.to(dtype).requires_grad_()
    b = None if B is None else B.to(dtype).requires_grad_()
    x = _direct(a, a if b is None else b, p)
    return torch.autograd.grad(x, [a] if b is None else [a, b], G.to(dtype))


def _rel(got, ref64):
    scale = ref64.abs().max().item()
    err = (got.double().cpu() - ref64).abs().max().item()
    return err / scale if scale > 0 else err


@pytest.mark.parametrize("d", (1, 17, 300))
@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("self_mode", (False, True))
@pytest.mark.parametrize("p", (1, 2))
def test_backward_matches_fp64_autograd(p, self_mode, n, m, d):
    A, B, G = _inputs(n, m, d)
    if self_mode:
        A, B, G = B, None, _inputs(m, m, d)[2]
    X = _K().pairwise_pnorm(A.to(DEV), None if B is None else B.to(DEV), p=p, negate=True)
    got = _K().pairwise_pnorm_backward(A.to(DEV), None if B is None else B.to(DEV), X, G.to(DEV), p=p, negate=True,
                                       want=("A",) if self_mode else ("A", "B"))
    ref64, ref32 = _grads(A, B, -G, p, torch.float64), _grads(A, B, -G, p, torch.float32)
    for name, g, r64, r32 in zip("AB", got, ref64, ref32):
        e, e32 = _rel(g, r64), _rel(r32, r64)
        print(f"PNORMERR d{name} p={p} self={self_mode} {n}x{m}x{d} kernel {e:.3e} cpu-fp32 {e32:.3e}")
        assert torch.isfinite(g).all().item()
        assert e <= 1e-5 and e <= 4 * e32


@pytest.mark.parametrize("p", (1, 2))
def test_duplicate_rows_contribute_exactly_zero(p):
    A, B, _ = _inputs(127, 129, 17)
    A, B = A.clone(), B.clone()
    A[5], B[3] = A[9], A[7]
    for a, b, pairs in ((A, None, ((5, 9), (9, 5))), (A, B, ((7, 3),))):
        ad, bd = a.to(DEV), None if b is None else b.to(DEV)
        X = _K().pairwise_pnorm(ad, bd, p=p)
        G = torch.zeros_like(X)
        for i, j in pairs:
            assert X[i, j].item() == 0.0
            G[i, j] = 1.0
        want = ("A",) if b is None else ("A", "B")
        for g in _K().pairwise_pnorm_backward(ad, bd, X, G, p=p, want=want)[: len(want)]:
            assert not g.any().item()  # finite, and exactly 0: only the equal pairs carry a gradient
        full = _K().pairwise_pnorm_backward(ad, bd, X, torch.ones_like(X), p=p, want=want)[: len(want)]
        assert all(torch.isfinite(g).all().item() for g in full)


def test_sign_of_zero_is_zero_on_integer_inputs():
    gen = torch.Generator().manual_seed(3)
    A = torch.randint(-2, 3, (129, 5), generator=gen).float()
    B = torch.randint(-2, 3, (67, 5), generator=gen).float()
    G = torch.randint(-4, 5, (129, 67), generator=gen).float()
    X = _K().pairwise_pnorm(A.to(DEV), B.to(DEV), p=1)
    assert torch.equal(X.cpu().double(), _direct(A.double(), B.double(), 1))
    got = _K().pairwise_pnorm_backward(A.to(DEV), B.to(DEV), X, G.to(DEV), p=1, want=("A", "B"))
    for g, r64 in zip(got, _grads(A, B, G, 1, torch.float64)):
        assert torch.equal(g.cpu().double(), r64)  # every term is a small integer: the sums are exact


@pytest.mark.parametrize("p", (1, 2))
def test_two_calls_return_the_same_bits(p):
    K = _K()
    A, B, G = (t.to(DEV) for t in _inputs(129, 257, 17))  # the backward splits j here
    for a, b, g, want in ((A, B, G, ("A", "B")), (B, None, _inputs(257, 257, 17)[2].to(DEV), ("A",))):
        X = K.pairwise_pnorm(a, b, p=p)
        assert torch.equal(X, K.pairwise_pnorm(a, b, p=p))
        first, second = (K.pairwise_pnorm_backward(a, b, X, g, p=p, want=want) for _ in range(2))
        assert all(torch.equal(u, v) for u, v in zip(first[: len(want)], second[: len(want)]))


def test_loss_on_the_kernel_route_matches_the_torch_route(monkeypatch):
    from notorch_amd.nn.loss import RankNContrastLoss

    n, temp, tol = 257, 2.0, 1e-5  # the inputs, scales and tolerance of tests/test_gpu_rnc.py
    gen = torch.Generator().manual_seed(1000 * n + len("distinct"))
    x, t = 0.5 * torch.randn(n, 8, generator=gen), torch.randn(n, 2, generator=gen)
    K = _K()
    real, calls = K.pairwise_pnorm_backward, []
    monkeypatch.setattr(K, "pairwise_pnorm_backward", lambda *a, **k: calls.append(k["want"]) or real(*a, **k))
    monkeypatch.delenv("NT_RNC", raising=False)
    crit = RankNContrastLoss(temp=temp)
    out = {}
    for knob in ("kernel", "torch"):
        monkeypatch.setenv("NT_PNORM", knob)
        xa = x.to(DEV).requires_grad_()
        loss = crit(xa, t.to(DEV))
        loss.backward()
        out[knob] = (loss.item(), xa.grad.double().cpu())
    assert calls == [("A",)]  # Sim's gradient, one self-mode pass; the label distance gets none
    (lk, gk), (lt, gt) = out["kernel"], out["torch"]
    assert abs(lk - lt) <= tol * max(1.0, abs(lt))
    assert (gk - gt).abs().max().item() <= tol * max(gt.abs().max().item(), 1.0 / (temp * n * (n - 1)))
    monkeypatch.setenv("NT_PNORM", "kernel")
    with torch.no_grad():
        quiet = crit(x.to(DEV).requires_grad_(), t.to(DEV))
    assert calls == [("A",)] and quiet.item() == lk
