"""GPU: RankNContrastLoss above 4096 rows on nt_rnc_rank_long (csrc/rnc_long.hip), up to N = 16384.

Inputs are those of tests/test_gpu_rnc.py: X = 0.5 randn(N, 8) at temp 2.0, targets "distinct" / "five" /
"equal", Sim and D from the default PNorms.  The yardstick is the sorted formulation in fp64 on the device,
evaluated per block of <= 1024 rows (rows are independent: loss = sum of the rows / (N (N - 1))), so that no
fp64 N x N set larger than a block exists at N = 16384; the block helper is first tied to rank_loss_torch in
fp64 at N = 257.  The criterion is the project's fp32 contract, as in tests/test_gpu_rnc.py:
    |L - L64| <= 1e-5 max(1, |L64|)
    max|dSim - dSim64| <= 1e-5 max(max|dSim64|, 1 / (temp N (N - 1)))
Every case prints ``RNCERR <class> <value> <case>``."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
TEMP, EPS, TOL = 2.0, 1e-6, 1e-5
BLOCK = 1024
# (N, targets): degenerate scans, the wave edge and tie groups that cross threads on the smallest P; the first
# N the module sends here (by element); a full P on the 8-position instance with 16-byte rows, groups of
# ~1600 and one group of N (k = i inside every sum); the first n on the 16-position instance (by element);
# a full P on the 16-position instance
CASES = ((2, "distinct"), (65, "distinct"), (1000, "five"), (4097, "distinct"), (8192, "five"), (8192, "equal"),
         (8193, "distinct"), (16384, "five"))


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


def _sim_dist(n, kind):
    """Sim, D (fp32, on the device, from the default PNorms)."""
    x, t = _inputs(n, kind)
    crit = _L().RankNContrastLoss()
    with torch.no_grad():
        return crit.similarity(x.to(DEV)).contiguous(), crit.distance(t.to(DEV)).contiguous()


_case = functools.lru_cache(maxsize=None)(_sim_dist)  # the cases that several tests share; never written to


def _block64(sim, dist, r0, r1):
    """The sorted formulation in fp64 for the anchor rows r0 .. r1 - 1 of the n x n problem: the sum of the
    rows' nll and its gradient with respect to sim[r0:r1] (both before the division by N (N - 1))."""
    n, b = sim.shape[1], r1 - r0
    s = sim[r0:r1].double().requires_grad_()
    logits = s / TEMP
    d_sorted, order = torch.sort(dist[r0:r1].double(), dim=1, descending=True, stable=True)
    csum = logits.exp().gather(1, order).cumsum(1)
    pos = torch.arange(n, device=sim.device).expand(b, n)
    ends = torch.ones(b, n, dtype=torch.bool, device=sim.device)
    ends[:, :-1] = d_sorted[:, 1:] != d_sorted[:, :-1]
    group_end = torch.where(ends, pos, n - 1).flip(1).cummin(1).values.flip(1)
    denom = torch.empty_like(csum).scatter(1, order, csum.gather(1, group_end) + EPS)
    nll = denom.log() - logits
    own = torch.zeros(b, n, dtype=torch.bool, device=sim.device)
    own[torch.arange(b, device=sim.device), torch.arange(r0, r1, device=sim.device)] = True
    total = nll.masked_fill(own, 0.0).sum()
    (g,) = torch.autograd.grad(total, s)
    return total, g


def _grad_floor(n):
    return 1.0 / (TEMP * n * (n - 1))


def _errors(sim, dist, outputs, block=BLOCK):
    """One pass over the fp64 blocks for every (row_nll, dsim) in outputs: L64, max|dSim64| and per output
    (|L - L64| / max(1, |L64|), max|dSim - dSim64| / max(max|dSim64|, floor))."""
    n = sim.shape[0]
    pairs = n * (n - 1)
    total = torch.zeros((), dtype=torch.float64, device=sim.device)
    gmax = torch.zeros((), dtype=torch.float64, device=sim.device)
    diff = [torch.zeros((), dtype=torch.float64, device=sim.device) for _ in outputs]
    for r0 in range(0, n, block):
        r1 = min(n, r0 + block)
        t, g = _block64(sim, dist, r0, r1)
        g = g / pairs
        total += t
        gmax = torch.maximum(gmax, g.abs().max())
        for i, (_, dsim) in enumerate(outputs):
            diff[i] = torch.maximum(diff[i], (dsim[r0:r1].double() - g).abs().max())
    l64, gmax = (total / pairs).item(), gmax.item()
    errs = []
    for (row_nll, _), d in zip(outputs, diff):
        loss = (row_nll.sum() / pairs).item()  # fp32, as RnCRankLongFunction reduces it
        errs.append((abs(loss - l64) / max(1.0, abs(l64)), d.item() / max(gmax, _grad_floor(n))))
    return l64, gmax, errs


def test_block_yardstick_is_the_fp64_torch_route():
    from notorch_amd.nn.loss.rnc import rank_loss_torch

    n = 257
    for kind in ("distinct", "five"):
        sim, dist = _sim_dist(n, kind)
        s64 = sim.double().requires_grad_()
        ref = rank_loss_torch(s64, dist.double(), TEMP, EPS)
        (gref,) = torch.autograd.grad(ref, s64)
        fake = (torch.zeros(n, device=DEV), torch.zeros(n, n, device=DEV))  # dSim = 0: diff = |dSim64|
        l64, gmax, _ = _errors(sim, dist, [fake], block=100)  # three blocks, the last one short
        assert abs(l64 - ref.item()) <= 1e-12 * max(1.0, abs(ref.item()))
        assert abs(gmax - gref.abs().max().item()) <= 1e-12 * gref.abs().max().item()
        worst = 0.0
        for r0 in range(0, n, 100):
            r1 = min(n, r0 + 100)
            _, g = _block64(sim, dist, r0, r1)
            worst = max(worst, (g / (n * (n - 1)) - gref[r0:r1]).abs().max().item())
        _report("yardstick", worst / gref.abs().max().item(), f"N={n} {kind} blocks of 100 vs rank_loss_torch fp64")
        assert worst <= 1e-12 * max(gref.abs().max().item(), _grad_floor(n))


@pytest.mark.parametrize("n,kind", CASES)
def test_long_kernel_matches_the_fp64_blocks(n, kind):
    K = _K()
    sim, dist = _sim_dist(n, kind) if n > 8192 else _case(n, kind)
    row_nll, dsim = K.rnc_rank_long(sim, dist, TEMP, EPS, True)
    assert row_nll.dtype == torch.float32 and row_nll.shape == (n,) and dsim.shape == (n, n)
    l64, gmax, ((e_loss, e_grad),) = _errors(sim, dist, [(row_nll, dsim)])
    _report("loss", e_loss, f"N={n} {kind} L64={l64:.6f}")
    _report("dsim", e_grad, f"N={n} {kind} max|dSim64|={gmax:.3e}")
    assert e_loss <= TOL
    assert e_grad <= TOL
    if kind != "distinct":  # k = i is inside the sums of the anchor's duplicates
        assert dsim.diagonal().abs().max().item() > 0.0


def test_both_kernels_meet_the_criterion_where_both_reach():
    K = _K()
    n, kind = 1000, "five"
    sim, dist = _case(n, kind)
    outs = [K.rnc_rank_long(sim, dist, TEMP, EPS, True), K.rnc_rank(sim, dist, TEMP, EPS, True)]
    _, _, errs = _errors(sim, dist, outs)
    for name, (e_loss, e_grad) in zip(("rnc_rank_long", "rnc_rank"), errs):
        _report("loss", e_loss, f"N={n} {kind} {name}")
        _report("dsim", e_grad, f"N={n} {kind} {name}")
        assert e_loss <= TOL and e_grad <= TOL


def test_two_calls_return_the_same_bits():
    K = _K()
    for n, kind in ((4097, "distinct"), (8192, "five")):
        sim, dist = _case(n, kind)
        a_nll, a_g = K.rnc_rank_long(sim, dist, TEMP, EPS, True)
        b_nll, b_g = K.rnc_rank_long(sim, dist, TEMP, EPS, True)
        assert torch.equal(a_nll, b_nll) and torch.equal(a_g, b_g)
        assert torch.isfinite(a_nll).all().item() and torch.isfinite(a_g).all().item()


@pytest.fixture
def calls(monkeypatch):
    """Count the launches of K.rnc_rank_long and K.rnc_rank: (entry, need_grad, dsim is None) of each."""
    K = _K()
    seen = []

    def counting(name):
        real = getattr(K, name)

        def counted(sim, dist, temp, eps, need_grad):
            out = real(sim, dist, temp, eps, need_grad)
            seen.append((name, bool(need_grad), out[1] is None))
            return out

        monkeypatch.setattr(K, name, counted)

    counting("rnc_rank_long")
    counting("rnc_rank")
    return seen


def test_end_to_end_at_4097_matches_the_device_torch_route(calls, monkeypatch):
    n = 4097
    x, t = _inputs(n, "distinct")
    crit = _L().RankNContrastLoss().to(DEV)
    grads, losses = [], []
    for knob in ("kernel", "torch"):  # NT_RNC=kernel: the test does not depend on the measured default
        monkeypatch.setenv("NT_RNC", knob)
        xa = x.to(DEV).requires_grad_()
        loss = crit(xa, t.to(DEV))
        loss.backward()
        grads.append(xa.grad.double().cpu())
        losses.append(loss.item())
    assert calls == [("rnc_rank_long", True, False)]  # one launch of the long kernel, none of the short one
    e_loss = abs(losses[0] - losses[1]) / max(1.0, abs(losses[1]))
    e_grad = (grads[0] - grads[1]).abs().max().item() / max(grads[1].abs().max().item(), _grad_floor(n))
    _report("loss_e2e", e_loss, f"N={n} vs the device torch route")
    _report("dinputs", e_grad, f"N={n} vs the device torch route")
    assert e_loss <= TOL and e_grad <= TOL


def test_no_grad_allocates_no_gradient_buffer(calls, monkeypatch):
    monkeypatch.setenv("NT_RNC", "kernel")
    x, t = _inputs(4097, "distinct")
    x, t = x.to(DEV), t.to(DEV)
    crit = _L().RankNContrastLoss()
    with_grad = crit(x.clone().requires_grad_(), t)
    with torch.no_grad():
        without = crit(x.clone().requires_grad_(), t)
    plain = crit(x, t)  # nothing requires a gradient
    assert calls == [("rnc_rank_long", True, False), ("rnc_rank_long", False, True), ("rnc_rank_long", False, True)]
    assert torch.equal(with_grad, without) and torch.equal(with_grad, plain)
    assert with_grad.requires_grad and not without.requires_grad
