"""CPU: notorch_amd.nn.loss.RankNContrastLoss against a literal evaluation of the loss.

The literal form below is the definition, written out with the N x N x N mask: for every ordered pair
(i, j), the scores s[i, k] of all k with D[i, k] >= D[i, j] are scatter-summed into denom[i, j], EPS is
added, and -log(s[i, j] / denom[i, j]) is averaged over the pairs with i != j.  The module's torch route
(a sort and two scans per row, O(N^2) memory) must agree with it in fp64 to 1e-12, loss and gradient,
with distinct targets, heavily tied targets and all targets equal.  On the CPU the module never reaches
the kernel, whatever NT_RNC says."""
import math

import pytest
import torch

SIZES = (2, 3, 17, 64)
TARGETS = ("distinct", "ties", "equal")
TOL = 1e-12


def _loss_mod():
    from notorch_amd.nn import loss

    return loss


def _targets(kind, n, gen):
    if kind == "distinct":
        return torch.randn(n, 2, generator=gen, dtype=torch.float64)
    if kind == "ties":
        return torch.randint(0, 3, (n, 1), generator=gen).double()
    return torch.full((n, 1), 0.75, dtype=torch.float64)


def literal_loss(sim, dist, temp, eps):
    """mean over i != j of -log(s_ij / (eps + sum_{k: D_ik >= D_ij} s_ik)), via the triple mask."""
    n = sim.shape[0]
    s = torch.exp(sim / temp)
    mask = dist[:, None, :] >= dist[:, :, None]  # [i, j, k]: D[i, k] >= D[i, j]
    i, j, k = mask.nonzero(as_tuple=True)
    denom = torch.zeros(n * n, dtype=sim.dtype).index_add(0, i * n + j, s[i, k]).view(n, n) + eps
    off = ~torch.eye(n, dtype=torch.bool)
    return -torch.log(s / denom)[off].mean()


def _literal_from_inputs(x, t, temp, eps, mode="use_mm_for_euclid_dist_if_necessary"):
    return literal_loss(-torch.cdist(x, x, p=2, compute_mode=mode), torch.cdist(t, t, p=1), temp, eps)


EXACT = "donot_use_mm_for_euclid_dist"


@pytest.mark.parametrize("kind", TARGETS)
@pytest.mark.parametrize("n", SIZES)
def test_module_matches_the_literal_form_in_fp64(n, kind):
    """Loss, dLoss/dSim (diagonal included) and inputs.grad at 1e-12, targets.grad None or zero.

    inputs.grad is compared through the direct form of torch.cdist on both sides.  Above 25 rows the default
    torch.cdist takes its matmul form, whose diagonal is ~1e-8 instead of 0 and whose backward multiplies
    dSim[i, i] (non-zero under ties) by 1 / (2 * that): the 6e-19 by which the two forms' dSim differ at
    N = 64 comes out as 1.8e-12 in inputs.grad, whatever the loss code does (measured: ties and equal
    targets at N = 64; 3e-18 with the direct form).  With the default PNorms the same 1e-12 is asserted on
    what the loss itself returns: the value and dLoss/dSim."""
    L = _loss_mod()

    class DirectPNorm(L.PNorm):
        def forward(self, A, B=None):
            X = torch.cdist(A, A if B is None else B, p=self.p, compute_mode=EXACT)
            return X.neg() if self.negate else X

    gen = torch.Generator().manual_seed(100 * n + len(kind))
    x = torch.randn(n, 5, generator=gen, dtype=torch.float64)
    t = _targets(kind, n, gen)

    # the default module: value and gradient with respect to Sim
    crit = L.RankNContrastLoss()
    kept = []

    def keep(mod, args, out):  # Sim is no leaf: keep its gradient
        out.retain_grad()
        kept.append(out)

    crit.similarity.register_forward_hook(keep)
    xa, ta = x.clone().requires_grad_(), t.clone().requires_grad_()
    got = crit(xa, ta)
    got.backward()
    sb = (-torch.cdist(x, x, p=2)).requires_grad_()
    want = literal_loss(sb, torch.cdist(t, t, p=1), crit.temp, crit.EPS)
    want.backward()
    assert got.dtype == torch.float64 and got.dim() == 0
    assert abs(got.item() - want.item()) <= TOL
    assert (kept[0].grad - sb.grad).abs().max().item() <= TOL
    assert ta.grad is None or ta.grad.abs().max().item() == 0.0

    # inputs.grad, through the direct cdist on both sides
    crit = L.RankNContrastLoss(similarity=DirectPNorm(p=2, negate=True))
    xa, ta = x.clone().requires_grad_(), t.clone().requires_grad_()
    got = crit(xa, ta)
    got.backward()
    xb = x.clone().requires_grad_()
    want = _literal_from_inputs(xb, t, crit.temp, crit.EPS, EXACT)
    want.backward()
    assert abs(got.item() - want.item()) <= TOL
    assert (xa.grad - xb.grad).abs().max().item() <= TOL
    assert ta.grad is None or ta.grad.abs().max().item() == 0.0


@pytest.mark.parametrize("kind", ("ties", "equal"))
def test_gradient_with_respect_to_sim_has_a_diagonal_under_ties(kind):
    """k = i is inside the sum of every j whose target equals the anchor's, so dL/dSim[i, i] != 0."""
    from notorch_amd.nn.loss.rnc import rank_loss_torch

    n = 17
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(n, 5, generator=gen, dtype=torch.float64)
    t = _targets(kind, n, gen)
    dist = torch.cdist(t, t, p=1)
    sa = (-torch.cdist(x, x, p=2)).requires_grad_()
    sb = sa.detach().clone().requires_grad_()
    rank_loss_torch(sa, dist, 2.0, 1e-6).backward()
    literal_loss(sb, dist, 2.0, 1e-6).backward()
    assert (sa.grad - sb.grad).abs().max().item() <= TOL
    diag = sa.grad.diagonal()
    assert diag.abs().min().item() > 0.0 if kind == "equal" else diag.abs().max().item() > 0.0
    # the closed form: (s_ik T_ik - [k != i]) / (temp M), T_ik = sum_{j != i, D_ij <= D_ik} 1 / denom_ij
    s = torch.exp(sa.detach() / 2.0)
    denom = ((dist[:, None, :] >= dist[:, :, None]) * s[:, None, :]).sum(-1) + 1e-6
    off = ~torch.eye(n, dtype=torch.bool)
    T = ((dist[:, :, None] <= dist[:, None, :]) * (off / denom)[:, :, None]).sum(1)  # [i, k], summed over j
    closed = (s * T - off.double()) / (2.0 * n * (n - 1))
    assert (sa.grad - closed).abs().max().item() <= TOL


def test_one_sample_gives_nan():
    L = _loss_mod()
    out = L.RankNContrastLoss()(torch.randn(1, 4), torch.randn(1, 1))
    assert out.dim() == 0 and math.isnan(out.item())


def test_loss_stays_finite_where_the_scores_underflow():
    """Fingerprints 1000 apart: s = exp(-500) is 0 in fp32, the literal log(s / denom) is inf; the module
    evaluates log denom - Sim / temp."""
    L = _loss_mod()
    x = torch.tensor([[0.0, 0.0], [1000.0, 0.0], [0.0, 1000.0]])
    t = torch.tensor([[0.0], [1.0], [3.0]])
    crit = L.RankNContrastLoss()
    assert math.isinf(_literal_from_inputs(x, t, crit.temp, crit.EPS).item())
    got = crit(x, t)
    assert torch.isfinite(got).item()
    # denom = EPS everywhere (every score is 0): each term is log EPS + d / temp
    d = torch.cdist(x, x, p=2).double()
    want = (math.log(1e-6) + d[~torch.eye(3, dtype=torch.bool)] / 2.0).mean().item()
    assert abs(got.item() - want) <= 1e-4 * abs(want)


def test_custom_distance_and_similarity_are_honoured():
    L = _loss_mod()

    class Dot(L.CDist):
        def forward(self, A, B=None):
            return A @ (A if B is None else B).T

    gen = torch.Generator().manual_seed(3)
    x = torch.randn(9, 4, generator=gen, dtype=torch.float64)
    t = torch.randn(9, 3, generator=gen, dtype=torch.float64)
    crit = L.RankNContrastLoss(distance=L.PNorm(p=2.0), similarity=Dot(), temp=0.5)
    assert isinstance(crit.distance, L.PNorm) and isinstance(crit.similarity, Dot)
    want = literal_loss(x @ x.T, torch.cdist(t, t, p=2), 0.5, crit.EPS)
    assert abs(crit(x, t).item() - want.item()) <= TOL
    assert abs(crit(x, t).item() - L.RankNContrastLoss()(x, t).item()) > 1e-3  # and they matter


def test_defaults_and_repr():
    L = _loss_mod()
    crit = L.RankNContrastLoss()
    assert L.RankNContrastLoss.EPS == 1e-6 and crit.temp == 2.0
    assert (crit.distance.p, crit.distance.negate) == (1, False)
    assert (crit.similarity.p, crit.similarity.negate) == (2, True)
    assert crit.extra_repr() == "(temp): 2.0"
    assert L.PNorm().extra_repr() == "p=2.0, negate=False"
    assert L.PNorm(p=1, negate=True).extra_repr() == "p=1.0, negate=True"
    rep = repr(crit)
    assert "(distance): PNorm(p=1.0, negate=False)" in rep
    assert "(similarity): PNorm(p=2.0, negate=True)" in rep and "(temp): 2.0" in rep
    assert issubclass(L.PNorm, L.CDist) and issubclass(L.CDist, torch.nn.Module)


@pytest.mark.parametrize("knob", (None, "torch", "kernel"))
def test_cpu_tensors_take_the_torch_route(monkeypatch, knob):
    from notorch_amd import kernels as K

    L = _loss_mod()

    def _fail(*a, **k):
        raise AssertionError("a CPU tensor reached the kernel binding")

    monkeypatch.setattr(K, "rnc_rank", _fail)
    monkeypatch.setattr(K, "rnc_max_n", _fail)
    if knob is None:
        monkeypatch.delenv("NT_RNC", raising=False)
    else:
        monkeypatch.setenv("NT_RNC", knob)
    gen = torch.Generator().manual_seed(5)
    x, t = torch.randn(12, 4, generator=gen), torch.randn(12, 1, generator=gen)
    got = L.RankNContrastLoss()(x, t)
    want = _literal_from_inputs(x.double(), t.double(), 2.0, 1e-6)
    assert got.dtype == torch.float32 and abs(got.item() - want.item()) <= 1e-5
