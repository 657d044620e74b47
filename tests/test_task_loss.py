"""CPU: the torch route of notorch_amd.nn.loss / notorch_amd.nn.metrics in fp64 against the literal formulas.

The literal forms below restate notorch/nn/loss/loss.py and notorch/nn/metrics.py element by element, with the
reduction the reference evidently means: every element is L[i, j] * w[i]; without a mask the result is the
mean over b t, with one it is sum(L w mask) / sum(mask).  Loss and preds.grad must agree to 1e-12.  AUROC is
held to the O(n^2) pairwise definition (greater-than plus half the ties), average precision to the
per-threshold definition.  On the CPU no module reaches the kernel, whatever NT_LOSS says."""
import math

import pytest
import torch
import torch.nn.functional as F

TOL = 1e-12
SHAPES = ((1, 1), (5, 3), (64, 1))
F64 = torch.float64


def _loss():
    from notorch_amd.nn import loss

    return loss


def _metrics():
    from notorch_amd.nn import metrics

    return metrics


# ------------------------------------------------------------------ literal element losses (b x t)
def lit_mse(p, y):
    return (p - y) ** 2


def lit_mae(p, y):
    return (p - y).abs()


def lit_rmse(p, y):
    return ((p - y) ** 2).sqrt()


def lit_bce(p, y):
    return F.binary_cross_entropy_with_logits(p, y, reduction="none")


def lit_mve(p, y):
    mean, var = p[..., 0], p[..., 1]
    return (mean - y) ** 2 / (2 * var) + (2 * math.pi * var).log() / 2


def lit_evidential(p, y, v_kl=0.2, eps=1e-8):
    mean, v, alpha, beta = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    res = y - mean
    two_b_lambda = 2 * beta * (1 + v)
    nll = (0.5 * (math.pi / v).log() - alpha * two_b_lambda.log()
           + (alpha + 0.5) * torch.log(v * res ** 2 + two_b_lambda) + torch.lgamma(alpha) - torch.lgamma(alpha + 0.5))
    return nll + v_kl * ((2 * v + alpha) * res.abs() - eps)


def lit_xent(p, y):
    return F.cross_entropy(p.transpose(1, 2), y.long(), reduction="none")


def lit_dirichlet(p, y, k, v_kl=0.2):
    alphas = F.softplus(p) + 1
    onehot = F.one_hot(y.long(), num_classes=k)
    S = alphas.sum(-1, keepdim=True)
    probs = alphas / S
    L_mse = (onehot - probs).square().sum(-1) + ((probs * (1 - probs)) / (S + 1)).sum(-1)
    alpha_t = onehot + (1 - onehot) * alphas
    beta = torch.ones_like(alpha_t)
    ln_alpha = alpha_t.sum(-1).lgamma() - alpha_t.lgamma().sum(-1)
    ln_beta = beta.lgamma().sum(-1) - beta.sum(-1).lgamma()
    dg = torch.digamma(alpha_t) - torch.digamma(alpha_t.sum(-1)).unsqueeze(-1)
    return L_mse + v_kl * (ln_alpha + ln_beta + ((alpha_t - beta) * dg).sum(-1))


def lit_reduce(L, mask, w):
    if w is not None:
        L = L * w[:, None]
    return L.mean() if mask is None else (L * mask).sum() / mask.sum()


def lit_clamp(p, y, lt, gt):
    p = torch.where((p < y) & lt, y, p)
    return torch.where((p > y) & gt, y, p)


def _sp(gen, *shape):
    return F.softplus(torch.randn(*shape, generator=gen, dtype=F64))


def _case(name, b, t, gen):
    """(module, literal element loss, preds, targets) in fp64."""
    L, M = _loss(), _metrics()
    y = torch.randn(b, t, generator=gen, dtype=F64)
    p1 = torch.randn(b, t, generator=gen, dtype=F64)
    if name == "mse":
        return L.MSE(), lit_mse, p1, y
    if name == "mae":
        return M.MAE(), lit_mae, p1, y
    if name == "rmse":
        return M.RMSE(), lit_rmse, p1, y
    if name == "bce":
        return L.BCE(), lit_bce, p1, (y > 0).to(F64)
    if name == "mve":
        return L.MVE(), lit_mve, torch.stack([p1, _sp(gen, b, t) + 0.1], -1), y
    if name == "evidential":
        p = torch.stack([p1, _sp(gen, b, t) + 0.1, _sp(gen, b, t) + 1, _sp(gen, b, t) + 0.1], -1)
        return L.Evidential(), lit_evidential, p, y
    if name == "xent":
        return L.XENT(), lit_xent, torch.randn(b, t, 4, generator=gen, dtype=F64), \
            torch.randint(0, 4, (b, t), generator=gen).to(F64)
    if name == "dirichlet2":
        return L.Dirichlet(), lambda p, y: lit_dirichlet(p, y, 2), torch.randn(b, t, 2, generator=gen, dtype=F64), \
            torch.randint(0, 2, (b, t), generator=gen).to(F64)
    assert name == "dirichlet3"
    return L.Dirichlet(), lambda p, y: lit_dirichlet(p, y, 3), torch.randn(b, t, 3, generator=gen, dtype=F64), \
        torch.randint(0, 3, (b, t), generator=gen).to(F64)


def _mask_weights(b, t, masked, weighted, gen):
    mask = None
    if masked:
        mask = torch.rand(b, t, generator=gen) < 0.6
        mask[0, 0] = True
    w = torch.rand(b, generator=gen, dtype=F64) + 0.5 if weighted else None
    return mask, w


def _both(mod, lit, p, y, mask, w, **bounds):
    """(loss, grad) of the module and of the literal form."""
    out = []
    for fn in (lambda q: mod(q, y, mask=mask, sample_weights=w, **bounds),
               lambda q: lit_reduce(lit(lit_clamp(q, y, bounds["lt_mask"], bounds["gt_mask"]) if bounds else q, y),
                                    mask, w)):
        q = p.clone().requires_grad_()
        loss = fn(q)
        (g,) = torch.autograd.grad(loss, q)
        out.append((loss, g))
    return out


KINDS = ("mse", "mae", "rmse", "bce", "mve", "evidential", "xent", "dirichlet2", "dirichlet3")


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("b,t", SHAPES)
@pytest.mark.parametrize("name", KINDS)
def test_torch_route_matches_the_literal_form_in_fp64(name, b, t, masked, weighted, monkeypatch):
    monkeypatch.setenv("NT_LOSS", "kernel")  # CPU tensors never reach the kernel
    gen = torch.Generator().manual_seed(1000 * b + 10 * t + len(name))
    mod, lit, p, y = _case(name, b, t, gen)
    mask, w = _mask_weights(b, t, masked, weighted, gen)
    (loss, g), (loss_l, g_l) = _both(mod, lit, p, y, mask, w)
    assert loss.dim() == 0 and loss.dtype == F64  # a scalar at t = 1 and at t = 3, with and without weights
    assert abs(loss.item() - loss_l.item()) <= TOL * max(1.0, abs(loss_l.item()))
    assert (g - g_l).abs().max().item() <= TOL * max(1.0, g_l.abs().max().item())


@pytest.mark.parametrize("t", (1, 3))
def test_sample_weights_scale_rows(t):
    b = 6
    gen = torch.Generator().manual_seed(t)
    p, y = torch.randn(b, t, generator=gen, dtype=F64), torch.randn(b, t, generator=gen, dtype=F64)
    w = torch.tensor([0.0, 1.0, 2.0, 0.5, 3.0, 1.5], dtype=F64)
    loss = _loss().MSE()(p, y, sample_weights=w)
    assert loss.shape == ()
    want = sum(w[i] * (p[i, j] - y[i, j]) ** 2 for i in range(b) for j in range(t)) / (b * t)
    assert abs(loss.item() - want.item()) <= TOL
    # row 0 has weight 0: its predictions do not matter
    p2 = p.clone()
    p2[0] += 100.0
    assert torch.equal(_loss().MSE()(p2, y, sample_weights=w), loss)


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("b,t", SHAPES)
@pytest.mark.parametrize("name", ("BoundedMSE", "BoundedMAE", "BoundedRMSE"))
def test_bounded_losses_run_and_clamped_elements_get_zero_gradient(name, b, t, masked, weighted):
    gen = torch.Generator().manual_seed(100 * b + t + len(name))
    mod = getattr(_loss(), name)() if name == "BoundedMSE" else getattr(_metrics(), name)()
    lit = {"BoundedMSE": lit_mse, "BoundedMAE": lit_mae, "BoundedRMSE": lit_rmse}[name]
    p, y = torch.randn(b, t, generator=gen, dtype=F64), torch.randn(b, t, generator=gen, dtype=F64)
    lt, gt = torch.rand(b, t, generator=gen) < 0.5, torch.rand(b, t, generator=gen) < 0.5
    if b * t > 1:  # one element clamped from below for sure, one from above
        p[0, 0], lt[0, 0] = y[0, 0] - 1.0, True
        p[-1, -1], gt[-1, -1] = y[-1, -1] + 1.0, True
    mask, w = _mask_weights(b, t, masked, weighted, gen)
    q = p.clone().requires_grad_()
    loss = mod(q, y, mask=mask, sample_weights=w, lt_mask=lt, gt_mask=gt)
    (g,) = torch.autograd.grad(loss, q)
    clamped = ((p < y) & lt) | ((p > y) & gt)
    assert torch.isfinite(g).all().item()
    assert b * t == 1 or clamped.sum().item() >= 2
    assert (g[clamped] == 0).all().item()
    free = ~clamped if mask is None else ~clamped & mask
    assert (g[free] != 0).all().item()
    want = lit_reduce(lit(lit_clamp(p, y, lt, gt), y), mask, w)
    assert abs(loss.item() - want.item()) <= TOL * max(1.0, abs(want.item()))
    if name == "BoundedMSE":  # the literal gradient is finite here too (sqrt and abs are not, at 0)
        (_, _), (_, g_l) = _both(mod, lit, p, y, mask, w, lt_mask=lt, gt_mask=gt)
        assert (g - g_l).abs().max().item() <= TOL * max(1.0, g_l.abs().max().item())


def test_bounded_needs_its_masks():
    p = torch.zeros(2, 2, dtype=F64)
    with pytest.raises(TypeError):
        _loss().BoundedMSE()(p, p)


@pytest.mark.parametrize("name", ("mse", "mve", "xent", "dirichlet2"))
def test_all_false_mask_gives_nan(name):
    gen = torch.Generator().manual_seed(5)
    mod, _, p, y = _case(name, 5, 3, gen)
    out = mod(p, y, mask=torch.zeros(5, 3, dtype=torch.bool))
    assert out.dim() == 0 and torch.isnan(out).item()


def test_names_aliases_and_reprs():
    L, M = _loss(), _metrics()
    assert L.BCE is L.BinaryCrossEntropy and L.XENT is L.CrossEntropy and L.MVE is L.MeanVarianceEstimation
    assert repr(L.Evidential()) == "Evidential(v_kl=0.2, eps=1.0e-08)"
    assert repr(L.Dirichlet(0.5)) == "Dirichlet(v_kl=0.5)"
    assert repr(M.AUROC("binary")) == "AUROC(task=binary)"
    assert repr(M.F1("binary")) == "F1(task=binary, threshold=0.5)"
    assert repr(M.Accuracy("multilabel", 0.3)) == "Accuracy(task=multilabel, threshold=0.3)"
    s = torch.tensor(2.0)
    assert L.SelfSupervisedLoss()(s) is s
    with pytest.raises(ValueError):
        L.SelfSupervisedLoss()(torch.zeros(2))
    for cls in (M.MAE, M.RMSE, M.BoundedMAE, M.BoundedRMSE, M.R2):
        assert isinstance(cls(), torch.nn.Module)


# ------------------------------------------------------------------ R2, Accuracy, F1
def test_r2_literal_with_and_without_weights_and_mask():
    gen = torch.Generator().manual_seed(3)
    b, t = 12, 3
    p, y = torch.randn(b, t, generator=gen, dtype=F64), torch.randn(b, t, generator=gen, dtype=F64)
    w = torch.rand(b, generator=gen, dtype=F64) + 0.5
    mask = torch.rand(b, t, generator=gen) < 0.7

    def lit(w_, m_):
        means = (w_[:, None] * y).mean(0, keepdim=True)
        rss = torch.sum(w_[:, None] * (p - y).square() * m_, dim=0)
        tss = torch.sum(w_[:, None] * (y - means).square() * m_, dim=0)
        return (1 - rss / tss).mean(0)

    ones_w, ones_m = torch.ones(b, dtype=F64), torch.ones(b, t, dtype=F64)
    R2 = _metrics().R2()
    assert abs(R2(p, y).item() - lit(ones_w, ones_m).item()) <= TOL
    assert abs(R2(p, y, mask=mask, sample_weights=w).item() - lit(w, mask.to(F64)).item()) <= TOL
    assert abs(R2(p, y, sample_weights=w).item() - lit(w, ones_m).item()) <= TOL
    assert R2(y, y).item() == 1.0


def test_accuracy_and_f1():
    M = _metrics()
    p = torch.tensor([[0.9, 0.2], [0.6, 0.7], [0.1, 0.8], [0.4, 0.3]], dtype=F64)
    y = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.0, 1.0]], dtype=F64)
    mask = torch.tensor([[True, True], [True, True], [True, False], [True, True]])
    # hard = [[1,0],[1,1],[0,1],[0,0]]; correct = [[1,1],[0,1],[0,1],[1,0]]
    assert abs(M.Accuracy("binary")(p, y).item() - 5 / 8) <= TOL
    assert abs(M.Accuracy("binary")(p, y, mask=mask).item() - 4 / 7) <= TOL
    logits = torch.tensor([[[0.1, 2.0, 0.3]], [[1.5, 0.2, 0.1]], [[0.0, 0.1, 0.9]]], dtype=F64)
    cls = torch.tensor([[1.0], [0.0], [1.0]], dtype=F64)
    assert abs(M.Accuracy("multilabel")(logits, cls).item() - 2 / 3) <= TOL
    # binary F1 from the pooled counts: TP = 3 (0,0; 1,1; 2,1), FP = 1 (1,0), FN = 2 (2,0; 3,1)
    assert abs(M.F1("binary")(p, y).item() - 6 / 9) <= TOL
    # masked (2,1) drops one TP
    assert abs(M.F1("binary")(p, y, mask=mask).item() - 4 / 7) <= TOL
    # per column: col 0 TP 1 FP 1 FN 1 -> 0.5; col 1 TP 2 FP 0 FN 1 -> 0.8
    assert abs(M.F1("multilabel")(p, y).item() - 0.65) <= TOL
    assert M.F1("binary")(torch.zeros(3, 1, dtype=F64), torch.zeros(3, 1, dtype=F64)).item() == 0.0


# ------------------------------------------------------------------ AUROC / AUPRC
def pairwise_auroc(s, y, keep):
    pos, neg = s[keep & (y == 1)], s[keep & (y == 0)]
    if len(pos) == 0 or len(neg) == 0:
        return float("nan")
    gt = (pos[:, None] > neg[None, :]).sum().item()
    eq = (pos[:, None] == neg[None, :]).sum().item()
    return (gt + 0.5 * eq) / (len(pos) * len(neg))


def threshold_ap(s, y, keep):
    s, y = s[keep], y[keep]
    P, N = int((y == 1).sum()), int((y == 0).sum())
    if P == 0 or N == 0:
        return float("nan")
    ap, recall_before = 0.0, 0.0
    for thr in sorted(set(s.tolist()), reverse=True):
        sel = s >= thr
        tp, fp = int((sel & (y == 1)).sum()), int((sel & (y == 0)).sum())
        ap += (tp / P - recall_before) * tp / (tp + fp)
        recall_before = tp / P
    return ap


def _scores(kind, n, t, gen):
    if kind == "distinct":
        return torch.randn(n, t, generator=gen, dtype=F64)
    if kind == "five":
        return torch.randint(0, 5, (n, t), generator=gen).to(F64) / 4 - 0.5  # -0.5 .. 0.5, with a 0
    return torch.full((n, t), 0.25, dtype=F64)


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("kind", ("distinct", "five", "equal"))
@pytest.mark.parametrize("n,t", ((2, 1), (17, 3), (64, 1), (200, 2)))
def test_rank_metrics_match_the_pairwise_and_threshold_definitions(n, t, kind, masked):
    M = _metrics()
    gen = torch.Generator().manual_seed(7 * n + t + len(kind))
    s = _scores(kind, n, t, gen)
    if kind == "five":
        s[0, 0] = -0.0  # -0 ties with +0
    y = (torch.rand(n, t, generator=gen) < 0.4).to(F64)
    y[0], y[1] = 1.0, 0.0  # both classes in every column
    mask = None
    if masked:
        mask = torch.rand(n, t, generator=gen) < 0.7
        mask[:2] = True
    keep = torch.ones(n, t, dtype=torch.bool) if mask is None else mask
    res = M.rank_metric_torch(s, y, mask)
    assert res.shape == (t, 4) and res.dtype == F64
    for j in range(t):
        assert abs(res[j, 0].item() - pairwise_auroc(s[:, j], y[:, j], keep[:, j])) <= TOL
        assert abs(res[j, 1].item() - threshold_ap(s[:, j], y[:, j], keep[:, j])) <= TOL
        assert res[j, 2].item() == (keep[:, j] & (y[:, j] == 1)).sum().item()
        assert res[j, 3].item() == (keep[:, j] & (y[:, j] == 0)).sum().item()
    for cls, lit in ((M.AUROC, pairwise_auroc), (M.AUPRC, threshold_ap)):
        macro = sum(lit(s[:, j], y[:, j], keep[:, j]) for j in range(t)) / t
        assert abs(cls("multilabel")(s, y, mask=mask).item() - macro) <= TOL
        pooled = lit(s.reshape(-1), y.reshape(-1), keep.reshape(-1))
        assert abs(cls("binary")(s, y, mask=mask).item() - pooled) <= TOL


def test_a_column_without_positives_is_nan_and_left_out_of_the_macro_mean():
    M = _metrics()
    gen = torch.Generator().manual_seed(9)
    n = 40
    s = torch.randn(n, 3, generator=gen, dtype=F64)
    y = (torch.rand(n, 3, generator=gen) < 0.5).to(F64)
    y[:2, 0], y[:2, 2] = torch.tensor([1.0, 0.0], dtype=F64), torch.tensor([1.0, 0.0], dtype=F64)
    y[:, 1] = 0.0  # no positives
    keep = torch.ones(n, dtype=torch.bool)
    res = M.rank_metric_torch(s, y)
    assert torch.isnan(res[1, :2]).all().item() and res[1, 2].item() == 0 and res[1, 3].item() == n
    for cls, lit in ((M.AUROC, pairwise_auroc), (M.AUPRC, threshold_ap)):
        want = (lit(s[:, 0], y[:, 0], keep) + lit(s[:, 2], y[:, 2], keep)) / 2
        assert abs(cls("multilabel")(s, y).item() - want) <= TOL
        assert torch.isnan(cls("multilabel")(s[:, 1:2], y[:, 1:2])).item()  # no column has both classes
    # positives that are all masked are no positives
    mask = torch.ones(n, 3, dtype=torch.bool)
    mask[:, 0] = y[:, 0] == 0
    assert torch.isnan(M.rank_metric_torch(s, y, mask)[0, 0]).item()
    # a perfect and an inverted ranking
    order = torch.arange(10, dtype=F64).reshape(10, 1)
    lab = (order >= 5).to(F64)
    assert M.AUROC("binary")(order, lab).item() == 1.0 and M.AUPRC("binary")(order, lab).item() == 1.0
    assert M.AUROC("binary")(-order, lab).item() == 0.0


def test_bindings_and_kinds():
    from notorch_amd import _lib

    assert set(_lib.LOSS_CODES) == {"mse", "mae", "rmse", "bce", "mve", "evidential", "xent"}
    assert sorted(_lib.LOSS_CODES.values()) == list(range(7))
    kinds = {c.KIND for c in (_loss().MSE, _metrics().MAE, _metrics().RMSE, _loss().BCE, _loss().MVE,
                              _loss().Evidential, _loss().XENT)}
    assert kinds == set(_lib.LOSS_CODES)
    assert _loss().Dirichlet.KIND is None and _metrics().R2.KIND is None and _metrics().Accuracy.KIND is None
