"""Deterministic input grids for the element math of nt_task_loss and its fp64 yardstick, shared by
tests/test_task_loss_host.py (task_loss_math.hpp compiled for the host) and tests/test_gpu_task_loss_edges.py
(the same values through the kernel).

A batch is (preds [n, c] or [n] fp32, targets [n] fp32).  ``element64`` is the yardstick: the module's
``_element`` (the literal formulas of nn/loss/loss.py and nn/metrics.py, with torch.digamma / torch.lgamma
behind autograd) in fp64 on the CPU on the same fp32 values, one element per row, and autograd's gradient of it.
"""
import functools
import itertools

import torch

V_KL, EPS = 0.2, 1e-8
MEAN = 0.25  # the mean channel of the Evidential and MVE grids: targets are fl(MEAN + r)

BELOW_6 = float(torch.nextafter(torch.tensor(6.0), torch.tensor(0.0)))  # the fp32 neighbour: digammaf's switch
EVIDENTIAL_ALPHAS = (1 + 1e-4, 1.5, 3.0, 5.5, BELOW_6, 6.0, 10.0, 30.0, 100.0, 1000.0, 1e4)
EVIDENTIAL_V = (1e-3, 0.1, 1.0, 10.0, 1e3)
EVIDENTIAL_BETA = (1e-2, 0.7, 50.0)
EVIDENTIAL_R = (0.0, 1e-3, -1e-3, 0.8, -0.8, 30.0, -30.0)
MVE_DECADES = tuple(range(-6, 6))  # v in [10^k, 10^(k+1)]
MVE_D = (0.0, 1e-3, -1e-3, 1.0, -1.0, 100.0, -100.0)
BCE_X = (0.0, 1e-4, 1.0, 10.0, 20.0, 40.0, 88.0, 100.0, 200.0)
BCE_Y = (0.0, 1.0, 0.3)
XENT_C = (1, 2, 3, 64, 1000)
XENT_SCALES = (1.0, 50.0, 1e4)
XENT_ROWS = 12


def module(kind):
    from notorch_amd.nn import loss as L
    from notorch_amd.nn import metrics as M

    return {"mse": L.MSE, "mae": M.MAE, "rmse": M.RMSE, "bce": L.BCE, "mve": L.MVE,
            "evidential": lambda: L.Evidential(V_KL, EPS), "xent": L.XENT}[kind]()


def element64(kind, p, y, lt=None, gt=None):
    """(L64 [n], g64 [n, c]) of fp32 preds p ([n] or [n, c]) and targets y ([n]); lt / gt ([n] bool) clamp an
    element to its target as _LossFunctionBase._forward does."""
    n = y.shape[0]
    q = p.double().reshape(n, 1, -1).clone().requires_grad_()
    t = y.double().reshape(n, 1)
    x = q.squeeze(-1) if p.dim() == 1 else q
    if lt is not None:
        x = torch.where((x < t) & lt.reshape(n, 1), t, x)
    if gt is not None:
        x = torch.where((x > t) & gt.reshape(n, 1), t, x)
    L = module(kind)._element(x, t)
    L.sum().backward()
    return L.detach().reshape(n), q.grad.reshape(n, -1)


def _f32(rows):
    return torch.tensor(rows, dtype=torch.float64).float()


@functools.lru_cache(maxsize=None)
def evidential(alpha):
    """Every (v, beta, r) at one alpha: 105 elements."""
    rows = [(MEAN, v, alpha, be, MEAN + r) for v, be, r in
            itertools.product(EVIDENTIAL_V, EVIDENTIAL_BETA, EVIDENTIAL_R)]
    a = _f32(rows)
    return a[:, :4].contiguous(), a[:, 4].contiguous()


@functools.lru_cache(maxsize=None)
def mve(decade):
    """v at 9 log-spaced points of [10^decade, 10^(decade + 1)], both ends included, times every d: 63 elements."""
    vs = [10.0 ** (decade + i / 8) for i in range(9)]
    a = _f32([(MEAN, v, MEAN - d) for v, d in itertools.product(vs, MVE_D)])  # d = m - y
    return a[:, :2].contiguous(), a[:, 2].contiguous()


@functools.lru_cache(maxsize=None)
def bce():
    xs = [s * x for x in BCE_X for s in (1.0, -1.0)]  # +0 and -0 both
    a = _f32(list(itertools.product(xs, BCE_Y)))
    return a[:, 0].contiguous(), a[:, 1].contiguous()


@functools.lru_cache(maxsize=None)
def xent(c, scale):
    """XENT_ROWS rows of randn * scale; the targets cycle through 0, c - 1, a fractional index (1.5 is class 1,
    as .long() truncates) and a seeded class."""
    gen = torch.Generator().manual_seed(1000 * c + int(scale))
    p = torch.randn(XENT_ROWS, c, generator=gen) * scale
    frac = 1.5 if c > 1 else 0.5
    rnd = torch.randint(0, c, (XENT_ROWS,), generator=gen).float()
    y = torch.tensor([(0.0, c - 1.0, frac, rnd[i].item())[i % 4] for i in range(XENT_ROWS)])
    return p.contiguous(), y


def xent_bad_targets(c):
    """Targets that are no class index: the element's loss and gradients are NaN."""
    return torch.tensor([-1.0, float(c), c + 0.5, -0.5, float("nan"), float("inf"), -float("inf")])


@functools.lru_cache(maxsize=None)
def bounded():
    """(x, y, lt, gt): x < y, x == y and x > y under all four (lt, gt) combinations."""
    pairs = [(0.5, 1.25), (1.25, 1.25), (2.0, 1.25), (-3.0, -1e-3), (0.0, 0.0), (1e-3, -1e-3), (-0.0, 0.0)]
    rows = [(x, y, lt, gt) for (x, y), lt, gt in itertools.product(pairs, (0, 1), (0, 1))]
    a = _f32(rows)
    return a[:, 0].contiguous(), a[:, 1].contiguous(), a[:, 2] != 0, a[:, 3] != 0
