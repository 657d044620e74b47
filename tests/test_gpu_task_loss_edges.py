"""GPU: nt_task_loss (csrc/task_loss.hip) at the seams and extremes tests/test_gpu_task_loss.py leaves out.

The scheme is that file's: the torch route in fp64 on the CPU as yardstick, NT_LOSS=kernel, the fp32 contract
    |L - L64| <= 1e-5 max(1, |L64|)        max|g - g64| <= 1e-5 max|g64|      (bf16: 2^-8 + 1e-5)
and ``LOSSERR <kind> <value> <case>`` lines.  Added here:
  * bf16 preds for every kind (the instantiation autocast reaches), Bounded forms included;
  * the launch-size seams: 8192 elements (the last one-launch size, as 8192 x 1 and 4096 x 2), 8193, 16384, and
    5462 x 3 = 16386, where a weights row straddles both workgroup boundaries; 1024 * 8192 + 1 elements once,
    1025 partials, the first size at which the finalize kernel's loop takes a second step;
  * XENT at c = 1, 2, 64 and 1000;
  * the grids of tests/task_loss_grids.py (alpha to 1e4, v over 1e-6 .. 1e6, |x| to 200, logits of 1e4), one
    batch per alpha / decade / scale so that a large element does not set the scale for a small one, with the
    gradient error taken per channel: e_k = max|g_k - g64_k| / max|g64_k|.  Nobody has measured the device's
    lgammaf, logf and expf at such arguments, so the yardstick for the bound is the torch route in fp32 on the
    device on the same inputs, e_torch, and the kernel must stay within e <= max(1e-5, 4 e_torch): the factor
    allows a different operation order a few more roundings of the largest intermediate, while a wrong branch,
    coefficient or stride shows at 1e-3 or worse.  A channel whose fp64 gradients are below fp32's smallest
    normal number over 1e-5 is measured on that scale: a flush to zero is within the contract there;
  * NaN parity with the device torch route.
"""
import time

import pytest
import torch

import task_loss_grids as G
from test_gpu_task_loss import DEV, TOL, _check, _inputs, _K, _module, _run

pytestmark = pytest.mark.gpu

BF16_GTOL = 2.0 ** -8 + TOL
SEAMS = ((8192, 1), (4096, 2), (8193, 1), (16384, 1), (5462, 3))
TINY = torch.finfo(torch.float32).tiny / TOL


def _lib():
    from notorch_amd import _lib

    return _lib


# ------------------------------------------------------------------------------------------- bf16, every kind
@pytest.mark.parametrize("b,t", ((65, 3), (2731, 3)))
@pytest.mark.parametrize("kind", ("mae", "rmse", "bce", "evidential", "xent"))
def test_bf16_preds(kind, b, t, monkeypatch):
    monkeypatch.setenv("NT_LOSS", "kernel")
    mod = _module(kind)
    p, y, rnd, _, w, _, _ = _inputs(kind, b, t)
    pb = p.bfloat16()
    for mask in (None, rnd):
        want = _run(mod, pb.double(), y, mask, w, {}, "cpu", torch.float64)
        got = _run(mod, pb, y, mask, w, {}, DEV, torch.bfloat16)
        assert got[1].dtype == torch.bfloat16
        _check(kind + "_bf16", f"b={b} t={t} mask={'none' if mask is None else 'random'}", got, want, gtol=BF16_GTOL)


@pytest.mark.parametrize("b,t", ((65, 3), (2731, 3)))
@pytest.mark.parametrize("kind", ("mse", "mae"))
def test_bf16_preds_bounded(kind, b, t, monkeypatch):
    from notorch_amd.nn.loss import BoundedMSE
    from notorch_amd.nn.metrics import BoundedMAE

    monkeypatch.setenv("NT_LOSS", "kernel")
    mod = BoundedMSE() if kind == "mse" else BoundedMAE()
    p, y, rnd, _, w, lt, gt = _inputs(kind, b, t)
    pb = p.bfloat16()
    bounds = dict(lt_mask=lt, gt_mask=gt)
    clamped = ((pb.float() < y) & lt) | ((pb.float() > y) & gt)
    assert 0 < clamped.sum().item() < b * t
    for mask in (None, rnd):
        want = _run(mod, pb.double(), y, mask, w, bounds, "cpu", torch.float64)
        got = _run(mod, pb, y, mask, w, bounds, DEV, torch.bfloat16)
        assert got[1].dtype == torch.bfloat16
        _check(f"bounded_{kind}_bf16", f"b={b} t={t} mask={'none' if mask is None else 'random'}", got, want,
               gtol=BF16_GTOL)
        assert (got[1].cpu()[clamped] == 0).all().item()


# ------------------------------------------------------------------------------------------------ size seams
def _xent_inputs(b, t, c):
    gen = torch.Generator().manual_seed(100 * b + 10 * t + c)
    p = torch.randn(b, t, c, generator=gen)
    y = torch.randint(0, c, (b, t), generator=gen).float()
    return p, y, torch.rand(b, t, generator=gen) < 0.6, torch.rand(b, generator=gen) + 0.5


def _seam_inputs(kind, b, t):
    if kind == "xent":
        return _xent_inputs(b, t, 3)
    p, y, rnd, _, w, _, _ = _inputs(kind, b, t)
    return p, y, rnd, w


@pytest.mark.parametrize("b,t", SEAMS)
@pytest.mark.parametrize("kind", ("mse", "xent"))
def test_launch_size_seams(kind, b, t, monkeypatch):
    monkeypatch.setenv("NT_LOSS", "kernel")
    K, lib = _K(), _lib()
    mod = _module(kind)
    p, y, rnd, w = _seam_inputs(kind, b, t)
    want = _run(mod, p.double(), y, rnd, w, {}, "cpu", torch.float64)
    got = _run(mod, p, y, rnd, w, {}, DEV, torch.float32)
    _check(kind, f"b={b} t={t} mask=random weights=random (seam)", got, want)
    need = int(lib.load().nt_task_loss_workspace(b, t))
    if b * t <= 8192:
        assert need == 0 and K.task_loss_single_max() == 8192
        return
    assert need == 16 + 16 * ((b * t + 8191) // 8192)
    # the same call as K.task_loss, on a workspace one byte short
    pd, yd, md, wd = p.to(DEV), y.to(DEV), rnd.to(DEV).view(torch.uint8), w.to(DEV)
    loss, ws = torch.empty((), device=DEV), torch.empty(need, dtype=torch.uint8, device=DEV)
    c = p.shape[2] if p.dim() == 3 else 1
    args = (pd.data_ptr(), lib.NT_F32, yd.data_ptr(), md.data_ptr(), wd.data_ptr(), None, None, b, t, c,
            lib.LOSS_CODES[kind], 0.0, 0.0, loss.data_ptr(), None, ws.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(lib.NativeLibraryError, match="workspace"):
        K._run(pd.device, lib.load().nt_task_loss, *args, need - 1, stream)
    K._run(pd.device, lib.load().nt_task_loss, *args, need, stream)
    assert torch.equal(loss, got[0])


def test_1025_partials_once(monkeypatch):
    """b = 1024 * 8192 + 1: the finalize kernel's loop over the partials takes a second step, for one partial."""
    monkeypatch.setenv("NT_LOSS", "kernel")
    K = _K()
    b, t = 1024 * 8192 + 1, 1
    assert (b * t + 8191) // 8192 == 1025
    gen = torch.Generator().manual_seed(1025)
    p, y = torch.randn(b, t, generator=gen), torch.randn(b, t, generator=gen)
    rnd, w = torch.rand(b, t, generator=gen) < 0.6, torch.rand(b, generator=gen) + 0.5
    mod = _module("mse")
    want = _run(mod, p.double(), y, rnd, w, {}, "cpu", torch.float64)
    args = (p.to(DEV), y.to(DEV), "mse", rnd.to(DEV), w.to(DEV), None, None, 0.0, 0.0, True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = K.task_loss(*args)
    torch.cuda.synchronize()
    print(f"LOSSTIME mse {1e3 * (time.perf_counter() - t0):.3f} ms first call b={b} t={t}")
    again = K.task_loss(*args)
    _check("mse", f"b={b} t={t} mask=random weights=random (1025 partials)", first, want)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


# ---------------------------------------------------------------------------------------- XENT class counts
@pytest.mark.parametrize("c", (1, 2, 64, 1000))
def test_xent_class_counts(c, monkeypatch):
    monkeypatch.setenv("NT_LOSS", "kernel")
    b, t = 257, 2
    mod = _module("xent")
    p, y, rnd, w = _xent_inputs(b, t, c)
    want = _run(mod, p.double(), y, rnd, w, {}, "cpu", torch.float64)
    got = _run(mod, p, y, rnd, w, {}, DEV, torch.float32)
    assert got[1].shape == (b, t, c)
    _check("xent", f"b={b} t={t} c={c} mask=random weights=random", got, want)
    if c == 1:
        assert got[0].item() == 0.0 and (got[1] == 0).all().item()


# ------------------------------------------------------------------------------------------- extreme values
def _three_routes(kind, p, y, monkeypatch):
    """(loss, grad [n, c]) in fp64 on the CPU, of the torch route in fp32 on the device and of K.task_loss: no mask,
    b = n, t = 1."""
    n = y.shape[0]
    p3 = p.reshape(n, 1, -1) if p.dim() == 2 else p.reshape(n, 1)
    y2 = y.reshape(n, 1)
    mod = G.module(kind)
    want = _run(mod, p3.double(), y2, None, None, {}, "cpu", torch.float64)
    monkeypatch.setenv("NT_LOSS", "torch")
    ref32 = _run(mod, p3, y2, None, None, {}, DEV, torch.float32)
    loss, g = _K().task_loss(p3.to(DEV).contiguous(), y2.to(DEV), kind, None, None, None, None, G.V_KL, G.EPS, True)
    assert loss.dtype == torch.float32 and g.dtype == torch.float32 and g.shape == p3.shape
    flat = lambda r: (r[0].double().cpu().item(), r[1].double().cpu().reshape(n, -1))  # noqa: E731
    return flat(want), flat(ref32), flat((loss, g))


def _hold_to_the_torch_route(kind, case, want, ref32, got):
    (l64, g64), (lt, gt), (lk, gk) = want, ref32, got
    assert l64 == l64 and torch.isfinite(g64).all().item()
    scale = g64.abs().amax(0).clamp_min(TINY)
    e_loss, t_loss = abs(lk - l64) / max(1.0, abs(l64)), abs(lt - l64) / max(1.0, abs(l64))
    e_g, t_g = (gk - g64).abs().amax(0) / scale, (gt - g64).abs().amax(0) / scale
    print(f"LOSSERR {kind} {e_loss:.3e} loss {case} e_torch={t_loss:.3e} L64={l64:.6e}")
    names = {"evidential": ("mean", "v", "alpha", "beta"), "mve": ("mean", "v")}.get(kind)
    if names:
        for k, name in enumerate(names):
            print(f"LOSSERR {kind} {e_g[k].item():.3e} grad_{name} {case} e_torch={t_g[k].item():.3e} "
                  f"max|g64|={g64[:, k].abs().max().item():.3e}")
    else:
        k = int(e_g.argmax())
        print(f"LOSSERR {kind} {e_g[k].item():.3e} grad {case} worst of {e_g.numel()} channels, its "
              f"e_torch={t_g[k].item():.3e}; worst e_torch={t_g.max().item():.3e}")
    assert e_loss <= max(TOL, 4 * t_loss if t_loss == t_loss else 0.0)
    bound = torch.where(torch.isfinite(t_g), 4 * t_g, torch.zeros_like(t_g)).clamp_min(TOL)
    assert (e_g <= bound).all().item(), (kind, case, e_g.tolist(), t_g.tolist())


@pytest.mark.parametrize("alpha", G.EVIDENTIAL_ALPHAS)
def test_extreme_evidential(alpha, monkeypatch):
    p, y = G.evidential(alpha)
    _hold_to_the_torch_route("evidential", f"alpha={alpha!r} n={len(y)}", *_three_routes("evidential", p, y, monkeypatch))


@pytest.mark.parametrize("decade", G.MVE_DECADES)
def test_extreme_mve(decade, monkeypatch):
    p, y = G.mve(decade)
    _hold_to_the_torch_route("mve", f"v in [1e{decade}, 1e{decade + 1}] n={len(y)}",
                             *_three_routes("mve", p, y, monkeypatch))


def test_extreme_bce(monkeypatch):
    p, y = G.bce()
    _hold_to_the_torch_route("bce", f"x in +-[0, 200] n={len(y)}", *_three_routes("bce", p, y, monkeypatch))


@pytest.mark.parametrize("scale", G.XENT_SCALES)
@pytest.mark.parametrize("c", G.XENT_C)
def test_extreme_xent(c, scale, monkeypatch):
    p, y = G.xent(c, scale)
    _hold_to_the_torch_route("xent", f"c={c} scale={scale:g} n={len(y)}", *_three_routes("xent", p, y, monkeypatch))


# ------------------------------------------------------------------------------------------------ NaN parity
@pytest.mark.parametrize("where", ("target under a false mask entry", "prediction under a true mask entry"))
def test_nan_parity_with_the_device_torch_route(where, monkeypatch):
    b, t = 65, 3
    p, y, rnd, _, w, _, _ = (x.clone() for x in _inputs("mse", b, t))
    if where.startswith("target"):
        i, j = (~rnd).nonzero()[3].tolist()
        y[i, j] = float("nan")
    else:
        i, j = rnd.nonzero()[3].tolist()
        p[i, j] = float("nan")
    mod = _module("mse")
    monkeypatch.setenv("NT_LOSS", "torch")
    t_loss, t_g = _run(mod, p, y, rnd, w, {}, DEV, torch.float32)
    monkeypatch.setenv("NT_LOSS", "kernel")
    k_loss, k_g = _run(mod, p, y, rnd, w, {}, DEV, torch.float32)
    print(f"LOSSERR mse nan-parity {where}: loss nan={torch.isnan(t_loss).item()} "
          f"grad nans={torch.isnan(t_g).sum().item()} at {torch.isnan(t_g).nonzero().tolist()}")
    assert torch.isnan(k_loss).item() == torch.isnan(t_loss).item()
    assert torch.equal(torch.isnan(k_g), torch.isnan(t_g))
    ok = ~torch.isnan(t_g)
    assert (k_g[ok] - t_g[ok]).abs().max().item() <= TOL * t_g[ok].abs().max().item()
    if not torch.isnan(t_loss).item():
        assert abs(k_loss.item() - t_loss.item()) <= TOL * max(1.0, abs(t_loss.item()))
