"""CPU: the element math of nt_task_loss (csrc/task_loss_math.hpp) compiled for the host.

tests/host/task_loss_host.cpp, a stand-alone program that includes the header and nothing else of the project,
is built once per session with the host compiler (g++, else hipcc --offload-host-only) and fed the grids of
tests/task_loss_grids.py through a pipe; no shared library is loaded into Python.  The yardstick is torch in
fp64 on the CPU (the modules' _element and autograd: task_loss_grids.element64), the criterion the project's
fp32 contract per element:
    |L - L64| <= 1e-5 max(1, |L64|)        max_k |g_k - g64_k| <= 1e-5 max(1, max_k |g64_k|)
The bf16 instantiation must store, bit for bit, torch's rounding of the fp32 instantiation's gradient on the
widened inputs.  Every batch prints ``HOSTERR <kind> <loss error> <gradient error> <case>``.

One point leaves autograd: RMSE at x == y, where sqrt(d^2) differentiates to 0 * inf = NaN; the header
documents MAE's subgradient 0 there, and that is what the test holds it to."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import task_loss_grids as G

TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "task_loss_host.cpp")
CODES = {"mse": 0, "mae": 1, "rmse": 2, "bce": 3, "mve": 4, "evidential": 5, "xent": 6}
DIGAMMA, TO_BF16, FROM_BF16 = 100, 101, 102
F32, BF16 = 0, 1


def _rocm_include():
    return os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.fixture(scope="session")
def host(tmp_path_factory):
    """Path of the built program."""
    out = str(tmp_path_factory.mktemp("task_loss_host") / "task_loss_host")
    gxx, hipcc = shutil.which("g++"), shutil.which("hipcc") or shutil.which("hipcc", path="/opt/rocm/bin")
    if gxx:
        cmd = [gxx, "-std=c++17", "-O2", "-I" + _rocm_include(), "-D__HIP_PLATFORM_AMD__", SOURCE, "-o", out]
    elif hipcc:
        cmd = [hipcc, "--offload-host-only", "-x", "hip", "-std=c++17", "-O2", SOURCE, "-o", out]
    else:
        pytest.skip("neither g++ nor hipcc: no host compiler for tests/host/task_loss_host.cpp")
    subprocess.run(cmd, check=True)
    return out


def _header(kind, c, dtype, n, v_kl=G.V_KL, eps=G.EPS):
    return struct.pack("<iiiffq", kind, c, dtype, v_kl, eps, n)


def _pipe(host, payload, nbytes):
    res = subprocess.run([host], input=payload, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=False)
    assert res.returncode == 0, res.stderr.decode()
    assert len(res.stdout) == nbytes
    return res.stdout


def _map(host, kind, values, in_dtype, out_dtype):
    """One of the three scalar functions over a numpy array."""
    a = np.ascontiguousarray(values, dtype=in_dtype)
    out = _pipe(host, _header(kind, 1, F32, a.size) + a.tobytes(), a.size * np.dtype(out_dtype).itemsize)
    return np.frombuffer(out, dtype=out_dtype)


def _bits(x):
    """The bf16 bit patterns of a torch.bfloat16 tensor, as a numpy uint16 array."""
    return x.contiguous().view(torch.int16).numpy().view(np.uint16)


def _elements(host, kind, p, y, lt=None, gt=None, bf16=False):
    """(L [n] fp32, g [n, c]: fp32, or bf16 with bf16=True) of the program on preds p ([n] or [n, c]: fp32, or
    torch.bfloat16 with bf16=True) and fp32 targets y."""
    n = y.shape[0]
    p2 = p.reshape(n, -1)
    c = p2.shape[1]
    pt = "<u2" if bf16 else "<f4"
    rec = np.zeros(n, dtype=np.dtype([("p", pt, (c,)), ("y", "<f4"), ("lt", "u1"), ("gt", "u1")]))
    rec["p"] = _bits(p2) if bf16 else p2.numpy()
    rec["y"] = y.numpy()
    if lt is not None:
        rec["lt"] = lt.numpy()
    if gt is not None:
        rec["gt"] = gt.numpy()
    res = np.dtype([("L", "<f4"), ("g", pt, (c,))])
    assert rec.dtype.itemsize == c * (2 if bf16 else 4) + 6
    out = _pipe(host, _header(CODES[kind], c, BF16 if bf16 else F32, n) + rec.tobytes(), n * res.itemsize)
    out = np.frombuffer(out, dtype=res)
    L = torch.from_numpy(out["L"].copy())
    g = out["g"].copy()
    g = torch.from_numpy(g.view(np.int16)).view(torch.bfloat16) if bf16 else torch.from_numpy(g)
    return L, g


def _errors(L, g, L64, g64):
    """The worst element's loss and gradient error on the contract's scales."""
    assert torch.isfinite(L64).all().item() and torch.isfinite(g64).all().item()
    e_loss = (L.double() - L64).abs() / L64.abs().clamp_min(1.0)
    e_grad = (g.double() - g64).abs().amax(1) / g64.abs().amax(1).clamp_min(1.0)
    return e_loss.max().item(), e_grad.max().item()


def _hold(kind, case, L, g, L64, g64):
    e_loss, e_grad = _errors(L, g, L64, g64)
    print(f"HOSTERR {kind} {e_loss:.3e} {e_grad:.3e} {case}")
    assert e_loss <= TOL and e_grad <= TOL, (kind, case, e_loss, e_grad)


# ------------------------------------------------------------------------------------------------ digammaf
def _digamma_points():
    sweep = np.logspace(-3, 6, 2251).astype(np.float32)
    named = []
    for k in range(1, 7):
        x = np.float32(k)
        named += [np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(np.inf))]
    return np.concatenate([sweep, np.array(named, dtype=np.float32)])


def test_digammaf_holds_the_contract_from_1e_3_to_1e6(host):
    x = _digamma_points()
    assert x.size >= 2000 + 18 and x.min() == np.float32(1e-3) and x.max() == np.float32(1e6)
    got = torch.from_numpy(_map(host, DIGAMMA, x, "<f4", "<f4").copy()).double()
    want = torch.digamma(torch.from_numpy(x).double())
    err = (got - want).abs() / want.abs().clamp_min(1.0)
    worst = err.argmax().item()
    print(f"HOSTERR digammaf {err.max().item():.3e} at x={x[worst]!r}")
    assert err.max().item() <= TOL


def test_digammaf_is_nan_outside_its_domain(host):
    x = np.array([0.0, -0.0, -1e-3, -1.0, -2.5, -np.inf, np.nan], dtype=np.float32)
    assert np.isnan(_map(host, DIGAMMA, x, "<f4", "<f4")).all()


# --------------------------------------------------------------------------------------------- fp32 elements
@pytest.mark.parametrize("alpha", G.EVIDENTIAL_ALPHAS)
def test_evidential(host, alpha):
    p, y = G.evidential(alpha)
    assert p.shape == (105, 4) and ((y - p[:, 0]) == 0).sum().item() == 15
    _hold("evidential", f"alpha={alpha!r}", *_elements(host, "evidential", p, y), *G.element64("evidential", p, y))


def test_evidential_at_r_0_has_autograds_sign_convention(host):
    p, y = G.evidential(3.0)
    zero = (y - p[:, 0]) == 0
    _, g = _elements(host, "evidential", p[zero], y[zero])
    _, g64 = G.element64("evidential", p[zero], y[zero])
    assert (g64[:, 0] == 0).all().item() and (g[:, 0] == 0).all().item()  # sign(0) = 0 on both sides


@pytest.mark.parametrize("decade", G.MVE_DECADES)
def test_mve(host, decade):
    p, y = G.mve(decade)
    _hold("mve", f"v in [1e{decade}, 1e{decade + 1}]", *_elements(host, "mve", p, y), *G.element64("mve", p, y))


def test_bce(host):
    p, y = G.bce()
    assert p.shape == (54,) and p.abs().max().item() == 200
    _hold("bce", "x in +-[0, 200]", *_elements(host, "bce", p, y), *G.element64("bce", p, y))


@pytest.mark.parametrize("scale", G.XENT_SCALES)
@pytest.mark.parametrize("c", G.XENT_C)
def test_xent(host, c, scale):
    p, y = G.xent(c, scale)
    L, g = _elements(host, "xent", p, y)
    _hold("xent", f"c={c} scale={scale:g}", L, g, *G.element64("xent", p, y))
    if c == 1:
        assert (L == 0).all().item() and (g == 0).all().item()


@pytest.mark.parametrize("c", G.XENT_C)
def test_xent_is_nan_for_a_target_that_is_no_class(host, c):
    bad = G.xent_bad_targets(c)
    p = G.xent(c, 1.0)[0][: bad.shape[0]]
    L, g = _elements(host, "xent", p, bad)
    assert torch.isnan(L).all().item() and torch.isnan(g).all().item()


@pytest.mark.parametrize("kind", ("mse", "mae", "rmse"))
def test_bounds(host, kind):
    x, y, lt, gt = G.bounded()
    L, g = _elements(host, kind, x, y, lt, gt)
    clamped = ((x < y) & lt) | ((x > y) & gt)
    assert 0 < clamped.sum().item() < x.shape[0] and (x == y).sum().item() >= 8
    assert (L[clamped] == 0).all().item() and (g[clamped, 0] == 0).all().item()
    L64, g64 = G.element64(kind, x, y, lt, gt)
    if kind == "rmse":  # x == y: autograd's 0 * inf; the documented value is MAE's 0
        assert torch.isnan(g64[x == y]).all().item() and (g[x == y] == 0).all().item()
        g64[x == y] = 0.0
    _hold("bounded_" + kind, "x < y, x == y, x > y under every (lt, gt)", L, g, L64, g64)
    assert (L64[clamped] == 0).all().item() and (g64[clamped] == 0).all().item()


# ------------------------------------------------------------------------------------------------------ bf16
def _bf16_cases():
    """(kind, preds fp32, targets, lt, gt): the grids plus seeded values, before rounding to bf16."""
    gen = torch.Generator().manual_seed(7)
    n = 257
    y = torch.randn(n, generator=gen)
    sp = lambda: torch.nn.functional.softplus(torch.randn(n, generator=gen))  # noqa: E731
    x, by, lt, gt = G.bounded()
    cases = [(k, x, by, lt, gt) for k in ("mse", "mae", "rmse")]
    cases += [(k, torch.randn(n, generator=gen), y, torch.rand(n, generator=gen) < 0.3,
               torch.rand(n, generator=gen) < 0.3) for k in ("mse", "mae", "rmse")]
    cases += [("bce", *G.bce(), None, None), ("bce", torch.randn(n, generator=gen) * 3, (y > 0).float(), None, None)]
    cases += [("mve", *G.mve(d), None, None) for d in (-6, 0, 5)]
    cases += [("mve", torch.stack([torch.randn(n, generator=gen), sp() + 0.1], 1), y, None, None)]
    cases += [("evidential", *G.evidential(a), None, None) for a in (1.5, 6.0, 100.0)]
    cases += [("evidential", torch.stack([torch.randn(n, generator=gen), sp() + 0.1, sp() + 1, sp() + 0.1], 1), y,
               None, None)]
    cases += [("xent", *G.xent(c, s), None, None) for c, s in ((1, 1.0), (2, 50.0), (3, 1.0), (64, 1.0), (1000, 50.0))]
    return cases


def test_bf16_instantiation_stores_torchs_rounding_of_the_fp32_gradient(host):
    seen = set()
    for kind, p, y, lt, gt in _bf16_cases():
        pb = p.bfloat16()
        L16, g16 = _elements(host, kind, pb, y, lt, gt, bf16=True)
        L32, g32 = _elements(host, kind, pb.float(), y, lt, gt)
        assert g16.dtype == torch.bfloat16 and g32.dtype == torch.float32
        assert np.array_equal(L16.numpy().view(np.uint32), L32.numpy().view(np.uint32))  # the loss is not rounded
        want = g32.bfloat16()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(g16), nan)
        assert np.array_equal(_bits(g16)[~nan.numpy()], _bits(want)[~nan.numpy()]), kind
        if (g32[~nan] != want[~nan].float()).any().item():
            seen.add(kind)  # the rounding had something to round
    assert seen == set(CODES) - {"mae", "rmse"}  # whose gradients are 0 and +-1


def _f32_patterns():
    """Every bf16 value, its midpoint to the next one, one fp32 ulp either side of both, and the last fp32
    before the next bf16 value: +-0, denormals, +-inf and NaNs among them."""
    high = np.arange(1 << 16, dtype=np.uint32) << 16
    low = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)
    return (high[:, None] | low[None, :]).reshape(-1)


def test_float_to_bf16_bits_is_torchs_rounding_on_every_bf16_value_and_midpoint(host):
    bits = _f32_patterns()
    assert bits.size == 6 << 16
    got = _map(host, TO_BF16, bits.view(np.float32), "<f4", "<u2")
    f = torch.from_numpy(bits.view(np.int32).copy()).view(torch.float32)
    want = _bits(f.bfloat16())
    nan = torch.isnan(f).numpy()
    assert nan.sum() > 0 and np.isinf(bits.view(np.float32)).sum() == 2
    got_nan = ((got & 0x7F80) == 0x7F80) & ((got & 0x007F) != 0)
    assert np.array_equal(got_nan, nan)  # a NaN stays a NaN, nothing else becomes one
    assert np.array_equal(got[~nan], want[~nan])
    # ties go to the even neighbour: a midpoint over an odd bf16 value rounds up, over an even one down
    mid = (bits & 0xFFFF) == 0x8000
    odd = ((bits >> 16) & 1) == 1
    finite = ~nan & (((bits >> 16) & 0x7F80) != 0x7F80)
    up = (bits >> 16).astype(np.uint16) + np.uint16(1)
    assert np.array_equal(got[mid & odd & finite], up[mid & odd & finite])
    assert np.array_equal(got[mid & ~odd & finite], (bits >> 16).astype(np.uint16)[mid & ~odd & finite])


def test_bf16_bits_to_float_is_exact(host):
    u = np.arange(1 << 16, dtype=np.uint16)
    got = _map(host, FROM_BF16, u, "<u2", "<f4")
    assert np.array_equal(got.view(np.uint32), u.astype(np.uint32) << 16)
    back = _map(host, TO_BF16, got, "<f4", "<u2")
    nan = np.isnan(got)
    assert np.array_equal(back[~nan], u[~nan])


def test_program_rejects_a_truncated_input(host):
    res = subprocess.run([host], input=_header(CODES["mse"], 1, F32, 4) + b"\0" * 7, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, check=False)
    assert res.returncode == 2 and b"truncated" in res.stderr
    res = subprocess.run([host], input=_header(CODES["mve"], 3, F32, 0), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, check=False)
    assert res.returncode == 2 and b"does not fit" in res.stderr
