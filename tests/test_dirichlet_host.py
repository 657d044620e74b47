"""CPU: the element math of nt_dirichlet_loss (csrc/dirichlet_math.hpp) compiled for the host
(tests/host/dirichlet_host.cpp, built once per session and fed through a pipe).  The yardstick is
``Dirichlet._element`` and autograd in fp64 on the CPU, the criterion tests/test_task_loss_host.py's per element:
    |L - L64| <= 1e-5 max(1, |L64|)        max_c |g_c - g64_c| <= 1e-5 max(1, max_c |g64_c|)
At logits of 1e4 the bound is max(1e-5, 4 e_torch), e_torch the same figure of ``_element`` in fp32 on the CPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

TOL, V_KL, ROWS = 1e-5, 0.2, 12
SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "dirichlet_host.cpp")
KS = (1, 2, 3, 64, 65)


@pytest.fixture(scope="session")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dirichlet_host") / "dirichlet_host")
    inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    gxx, hipcc = shutil.which("g++"), shutil.which("hipcc") or shutil.which("hipcc", path="/opt/rocm/bin")
    if gxx:
        cmd = [gxx, "-std=c++17", "-O2", "-I" + inc, "-D__HIP_PLATFORM_AMD__", SOURCE, "-o", out]
    elif hipcc:
        cmd = [hipcc, "--offload-host-only", "-x", "hip", "-std=c++17", "-O2", SOURCE, "-o", out]
    else:
        pytest.skip("neither g++ nor hipcc: no host compiler for tests/host/dirichlet_host.cpp")
    subprocess.run(cmd, check=True)
    return out


def _pipe(host, what, k, rec):
    """The program's fp32 results on the fp32 records rec [n, width], in the same shape."""
    rec = np.ascontiguousarray(rec, dtype="<f4")
    res = subprocess.run([host], input=struct.pack("<iifi", what, k, V_KL, rec.shape[0]) + rec.tobytes(),
                         stdout=subprocess.PIPE, check=True)
    return torch.from_numpy(np.frombuffer(res.stdout, dtype="<f4").reshape(rec.shape).copy())


def _errors(host, x, y, dtype=None):
    """The worst element's (loss, gradient) error against fp64 of the program, or of _element in ``dtype``."""
    from notorch_amd.nn.loss import Dirichlet

    def element(dt):
        q = x.to(dt).unsqueeze(1).clone().requires_grad_()
        L = Dirichlet(V_KL)._element(q, y.to(dt).unsqueeze(1))
        L.sum().backward()
        return L.detach().double().reshape(-1), q.grad.double().squeeze(1)

    L64, g64 = element(torch.float64)
    assert torch.isfinite(L64).all().item() and torch.isfinite(g64).all().item()
    out = _pipe(host, 0, x.shape[1], torch.cat([x, y[:, None]], 1).numpy()) if dtype is None else None
    L, g = (out[:, 0], out[:, 1:]) if dtype is None else element(dtype)
    e_loss = (L.double() - L64).abs() / L64.abs().clamp_min(1.0)
    e_grad = (g.double() - g64).abs().amax(1) / g64.abs().amax(1).clamp_min(1.0)
    return e_loss.max().item(), e_grad.max().item()


def _batch(k, scale):
    """ROWS rows of randn * scale (a float) or of the constant ``scale`` (an int); the targets cycle through 0,
    k - 1 and a fractional index (1.5 is class 1, as .long() truncates)."""
    gen = torch.Generator().manual_seed(1000 * k + int(abs(scale)))
    x = torch.randn(ROWS, k, generator=gen) * scale if isinstance(scale, float) else torch.full((ROWS, k), float(scale))
    return x.contiguous(), torch.tensor([(0.0, k - 1.0, 1.5 if k > 1 else 0.5)[i % 3] for i in range(ROWS)])


def test_trigammaf_holds_the_contract_from_1_to_1e6(host):
    named = [np.nextafter(np.float32(i), np.float32(d)) for i in range(1, 7) for d in (0, i, np.inf)]
    x = np.concatenate([np.logspace(0, 6, 1501), named]).astype(np.float32)  # the shift covers 1's lower neighbour
    assert x.size == 1519 and x.min() == named[0] < 1 and x.max() == np.float32(1e6)
    want = torch.polygamma(1, torch.from_numpy(x).double())
    err = (_pipe(host, 1, 1, x[:, None])[:, 0].double() - want).abs() / want
    print(f"HOSTERR trigammaf {err.max().item():.3e} at x={x[err.argmax().item()]!r}")
    assert err.max().item() <= TOL


@pytest.mark.parametrize("scale", (1.0, 50.0, 200, -200, 1e4))
@pytest.mark.parametrize("k", KS)
def test_element_holds_the_contract(host, k, scale):
    x, y = _batch(k, scale)
    e_loss, e_grad = _errors(host, x, y)
    t_loss, t_grad = _errors(host, x, y, torch.float32) if scale == 1e4 else (0.0, 0.0)
    print(f"HOSTERR dirichlet {e_loss:.3e} {e_grad:.3e} k={k} scale={scale} e_torch={t_loss:.3e} {t_grad:.3e}")
    assert e_loss <= max(TOL, 4 * t_loss) and e_grad <= max(TOL, 4 * t_grad)


@pytest.mark.parametrize("k", KS)
def test_a_target_that_is_no_class_is_nan(host, k):
    bad = torch.tensor([-1.0, float(k), k + 0.5, -0.5, float("nan"), float("inf"), -float("inf")])
    assert torch.isnan(_pipe(host, 0, k, torch.cat([_batch(k, 1.0)[0][:7], bad[:, None]], 1).numpy())).all().item()
