"""CPU: nt_mlp_head_supported / nt_mlp_head_forward (include/notorch_amd_train.h, csrc/mlp_head.hip) are bound and
validate on the host before any device call (fake, aligned pointers only, as tests/test_abi_dirichlet.py), and
nn/mlp.py's pure mlp_route decides as documented."""
import ctypes

import pytest
import torch

OK, EINVAL, EUNSUPPORTED = 0, 1, 3
F32, BF16 = 0, 1
X, OUT, W0, W1, B0 = (ctypes.c_void_p(0x1000 * (i + 1)) for i in range(5))


def _lib():
    from notorch_amd import _lib

    return _lib.load()


def _dims(*d):
    return (ctypes.c_int64 * len(d))(*d)


def _fwd(lib, dims=(300, 256, 1), rows=8, pitch=None, x=X, out=OUT, W=(W0, W1), b=(B0, None), xdt=F32, pdt=F32,
         odt=F32, act=1, nlayers=None, dims_ptr=True):
    n = len(dims) - 1 if nlayers is None else nlayers
    Wp = None if W is None else (ctypes.c_void_p * len(W))(*W)
    bp = None if b is None else (ctypes.c_void_p * len(b))(*b)
    return lib.nt_mlp_head_forward(x, xdt, rows, dims[0] if pitch is None else pitch, n, Wp, bp, pdt,
                                   _dims(*dims) if dims_ptr else None, act, 0.1, out, odt, None)


def test_bound_and_limits_stated_once():
    from notorch_amd import _lib as L

    lib = _lib()
    for name in ("nt_mlp_head_supported", "nt_mlp_head_forward"):
        assert name in L.EXT_SIGNATURES and name not in L.SIGNATURES and hasattr(lib, name)
    assert lib.nt_abi_version() == L.ABI_VERSION == 8
    ok = lib.nt_mlp_head_supported
    assert ok(F32, F32, 2, _dims(300, 256, 1)) == 1 and ok(BF16, F32, 1, _dims(300, 5)) == 1
    # at and one past each bound: 8 layers, in <= 8192, every later width <= 1264
    assert ok(F32, F32, 8, _dims(*[8] * 9)) == 1 and ok(F32, F32, 9, _dims(*[8] * 10)) == 0
    assert ok(F32, F32, 0, _dims(8)) == 0
    assert ok(F32, F32, 2, _dims(8192, 1264, 1264)) == 1
    assert ok(F32, F32, 2, _dims(8193, 8, 8)) == 0
    assert ok(F32, BF16, 2, _dims(8, 1265, 8)) == 0 and ok(BF16, BF16, 2, _dims(8, 8, 1265)) == 0
    assert ok(F32, F32, 2, _dims(8, 0, 8)) == 0 and ok(5, F32, 1, _dims(8, 8)) == 0 and ok(F32, 5, 1, _dims(8, 8)) == 0
    assert ok(F32, F32, 1, None) == 0


def test_forward_validates_on_the_host():
    lib = _lib()
    for bad in (dict(x=None), dict(out=None), dict(W=None), dict(dims_ptr=False), dict(W=(W0, None))):
        assert _fwd(lib, **bad) == EINVAL and b"NULL" in lib.nt_last_error(), bad
    for n in (0, 9, -1):
        assert _fwd(lib, nlayers=n) == EINVAL and b"nlayers" in lib.nt_last_error()
    for bad in (dict(dims=(300, 0, 1)), dict(dims=(-3, 256, 1)), dict(rows=-1)):
        assert _fwd(lib, **bad) == EINVAL and b"bad sizes" in lib.nt_last_error(), bad
    for bad in (dict(xdt=5), dict(pdt=2), dict(odt=7), dict(xdt=BF16), dict(pdt=BF16)):  # fp32 out: fp32 operands
        assert _fwd(lib, **bad) == EUNSUPPORTED and b"dtype" in lib.nt_last_error(), bad
    assert _fwd(lib, act=8) == EINVAL and b"act" in lib.nt_last_error()
    assert _fwd(lib, pitch=299) == EINVAL and b"pitch" in lib.nt_last_error()
    assert _fwd(lib, pitch=302) == EINVAL and b"16 bytes" in lib.nt_last_error()  # fp32: pieces of 4
    assert _fwd(lib, pitch=308, xdt=BF16, odt=BF16) == EINVAL and b"16 bytes" in lib.nt_last_error()  # bf16: of 8
    assert _fwd(lib, dims=(300, 1265, 1)) == EUNSUPPORTED and b"LDS" in lib.nt_last_error()
    assert _fwd(lib, dims=(8193, 256, 1)) == EUNSUPPORTED
    # nothing to do: OK without a launch (a launch on this CPU-only path would answer NT_EHIP = 2)
    assert _fwd(lib, rows=0) == OK and _fwd(lib, rows=0, pitch=304, b=None) == OK
    assert _fwd(lib, rows=0, xdt=BF16, pdt=BF16, odt=BF16, pitch=304) == OK


def test_kernels_binding_validates_before_the_library():
    from notorch_amd import kernels as K

    with pytest.raises(RuntimeError, match="ROCm devices only"):
        K.mlp_head(torch.zeros(4, 8), [torch.zeros(2, 8)], [None], (1, 0.0))
    assert K.mlp_head_supported(torch.float32, torch.float32, [300, 1264, 1]) is True
    assert K.mlp_head_supported(torch.float16, torch.float32, [300, 1]) is False


def test_mlp_route_decisions(monkeypatch):
    from notorch_amd.nn import mlp

    f32, bf16 = torch.float32, torch.bfloat16
    base = dict(device_type="cuda", chain_ok=True, hooks=False, dropout_active=False, needs_grad=False, x_dtype=f32,
                param_dtype=f32, autocast="", supported=True, rows=4096, widest=300, nlayers=2, knob="kernel")

    def route(**over):
        return mlp.mlp_route(**{**base, **over})

    assert route() == "kernel"
    for over in (dict(knob="torch"), dict(device_type="cpu"), dict(chain_ok=False), dict(hooks=True),
                 dict(dropout_active=True), dict(needs_grad=True), dict(supported=False), dict(param_dtype=None),
                 dict(x_dtype=bf16), dict(param_dtype=bf16), dict(x_dtype=bf16, param_dtype=bf16),
                 dict(autocast="other"), dict(autocast="bf16", x_dtype=torch.float16),
                 dict(autocast="bf16", param_dtype=torch.float64)):
        assert route(**over) == "torch", over
    for x_dtype in (f32, bf16):
        for param_dtype in (f32, bf16):
            assert route(autocast="bf16", x_dtype=x_dtype, param_dtype=param_dtype) == "kernel"
    # NT_MLP unset: the measured range alone
    monkeypatch.setattr(mlp, "MLP_KERNEL_ROWS", {"fp32": (0, 0), "bf16": (1, 512)})
    monkeypatch.setattr(mlp, "MLP_KERNEL_MAX_WIDTH", 300)
    monkeypatch.setattr(mlp, "MLP_KERNEL_LAYERS", (2, 3))
    assert route(knob="") == "torch" and route(knob="", autocast="bf16") == "torch"
    assert route(knob="", autocast="bf16", rows=512) == "kernel" and route(knob="", autocast="bf16", rows=513) == "torch"
    assert route(knob="", autocast="bf16", rows=512, widest=301) == "torch"
    assert route(knob="", autocast="bf16", rows=0) == "torch"
    assert route(knob="", autocast="bf16", rows=512, nlayers=3) == "kernel"
    assert route(knob="", autocast="bf16", rows=512, nlayers=1) == "torch"
