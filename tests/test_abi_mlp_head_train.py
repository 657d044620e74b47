"""CPU: the training entries of the fused MLP head (include/notorch_amd_train.h, csrc/mlp_head.hip,
csrc/mlp_head_train.hip) are bound and validate on the host before any device call (fake, aligned pointers only, as
tests/test_abi_mlp_head.py), and nn/mlp.py's pure mlp_train_route decides as documented."""
import ctypes

import pytest
import torch

OK, EINVAL, EUNSUPPORTED = 0, 1, 3
F32, BF16 = 0, 1
DY, X, DX, W0, W1, Z0, G0, G1, B0, WS = (ctypes.c_void_p(0x1000 * (i + 1)) for i in range(10))
NAMES = ("nt_mlp_head_train_supported", "nt_mlp_head_forward_train", "nt_mlp_head_backward_workspace",
         "nt_mlp_head_backward")


def _lib():
    from notorch_amd import _lib

    return _lib.load()


def _dims(*d):
    return (ctypes.c_int64 * len(d))(*d)


def _arr(ps):
    return None if ps is None else (ctypes.c_void_p * len(ps))(*ps)


def _bwd(lib, dims=(300, 256, 1), rows=8, pitch=None, dy=DY, x=X, dx=DX, W=(W0, W1), saved=(Z0,), dW=(G0, G1),
         db=(B0, None), dt=F32, xdt=F32, pdt=F32, act=1, nlayers=None, dims_ptr=True, ws=WS, ws_bytes=1 << 30):
    n = len(dims) - 1 if nlayers is None else nlayers
    return lib.nt_mlp_head_backward(dy, dt, x, xdt, rows, dims[0] if pitch is None else pitch, n, _arr(saved), _arr(W),
                                    pdt, _dims(*dims) if dims_ptr else None, act, 0.1, dx, _arr(dW), _arr(db), ws,
                                    ws_bytes, None)


def test_entries_bounds_and_workspace():
    from notorch_amd import _lib as L

    lib = _lib()
    for name in NAMES:
        assert name in L.EXT_SIGNATURES and name not in L.SIGNATURES and hasattr(lib, name)
    assert lib.nt_abi_version() == L.ABI_VERSION == 8
    ok = lib.nt_mlp_head_train_supported
    assert ok(F32, F32, 2, _dims(300, 256, 1)) == 1 and ok(BF16, F32, 1, _dims(300, 5)) == 1
    # at and one past each bound: 8 layers, in <= 8192, every later width <= 1264 (at least 512, as asked)
    assert ok(F32, F32, 8, _dims(*[8] * 9)) == 1 and ok(F32, F32, 9, _dims(*[8] * 10)) == 0
    assert ok(F32, F32, 2, _dims(8192, 1264, 1264)) == 1 and ok(F32, F32, 2, _dims(8193, 8, 8)) == 0
    assert ok(F32, BF16, 2, _dims(8, 1265, 8)) == 0 and ok(BF16, BF16, 2, _dims(8, 8, 1265)) == 0
    assert ok(F32, F32, 2, _dims(8, 0, 8)) == 0 and ok(5, F32, 1, _dims(8, 8)) == 0 and ok(F32, F32, 1, None) == 0
    # the workspace: dZ of the hidden layers, and fp32 partials per chunk once the rows make more than one chunk
    ws = lib.nt_mlp_head_backward_workspace
    assert ws(8, 1, _dims(300, 5), F32) == 0 and ws(0, 2, _dims(300, 256, 1), F32) == 0
    assert ws(128, 2, _dims(300, 256, 1), F32) == 128 * 256 * 4
    assert ws(128, 2, _dims(300, 256, 1), BF16) == 128 * 256 * 2
    assert ws(293, 2, _dims(300, 256, 1), F32) == 293 * 256 * 4 + 3 * 4 * (256 * 300 + 256 + 256) + 16  # 3 chunks
    assert ws(-1, 2, _dims(300, 256, 1), F32) == -1 and ws(8, 0, _dims(300), F32) == -1
    assert ws(8, 2, _dims(300, 0, 1), F32) == -1 and ws(8, 2, None, F32) == -1 and ws(8, 2, _dims(300, 256, 1), 5) == -1


def test_backward_validates_on_the_host():
    lib = _lib()
    for bad in (dict(dy=None), dict(x=None), dict(W=None), dict(dW=None), dict(dims_ptr=False), dict(W=(W0, None)),
                dict(dW=(None, G1)), dict(saved=None), dict(saved=(None,))):
        assert _bwd(lib, **bad) == EINVAL and b"NULL" in lib.nt_last_error(), bad
    for n in (0, 9, -1):
        assert _bwd(lib, nlayers=n) == EINVAL and b"nlayers" in lib.nt_last_error()
    for bad in (dict(dims=(300, 0, 1)), dict(dims=(-3, 256, 1)), dict(rows=-1)):
        assert _bwd(lib, **bad) == EINVAL and b"bad sizes" in lib.nt_last_error(), bad
    for bad in (dict(dt=5), dict(xdt=2), dict(pdt=7), dict(xdt=BF16), dict(pdt=BF16)):  # fp32 dy: fp32 operands
        assert _bwd(lib, **bad) == EUNSUPPORTED and b"dtype" in lib.nt_last_error(), bad
    assert _bwd(lib, act=8) == EINVAL and b"act" in lib.nt_last_error()
    assert _bwd(lib, pitch=299) == EINVAL and b"pitch" in lib.nt_last_error()
    assert _bwd(lib, pitch=302) == EINVAL and b"16 bytes" in lib.nt_last_error()
    assert _bwd(lib, dims=(300, 1265, 1)) == EUNSUPPORTED and b"LDS" in lib.nt_last_error()
    assert _bwd(lib, dims=(8193, 256, 1)) == EUNSUPPORTED
    need = lib.nt_mlp_head_backward_workspace(8, 2, _dims(300, 256, 1), F32)
    for bad in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws=ctypes.c_void_p(0x1008))):
        assert _bwd(lib, **bad) == EINVAL and b"workspace" in lib.nt_last_error(), bad


def test_forward_train_validates_on_the_host():
    lib = _lib()

    def fwd(rows=8, saved=(Z0,), sdt=F32, odt=F32, xdt=F32, x=X):
        return lib.nt_mlp_head_forward_train(x, xdt, rows, 300, 2, _arr((W0, W1)), _arr((B0, None)), F32,
                                             _dims(300, 256, 1), 1, 0.1, DX, odt, _arr(saved), sdt, None)

    for bad in (dict(x=None), dict(saved=None), dict(saved=(None,))):
        assert fwd(**bad) == EINVAL and b"NULL" in lib.nt_last_error(), bad
    assert fwd(sdt=BF16) == EUNSUPPORTED and fwd(odt=BF16) == EUNSUPPORTED and b"dtype" in lib.nt_last_error()
    assert fwd(rows=0) == OK and fwd(rows=0, odt=BF16, sdt=BF16, xdt=BF16) == OK  # nothing to do: no launch


def test_kernels_binding_validates_before_the_library():
    from notorch_amd import kernels as K

    with pytest.raises(RuntimeError, match="ROCm devices only"):
        K.mlp_head_train_forward(torch.zeros(4, 8), [torch.zeros(2, 8)], [None], (1, 0.0))
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        K.mlp_head_backward(torch.zeros(4, 2), torch.zeros(4, 8), [], [torch.zeros(2, 8)], [False], (1, 0.0))
    assert K.mlp_head_train_supported(torch.float32, torch.float32, [300, 1264, 1]) is True
    assert K.mlp_head_train_supported(torch.float32, torch.float32, [300, 1265, 1]) is False


def test_mlp_train_route_decisions():
    from notorch_amd.nn import mlp

    f32, bf16 = torch.float32, torch.bfloat16
    base = dict(device_type="cuda", chain_ok=True, hooks=False, dropout_active=False, needs_grad=True,
                all_params_grad=True, x_dtype=f32, param_dtype=f32, autocast="", supported=True, train_knob="kernel",
                knob="")

    def route(**over):
        return mlp.mlp_train_route(**{**base, **over})

    assert route() == "kernel" and route(knob="kernel") == "kernel"
    for over in (dict(train_knob=""), dict(train_knob="torch"), dict(knob="torch"), dict(device_type="cpu"),
                 dict(chain_ok=False), dict(hooks=True), dict(dropout_active=True), dict(needs_grad=False),
                 dict(all_params_grad=False), dict(supported=False), dict(param_dtype=None), dict(x_dtype=bf16),
                 dict(param_dtype=bf16), dict(autocast="other"), dict(autocast="bf16", x_dtype=torch.float16),
                 dict(autocast="bf16", param_dtype=torch.float64)):
        assert route(**over) == "torch", over
    for x_dtype in (f32, bf16):
        for param_dtype in (f32, bf16):
            assert route(autocast="bf16", x_dtype=x_dtype, param_dtype=param_dtype) == "kernel"
