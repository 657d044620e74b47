"""CPU: nt_node_scores_mixed / nt_softmax_pool_backward_mixed (include/notorch_amd_train.h, csrc/mixed.hip),
the attention readouts for bf16 rows with fp32 keys, validate on the host before any device call, and
the kernels.py bindings reject bad operands before the library is reached.  Fake, aligned pointers only:
no device call is reached (a launch on this CPU-only path would answer NT_EHIP = 2, never the statuses
asserted here)."""
import ctypes

import pytest
import torch

F32, BF16 = 0, 1
OK, EINVAL, EUNSUPPORTED = 0, 1, 3
NAMES = ("nt_node_scores_mixed", "nt_softmax_pool_backward_mixed")


def _lib():
    from notorch_amd import _lib

    return _lib.load()


def _p(i):
    return ctypes.c_void_p(0x1000 * (i + 1))


def test_entry_points_are_bound_and_exported():
    from notorch_amd import _lib

    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXT_SIGNATURES and name not in _lib.SIGNATURES
        assert hasattr(lib, name)
        assert list(getattr(lib, name).argtypes) == list(_lib.EXT_SIGNATURES[name][1])
    # the plain entry points' argument lists, one for one
    assert _lib.EXT_SIGNATURES["nt_node_scores_mixed"] == _lib.SIGNATURES["nt_node_scores"]
    assert _lib.EXT_SIGNATURES["nt_softmax_pool_backward_mixed"] == _lib.SIGNATURES["nt_softmax_pool_backward"]
    assert lib.nt_abi_version() == _lib.ABI_VERSION == 8


def _scores(lib, X, n, h, a, a_bias, Q, node_seg, sqrt_key, dtype, s):
    return lib.nt_node_scores_mixed(X, n, h, a, a_bias, Q, node_seg, sqrt_key, dtype, s, None)


def test_node_scores_mixed_validates_on_the_host():
    lib = _lib()
    X, a, b, Q, seg, s = (_p(i) for i in range(6))
    n, h = 10, 64
    # NULL pointers
    assert _scores(lib, None, n, h, a, b, None, None, 1.0, BF16, s) == EINVAL and b"NULL" in lib.nt_last_error()
    assert _scores(lib, X, n, h, a, b, None, None, 1.0, BF16, None) == EINVAL and b"NULL" in lib.nt_last_error()
    assert _scores(lib, X, n, h, None, None, Q, None, 8.0, BF16, s) == EINVAL and b"node_seg" in lib.nt_last_error()
    assert _scores(lib, X, n, h, None, None, Q, seg, 0.0, BF16, s) == EINVAL and b"sqrt_key" in lib.nt_last_error()
    # both keys, or neither
    assert _scores(lib, X, n, h, a, b, Q, seg, 8.0, BF16, s) == EINVAL and b"exactly one" in lib.nt_last_error()
    assert _scores(lib, X, n, h, None, None, None, seg, 8.0, BF16, s) == EINVAL and b"exactly one" in lib.nt_last_error()
    # bad sizes
    assert _scores(lib, X, -1, h, a, b, None, None, 1.0, BF16, s) == EINVAL and b"bad sizes" in lib.nt_last_error()
    assert _scores(lib, X, n, 0, a, b, None, None, 1.0, BF16, s) == EINVAL and b"bad sizes" in lib.nt_last_error()
    # X is bf16 here: NT_F32 (the plain entry point's case) and unknown codes are unsupported, said so
    for code in (F32, 7, -1):
        assert _scores(lib, X, n, h, a, b, None, None, 1.0, code, s) == EUNSUPPORTED
        assert b"dtype" in lib.nt_last_error() and b"NT_BF16" in lib.nt_last_error()
    # the dtype is checked first, as in nt_node_scores
    assert _scores(lib, None, -1, 0, None, None, None, None, 0.0, 7, None) == EUNSUPPORTED
    # nothing to do
    assert _scores(lib, None, 0, h, a, None, None, None, 1.0, BF16, None) == OK
    assert _scores(lib, None, 0, h, None, None, Q, seg, 8.0, BF16, None) == OK


def _backward(lib, a=None, Q=None, nseg=4, n=10, h=64, sqrt_key=1.0, dtype=BF16, null=()):
    names = ("X", "scores", "seg_ptr", "perm", "node_seg", "out", "dout", "stats", "dX", "ds", "P")
    p = {nm: (None if nm in null else _p(i)) for i, nm in enumerate(names)}
    return lib.nt_softmax_pool_backward_mixed(
        p["X"], p["scores"], p["seg_ptr"], p["perm"], p["node_seg"], nseg, n, h, p["out"], p["dout"], a, Q,
        sqrt_key, dtype, p["stats"], p["dX"], p["ds"], p["P"], None)


def test_softmax_pool_backward_mixed_validates_on_the_host():
    lib = _lib()
    a, Q = _p(20), _p(21)
    for nm in ("X", "scores", "seg_ptr", "node_seg", "out", "dout", "stats", "dX", "ds", "P"):
        assert _backward(lib, a=a, null=(nm,)) == EINVAL and b"NULL" in lib.nt_last_error(), nm
        assert _backward(lib, Q=Q, sqrt_key=8.0, null=(nm,)) == EINVAL and b"NULL" in lib.nt_last_error(), nm
    assert _backward(lib, a=a, Q=Q) == EINVAL and b"exactly one" in lib.nt_last_error()
    assert _backward(lib) == EINVAL and b"exactly one" in lib.nt_last_error()
    assert _backward(lib, Q=Q, sqrt_key=0.0) == EINVAL and b"sqrt_key" in lib.nt_last_error()
    for bad in (dict(nseg=-1), dict(n=-1), dict(h=0)):
        assert _backward(lib, a=a, **bad) == EINVAL and b"bad sizes" in lib.nt_last_error(), bad
    for code in (F32, 7, -1):
        assert _backward(lib, a=a, dtype=code) == EUNSUPPORTED
        assert b"dtype" in lib.nt_last_error() and b"NT_BF16" in lib.nt_last_error()
    assert _backward(lib, dtype=7, nseg=-1, null=("X",)) == EUNSUPPORTED  # the dtype is checked first
    # nothing to do
    assert _backward(lib, a=a, nseg=0, n=0, null=("X", "scores", "seg_ptr", "node_seg", "out", "dout", "stats",
                                                  "dX", "ds", "P")) == OK


@pytest.fixture
def no_library(monkeypatch):
    """The bindings below must raise before they reach the library."""
    from notorch_amd import _lib

    def _fail():
        raise AssertionError("the binding reached the library")

    monkeypatch.setattr(_lib, "load", _fail)


def test_node_scores_mixed_binding_validates_before_the_library(no_library):
    from notorch_amd import kernels as K

    bf, h = torch.bfloat16, 8
    X = torch.zeros(5, h, dtype=bf)
    a, bias = torch.zeros(h), torch.zeros(1)
    Q, seg = torch.zeros(2, h), torch.zeros(5, dtype=torch.int64)
    with pytest.raises(TypeError, match="X must be bfloat16"):  # an fp32 X: the plain entry point's case
        K.node_scores_mixed(X.float(), a=a, a_bias=bias)
    for kw in (dict(a=a.to(bf)), dict(a=a, a_bias=bias.to(bf)), dict(Q=Q.to(bf), node_seg=seg)):
        with pytest.raises(TypeError, match="must be float32 on the mixed readout path"):  # a bf16 key
            K.node_scores_mixed(X, **kw)
    with pytest.raises(ValueError, match="h entries"):
        K.node_scores_mixed(X, a=torch.zeros(h + 1))
    with pytest.raises(ValueError, match="one entry"):
        K.node_scores_mixed(X, a=a, a_bias=torch.zeros(2))
    with pytest.raises(RuntimeError, match="Q must be b x 8"):
        K.node_scores_mixed(X, Q=torch.zeros(2, h + 1), node_seg=seg)
    with pytest.raises(ValueError, match="one entry per row"):
        K.node_scores_mixed(X, Q=Q, node_seg=seg[:4])
    with pytest.raises(ValueError, match="batch_node_index"):
        K.node_scores_mixed(X, Q=Q)
    with pytest.raises(ValueError, match="X must be contiguous"):
        K.node_scores_mixed(torch.zeros(5, 2 * h, dtype=bf)[:, :h], a=a)
    with pytest.raises(ValueError, match="a must be contiguous"):
        K.node_scores_mixed(X, a=torch.zeros(2 * h)[::2])
    with pytest.raises(ValueError, match="exactly one"):
        K.node_scores_mixed(X, a=a, Q=Q, node_seg=seg)
    with pytest.raises(ValueError, match="exactly one"):
        K.node_scores_mixed(X)
    with pytest.raises(RuntimeError, match="ROCm devices only"):  # all valid but on the CPU
        K.node_scores_mixed(X, a=a, a_bias=bias)


def test_softmax_pool_backward_mixed_binding_validates_before_the_library(no_library):
    from notorch_amd import kernels as K

    bf, h, n, B = torch.bfloat16, 8, 5, 2
    X = torch.zeros(n, h, dtype=bf)
    s = torch.zeros(n)
    ptr = torch.zeros(B + 1, dtype=torch.int32)
    seg = torch.zeros(n, dtype=torch.int64)
    out = torch.zeros(B, h, dtype=bf)
    a, Q = torch.zeros(h), torch.zeros(B, h)

    def call(X=X, s=s, ptr=ptr, seg=seg, out=out, dout=out, **kw):
        return K.softmax_pool_backward_mixed(X, s, ptr, None, seg, B, out, dout, **kw)

    with pytest.raises(TypeError, match="X must be bfloat16"):
        call(X=X.float(), a=a)
    with pytest.raises(TypeError, match="must be float32 on the mixed readout path"):
        call(a=a.to(bf))
    with pytest.raises(TypeError, match="must be float32 on the mixed readout path"):
        call(Q=Q.to(bf))
    with pytest.raises(TypeError, match="dout must be bfloat16"):
        call(dout=out.float(), a=a)
    with pytest.raises(ValueError, match="h entries"):
        call(a=torch.zeros(h - 1))
    with pytest.raises(RuntimeError, match="Q must be b x 8"):
        call(Q=torch.zeros(B, h + 8))
    with pytest.raises(ValueError, match="X must be contiguous"):
        call(X=torch.zeros(n, 2 * h, dtype=bf)[:, :h], a=a)
    with pytest.raises(ValueError, match="out must be nseg x h"):
        call(out=torch.zeros(B + 1, h, dtype=bf), a=a)
    with pytest.raises(ValueError, match="scores"):
        call(s=torch.zeros(n + 1), a=a)
    with pytest.raises(ValueError, match="seg_ptr"):
        call(ptr=torch.zeros(B, dtype=torch.int32), a=a)
    with pytest.raises(ValueError, match="exactly one"):
        call(a=a, Q=Q)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        call(a=a)
