"""CPU: the mixed-precision entry points of include/notorch_amd_train.h (csrc/mixed.hip) validate on
the host before any device call.  Fake, aligned pointers only: no device call is reached (a launch on
this CPU-only path would answer NT_EHIP = 2, never the statuses asserted here)."""
import ctypes

NULL_ARR = None
F32, BF16 = 0, 1
RULE = b"h <= 512, or h % 8 == 0 and h <= 8192"


def _lib():
    from notorch_amd import _lib

    return _lib.load()


def _arr(n, base=0x10000, none_at=()):
    vals = [None if i in none_at else base + 0x1000 * i for i in range(n)]
    return (ctypes.c_void_p * n)(*vals)


def _pack(lib, W, n, h, dt, Wp, WpT=None, b=None, b16=None):
    return lib.nt_dmpnn_pack_weights_mixed(W, n, h, dt, Wp, WpT, b, b16, None)


def test_entry_points_are_bound():
    from notorch_amd import _lib

    for name in ("nt_dmpnn_pack_weights_mixed", "nt_dmpnn_init_mixed", "nt_dmpnn_init_embed_mixed"):
        assert name in _lib.EXT_SIGNATURES and name not in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert _lib.load().nt_abi_version() == 8


def test_pack_weights_mixed_validates_on_the_host():
    lib = _lib()
    n, h = 3, 64
    W, Wp, WpT, b, b16 = (_arr(n, 0x10000 * (k + 1)) for k in range(5))
    # NULL pointer arrays and NULL entries: status 1
    assert _pack(lib, None, n, h, F32, Wp) == 1 and b"NULL" in lib.nt_last_error()
    assert _pack(lib, W, n, h, F32, None) == 1 and b"NULL" in lib.nt_last_error()
    assert _pack(lib, _arr(n, none_at=(1,)), n, h, F32, Wp) == 1 and b"NULL" in lib.nt_last_error()
    assert _pack(lib, W, n, h, F32, _arr(n, none_at=(2,))) == 1 and b"NULL" in lib.nt_last_error()
    assert _pack(lib, W, n, h, F32, Wp, _arr(n, none_at=(0,))) == 1 and b"NULL" in lib.nt_last_error()
    assert _pack(lib, W, n, h, F32, Wp, WpT, b, None) == 1 and b"NULL" in lib.nt_last_error()
    assert _pack(lib, W, n, h, F32, Wp, WpT, b, _arr(n, none_at=(1,))) == 1 and b"NULL" in lib.nt_last_error()
    # a misaligned image pointer: status 1
    assert _pack(lib, W, n, h, F32, _arr(n, 0x20008)) == 1 and b"misaligned" in lib.nt_last_error()
    # unknown source dtype code: status 3
    assert _pack(lib, W, n, h, 7, Wp, WpT, b, b16) == 3 and b"dtype" in lib.nt_last_error()
    # nlayers outside 1..16: status 1
    W17, Wp17 = _arr(17), _arr(17, 0x80000)
    assert _pack(lib, W17, 0, h, F32, Wp17) == 1 and b"bad sizes" in lib.nt_last_error()
    assert _pack(lib, W17, 17, h, F32, Wp17) == 1 and b"bad sizes" in lib.nt_last_error()
    assert _pack(lib, W, n, 0, F32, Wp) == 1 and b"bad sizes" in lib.nt_last_error()
    # a hidden size outside the bf16 rule: status 3, the message names the rule
    for dt in (F32, BF16):
        assert _pack(lib, W, n, 516, dt, Wp, WpT, b, b16) == 3 and RULE in lib.nt_last_error()
    assert _pack(lib, W, n, 8200, F32, Wp) == 3 and RULE in lib.nt_last_error()


def _init(lib, Xv, Xe, src, seg, perm, V, E, h, H0, S, act=1, reduce=0):
    return lib.nt_dmpnn_init_mixed(Xv, Xe, src, seg, perm, V, E, h, act, 0.0, reduce, H0, S, None)


def test_init_mixed_validates_on_the_host():
    lib = _lib()
    Xv, Xe, src, seg, perm, H0, S = (ctypes.c_void_p(0x1000 * (i + 1)) for i in range(7))
    V, E, h = 10, 20, 64
    for bad in ("Xv", "Xe", "src", "H0"):
        a = dict(Xv=Xv, Xe=Xe, src=src, H0=H0)
        a[bad] = None
        rc = _init(lib, a["Xv"], a["Xe"], a["src"], seg, perm, V, E, h, a["H0"], S)
        assert rc == 1 and b"NULL" in lib.nt_last_error(), bad
    # the fused aggregation without its CSR
    assert _init(lib, Xv, Xe, src, None, perm, V, E, h, H0, S) == 1 and b"NULL" in lib.nt_last_error()
    assert _init(lib, Xv, Xe, src, seg, None, V, E, h, H0, S) == 1 and b"NULL" in lib.nt_last_error()
    # bad codes and sizes: status 1
    assert _init(lib, Xv, Xe, src, seg, perm, V, E, h, H0, S, reduce=9) == 1 and b"reduce" in lib.nt_last_error()
    assert _init(lib, Xv, Xe, src, seg, perm, V, E, h, H0, S, act=99) == 1 and b"act" in lib.nt_last_error()
    assert _init(lib, Xv, Xe, src, seg, perm, -1, E, h, H0, S) == 1 and b"bad sizes" in lib.nt_last_error()
    assert _init(lib, Xv, Xe, src, seg, perm, V, E, 0, H0, S) == 1 and b"bad sizes" in lib.nt_last_error()
    # h outside the bf16 rule: status 3 with the rule
    assert _init(lib, Xv, Xe, src, seg, perm, V, E, 516, H0, S) == 3 and RULE in lib.nt_last_error()


def _init_embed(lib, Tv, nv, vt, kv, Te, ne, et, ke, src, seg, perm, V, E, h, H0, S, act=1, reduce=0):
    return lib.nt_dmpnn_init_embed_mixed(Tv, nv, vt, kv, Te, ne, et, ke, src, seg, perm, V, E, h, act, 0.0, reduce,
                                         H0, S, None)


def test_init_embed_mixed_validates_on_the_host():
    lib = _lib()
    Tv, vt, Te, et, src, seg, perm, H0, S = (ctypes.c_void_p(0x1000 * (i + 1)) for i in range(9))
    V, E, h = 10, 20, 64
    for bad in ("Tv", "vt", "Te", "et", "src", "H0"):
        a = dict(Tv=Tv, vt=vt, Te=Te, et=et, src=src, H0=H0)
        a[bad] = None
        rc = _init_embed(lib, a["Tv"], 42, a["vt"], 7, a["Te"], 13, a["et"], 2, a["src"], seg, perm, V, E, h,
                         a["H0"], S)
        assert rc == 1 and b"NULL" in lib.nt_last_error(), bad
    rc = _init_embed(lib, Tv, 42, vt, 7, Te, 13, et, 2, src, None, perm, V, E, h, H0, S)
    assert rc == 1 and b"NULL" in lib.nt_last_error()
    rc = _init_embed(lib, Tv, 42, vt, -1, Te, 13, et, 2, src, seg, perm, V, E, h, H0, S)
    assert rc == 1 and b"bad sizes" in lib.nt_last_error()
    rc = _init_embed(lib, Tv, 42, vt, 7, Te, 13, et, 2, src, seg, perm, V, E, h, H0, S, reduce=-1)
    assert rc == 1 and b"reduce" in lib.nt_last_error()
    rc = _init_embed(lib, Tv, 42, vt, 7, Te, 13, et, 2, src, seg, perm, V, E, 516, H0, S)
    assert rc == 3 and RULE in lib.nt_last_error()


def test_kernels_bindings_validate_before_the_library():
    """The tensor-level wrappers reject CPU tensors and bad sizes up front (no device here)."""
    import pytest
    import torch

    from notorch_amd import kernels as K

    with pytest.raises(RuntimeError, match="ROCm devices only"):
        K.dmpnn_init_mixed(torch.zeros(4, 8), torch.zeros(6, 8), torch.zeros(6, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        K.pack_weights_mixed([torch.zeros(8, 8)])
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        K.dmpnn_init_embed_mixed(torch.zeros(4, 8), torch.zeros(3, 2, dtype=torch.int64), torch.zeros(4, 8),
                                 torch.zeros(5, 1, dtype=torch.int64), torch.zeros(5, dtype=torch.int64))
    assert K.bf16_h_supported(36) and K.bf16_h_supported(512) and K.bf16_h_supported(528) and K.bf16_h_supported(8192)
    assert not K.bf16_h_supported(516) and not K.bf16_h_supported(8200) and not K.bf16_h_supported(0)
