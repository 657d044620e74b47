"""CPU: the training-side additions of include/notorch_amd_train.h are exported by the library and
bound from _lib.EXT_SIGNATURES; the pinned v8 boundary of include/notorch_amd.h does not move.
Only host-side argument validation is exercised (no device call is reached)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "notorch_amd_train.h")


def header_functions():
    txt = open(HEADER).read()
    return re.findall(r"^NT_API\s+[\w\s\*]+?\b(nt_\w+)\s*\(", txt, flags=re.M)


def test_train_header_is_exported_and_bound():
    from notorch_amd import _lib

    names = header_functions()
    assert "nt_embed_bag_backward" in names and "nt_embed_bag_backward_workspace" in names
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} not built (run make)")
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name), name
        assert list(getattr(lib, name).argtypes) == list(_lib.EXT_SIGNATURES[name][1])
    assert set(_lib.EXT_SIGNATURES) == set(names)  # the table covers exactly that header
    assert not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)


def test_abi_version_unchanged():
    from notorch_amd import _lib

    assert _lib.load().nt_abi_version() == _lib.ABI_VERSION == 8


def test_workspace_query():
    from notorch_amd import _lib

    lib = _lib.load()
    ws = lib.nt_embed_bag_backward_workspace
    assert ws(-1, 42, 300) == -1 and ws(10, -1, 300) == -1 and ws(10, 42, 0) == -1
    one = 42 * 300 * 4
    assert ws(0, 42, 300) == one  # n = 0 still owns one partial table (of zeros)
    assert ws(64, 42, 300) == one and ws(65, 42, 300) == 2 * one
    # the number of partial tables is bounded however many rows there are
    assert ws(10**9, 42, 300) == ws(10**8, 42, 300) <= 1024 * one
    assert ws(10, 0, 300) > 0


def _call(lib, dX, ld, n_dx, idx, n, k, ntypes, h, seg, perm, dt, odt, out, ws, ws_bytes):
    return lib.nt_embed_bag_backward(dX, ld, n_dx, idx, n, k, ntypes, h, seg, perm, dt, odt, out, ws, ws_bytes, None)


def test_embed_bag_backward_validates_on_the_host():
    from notorch_amd import _lib

    lib = _lib.load()
    fake = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(6)]
    dX, idx, seg, perm, out, ws = fake
    need = lib.nt_embed_bag_backward_workspace(100, 42, 300)
    # NULL pointers: status 1 with a message
    rc = _call(lib, None, 300, 100, None, 100, 7, 42, 300, None, None, 0, 0, None, None, 0)
    assert rc == 1 and b"NULL" in lib.nt_last_error()
    rc = _call(lib, dX, 300, 100, idx, 100, 7, 42, 300, None, None, 0, 0, None, ws, need)
    assert rc == 1 and b"NULL" in lib.nt_last_error()
    rc = _call(lib, dX, 300, 100, None, 100, 7, 42, 300, None, None, 0, 0, out, ws, need)
    assert rc == 1 and b"NULL" in lib.nt_last_error()
    rc = _call(lib, dX, 300, 200, idx, 100, 7, 42, 300, seg, None, 0, 0, out, ws, need)  # a CSR without perm
    assert rc == 1 and b"NULL" in lib.nt_last_error()
    # unknown dtype codes: status 3
    assert _call(lib, dX, 300, 100, idx, 100, 7, 42, 300, None, None, 7, 0, out, ws, need) == 3
    assert _call(lib, dX, 300, 100, idx, 100, 7, 42, 300, None, None, 0, 7, out, ws, need) == 3
    assert b"dtype" in lib.nt_last_error()
    # negative / inconsistent sizes: status 1
    for bad in (dict(n=-1, n_dx=-1), dict(k=-1), dict(ntypes=-1), dict(h=0), dict(ld=299), dict(n_dx=99)):
        a = dict(ld=300, n_dx=100, n=100, k=7, ntypes=42, h=300)
        a.update(bad)
        rc = _call(lib, dX, a["ld"], a["n_dx"], idx, a["n"], a["k"], a["ntypes"], a["h"], None, None, 0, 0, out, ws,
                   need)
        assert rc == 1 and b"bad sizes" in lib.nt_last_error(), bad
    # a workspace that is missing or too small: status 1, and the message names the workspace
    rc = _call(lib, dX, 300, 100, idx, 100, 7, 42, 300, None, None, 0, 1, out, ws, need - 1)
    assert rc == 1 and b"workspace" in lib.nt_last_error()
    rc = _call(lib, dX, 300, 100, idx, 100, 7, 42, 300, seg, perm, 1, 0, out, None, need)
    assert rc == 1 and b"workspace" in lib.nt_last_error()
    # a row that does not fit the LDS partial: unsupported, said so
    rc = _call(lib, dX, 30000, 100, idx, 100, 7, 42, 30000, None, None, 0, 0, out, ws, 1 << 40)
    assert rc == 3 and b"LDS" in lib.nt_last_error()


def test_kernels_binding_validates_before_the_library():
    """kernels.embed_bag_backward rejects CPU tensors up front (no device here)."""
    import torch

    from notorch_amd import kernels as K

    with pytest.raises(RuntimeError, match="ROCm devices only"):
        K.embed_bag_backward(torch.zeros(4, 8), torch.zeros(4, 2, dtype=torch.int64), 3)
