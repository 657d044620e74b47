"""CPU: nt_rank_metric_long* (include/notorch_amd_train.h, csrc/rank_metric_long.hip) are exported and bound, size
their workspace and validate on the host before any device call.  Fake, aligned pointers only: no device call
is reached (a launch on this CPU-only path would answer NT_EHIP = 2, never the statuses asserted here)."""
import ctypes

import pytest
import torch

OK, EINVAL, EUNSUPPORTED = 0, 1, 3
NAMES = ("nt_rank_metric_long_max_n", "nt_rank_metric_long_workspace", "nt_rank_metric_long")
TILE = 4096


def _lib():
    from notorch_amd import _lib

    return _lib.load()


def _p(i):
    return ctypes.c_void_p(0x1000 * (i + 1))


SCORES, TARGETS, MASK, OUT, WS = (_p(i) for i in range(5))


def _call(lib, n=8192, t=1, **over):
    a = dict(scores=SCORES, targets=TARGETS, mask=None, out=OUT, ws=WS, ws_bytes=1 << 62)
    a.update(over)
    return lib.nt_rank_metric_long(a["scores"], a["targets"], a["mask"], n, t, a["out"], a["ws"], a["ws_bytes"], None)


def test_entry_points_are_bound_and_exported():
    from notorch_amd import _lib

    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXT_SIGNATURES and name not in _lib.SIGNATURES
        assert hasattr(lib, name)
        assert list(getattr(lib, name).argtypes) == list(_lib.EXT_SIGNATURES[name][1])
    assert lib.nt_abi_version() == _lib.ABI_VERSION == 8


def test_limit_and_workspace_query():
    from notorch_amd import kernels as K

    lib = _lib()
    assert lib.nt_rank_metric_long_max_n() == 1 << 24 == K.rank_metric_long_max_n()
    ws = lib.nt_rank_metric_long_workspace
    for n, t in ((-1, 1), (1, -1), (8, 1 << 31), (1 << 24, 1 << 19), (1 << 62, 1), ((1 << 63) - 1, 3)):
        assert ws(n, t) == -1, (n, t)
    assert ws(0, 5) == 0 and ws(5, 0) == 0
    assert 0 < ws(1, 1) == ws(TILE, 1) < ws(TILE + 1, 1) == ws(2 * TILE, 1)  # by whole tiles
    assert ws(TILE, 3) == 3 * ws(TILE, 1)
    # two buffers of 8-byte words and the tile partials, carries and terms
    assert ws(TILE + 1, 1) >= 2 * 2 * TILE * 8
    for n, t in ((1, 1), (TILE + 1, 1), (20480, 3), (1 << 24, 1), (12345, 7)):
        assert ws(n, t) > 0 and ws(n, t) % 16 == 0, (n, t)


def test_validates_on_the_host():
    lib = _lib()
    for null in ("scores", "targets", "out"):
        assert _call(lib, **{null: None}) == EINVAL and b"NULL" in lib.nt_last_error(), null
    for n, t in ((-1, 1), (8192, -1), (8192, 1 << 31), (1 << 24, 1 << 19), (1 << 62, 1)):
        assert _call(lib, n=n, t=t) == EINVAL and b"bad sizes" in lib.nt_last_error(), (n, t)
    top = lib.nt_rank_metric_long_max_n()
    assert _call(lib, n=top + 1) == EUNSUPPORTED
    assert b"nt_rank_metric_long_max_n" in lib.nt_last_error() and str(top).encode() in lib.nt_last_error()
    # the workspace: required, whole and aligned, once there is something to rank
    for n, t in ((8192, 1), (1, 1), (TILE + 1, 3)):
        need = lib.nt_rank_metric_long_workspace(n, t)
        assert _call(lib, n=n, t=t, ws=None, ws_bytes=need) == EINVAL and b"workspace" in lib.nt_last_error()
        assert _call(lib, n=n, t=t, ws_bytes=need - 1) == EINVAL and b"workspace" in lib.nt_last_error()
        assert _call(lib, n=n, t=t, ws=ctypes.c_void_p(0x9008), ws_bytes=need) == EINVAL
        assert b"workspace" in lib.nt_last_error()
    # no columns: no launch, whatever else is passed
    assert _call(lib, n=8192, t=0, mask=MASK, ws=None, ws_bytes=0) == OK
    assert _call(lib, n=0, t=0, ws=None, ws_bytes=0) == OK


def test_binding_validates_before_the_library(monkeypatch):
    from notorch_amd import _lib
    from notorch_amd import kernels as K

    def _fail():
        raise AssertionError("the binding reached the library")

    monkeypatch.setattr(_lib, "load", _fail)
    assert "rank_metric_long" in K.__all__ and "rank_metric_long_max_n" in K.__all__
    p, y = torch.zeros(5000, 2), torch.zeros(5000, 2)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        K.rank_metric_long(p, y)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        K.rank_metric_long(p, y, torch.ones(5000, 2, dtype=torch.bool), torch.zeros(64, dtype=torch.uint8))


def test_cpu_and_fp64_inputs_stay_on_torch_ops(monkeypatch):
    from notorch_amd import kernels as K
    from notorch_amd.nn import metrics as M

    def _fail(*args, **kwargs):
        raise AssertionError("a CPU tensor reached a kernel binding")

    monkeypatch.setattr(K, "rank_metric_long", _fail)
    monkeypatch.setattr(K, "rank_metric", _fail)
    monkeypatch.setenv("NT_LOSS", "kernel")
    gen = torch.Generator().manual_seed(5)
    s, y = torch.randn(5000, 1, generator=gen), (torch.rand(5000, 1, generator=gen) < 0.4).float()
    want = M.rank_metric_torch(s.double(), y.double())[0, 0].item()
    assert abs(M.AUROC("multilabel")(s, y).item() - want) <= 1e-5
    assert abs(M.AUROC("multilabel")(s.double(), y.double()).item() - want) <= 1e-12
    # the default bound is 0 (off) or one of the sizes timed for it
    assert M.RANK_LONG_DEFAULT_MAX_N in (0, 4097, 12288, 49152, 1 << 17, 1 << 20)
