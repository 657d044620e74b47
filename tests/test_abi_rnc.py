"""CPU: nt_rnc_max_n / nt_rnc_rank (include/notorch_amd_train.h, csrc/rnc.hip) are exported and bound, and
nt_rnc_rank validates on the host before any device call.  Fake, aligned pointers only: no device call
is reached (a launch on this CPU-only path would answer NT_EHIP = 2, never the statuses asserted here)."""
import ctypes

import pytest
import torch

OK, EINVAL, EUNSUPPORTED = 0, 1, 3
NAMES = ("nt_rnc_max_n", "nt_rnc_rank")


def _lib():
    from notorch_amd import _lib

    return _lib.load()


def _p(i):
    return ctypes.c_void_p(0x1000 * (i + 1))


def _rank(lib, sim, dist, n, temp=2.0, eps=1e-6, row_nll=None, dsim=None):
    return lib.nt_rnc_rank(sim, dist, n, temp, eps, row_nll, dsim, None)


def test_entry_points_are_bound_and_exported():
    from notorch_amd import _lib

    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXT_SIGNATURES and name not in _lib.SIGNATURES
        assert hasattr(lib, name)
        assert list(getattr(lib, name).argtypes) == list(_lib.EXT_SIGNATURES[name][1])
    assert lib.nt_abi_version() == _lib.ABI_VERSION == 8


def test_max_n_covers_the_bench_batch():
    from notorch_amd import kernels as K

    assert _lib().nt_rnc_max_n() >= 4096
    assert K.rnc_max_n() == _lib().nt_rnc_max_n()


def test_rank_validates_on_the_host():
    lib = _lib()
    sim, dist, nll, dsim = (_p(i) for i in range(4))
    n = 64
    for null in ("sim", "dist", "row_nll"):
        args = dict(sim=sim, dist=dist, row_nll=nll)
        args[null] = None
        rc = _rank(lib, args["sim"], args["dist"], n, row_nll=args["row_nll"], dsim=dsim)
        assert rc == EINVAL and b"NULL" in lib.nt_last_error(), null
    assert _rank(lib, sim, dist, -1, row_nll=nll) == EINVAL and b"n < 0" in lib.nt_last_error()
    for temp in (0.0, -2.0, float("inf"), float("nan")):
        assert _rank(lib, sim, dist, n, temp=temp, row_nll=nll) == EINVAL, temp
        assert b"temp" in lib.nt_last_error()
    too_many = lib.nt_rnc_max_n() + 1
    assert _rank(lib, sim, dist, too_many, row_nll=nll, dsim=dsim) == EUNSUPPORTED
    assert b"nt_rnc_max_n" in lib.nt_last_error() and str(too_many - 1).encode() in lib.nt_last_error()
    # nothing to do: no launch, with and without a gradient buffer
    assert _rank(lib, sim, dist, 0, row_nll=nll) == OK
    assert _rank(lib, sim, dist, 0, row_nll=nll, dsim=dsim) == OK


def test_binding_validates_before_the_library(monkeypatch):
    from notorch_amd import _lib
    from notorch_amd import kernels as K

    def _fail():
        raise AssertionError("the binding reached the library")

    monkeypatch.setattr(_lib, "load", _fail)
    sim, dist = torch.zeros(6, 6), torch.zeros(6, 6)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        K.rnc_rank(sim, dist, 2.0, 1e-6, True)
