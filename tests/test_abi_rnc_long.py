"""CPU: nt_rnc_long_max_n / nt_rnc_rank_long (include/notorch_amd_train.h, csrc/rnc_long.hip) are exported
and bound, nt_rnc_rank_long validates on the host before any device call, and RankNContrastLoss's route is
decided by a pure function of (N, device type, dtypes, NT_RNC).  Fake, aligned pointers only: no device
call is reached (a launch on this CPU-only path would answer NT_EHIP = 2, never the statuses asserted
here)."""
import ctypes

import pytest
import torch

OK, EINVAL, EUNSUPPORTED = 0, 1, 3
NAMES = ("nt_rnc_long_max_n", "nt_rnc_rank_long")
F32, F64 = torch.float32, torch.float64


def _lib():
    from notorch_amd import _lib

    return _lib.load()


def _p(i):
    return ctypes.c_void_p(0x1000 * (i + 1))


def _rank(lib, sim, dist, n, temp=2.0, eps=1e-6, row_nll=None, dsim=None):
    return lib.nt_rnc_rank_long(sim, dist, n, temp, eps, row_nll, dsim, None)


def test_entry_points_are_bound_and_exported():
    from notorch_amd import _lib
    from notorch_amd import kernels as K

    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXT_SIGNATURES and name not in _lib.SIGNATURES
        assert hasattr(lib, name)
        assert list(getattr(lib, name).argtypes) == list(_lib.EXT_SIGNATURES[name][1])
    assert list(lib.nt_rnc_rank_long.argtypes) == list(lib.nt_rnc_rank.argtypes)
    assert lib.nt_abi_version() == _lib.ABI_VERSION == 8
    assert "rnc_rank_long" in K.__all__ and "rnc_long_max_n" in K.__all__


def test_max_n_is_16384_and_the_short_limit_stays():
    from notorch_amd import kernels as K

    assert _lib().nt_rnc_long_max_n() == 16384
    assert K.rnc_long_max_n() == 16384
    assert K.rnc_max_n() == _lib().nt_rnc_max_n() == 4096


def test_rank_long_validates_on_the_host():
    lib = _lib()
    sim, dist, nll, dsim = (_p(i) for i in range(4))
    n = 5000
    for null in ("sim", "dist", "row_nll"):
        args = dict(sim=sim, dist=dist, row_nll=nll)
        args[null] = None
        rc = _rank(lib, args["sim"], args["dist"], n, row_nll=args["row_nll"], dsim=dsim)
        assert rc == EINVAL and b"NULL" in lib.nt_last_error(), null
    assert _rank(lib, sim, dist, -1, row_nll=nll) == EINVAL and b"n < 0" in lib.nt_last_error()
    for temp in (0.0, -2.0, float("inf"), float("nan")):
        assert _rank(lib, sim, dist, n, temp=temp, row_nll=nll) == EINVAL, temp
        assert b"temp" in lib.nt_last_error()
    too_many = lib.nt_rnc_long_max_n() + 1
    assert _rank(lib, sim, dist, too_many, row_nll=nll, dsim=dsim) == EUNSUPPORTED
    assert b"nt_rnc_long_max_n" in lib.nt_last_error() and b"16384" in lib.nt_last_error()
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
        K.rnc_rank_long(sim, dist, 2.0, 1e-6, True)


def test_route_is_a_pure_function_of_size_device_dtypes_and_knob():
    from notorch_amd import kernels as K
    from notorch_amd.nn.loss import rnc

    short, long_max, default = K.rnc_max_n(), K.rnc_long_max_n(), rnc.RNC_LONG_DEFAULT_MAX_N
    assert default == 0 or short < default <= long_max

    def route(n, knob="", device="cuda", sim=F32, dist=F32):
        return rnc.rnc_route(n, device, sim, dist, knob)

    assert route(2) == "kernel" and route(short) == "kernel"
    if default > short:
        assert route(short + 1) == "long" and route(default) == "long"
    assert route(max(default, short) + 1) == "torch"
    assert route(long_max + 1) == "torch"
    # NT_RNC=kernel: as far as the kernels reach
    assert route(short, "kernel") == "kernel"
    assert route(short + 1, "kernel") == "long" and route(long_max, "kernel") == "long"
    assert route(long_max + 1, "kernel") == "torch"
    # NT_RNC=torch, fp64 on either side, a CPU tensor: torch at every size, whatever the knob
    for n in (2, short, short + 1, long_max, long_max + 1):
        assert route(n, "torch") == "torch"
        for knob in ("", "kernel"):
            assert route(n, knob, sim=F64) == "torch" and route(n, knob, dist=F64) == "torch"
            assert route(n, knob, device="cpu") == "torch"
    # the narrow dtypes are widened onto the kernels
    assert route(short + 1, "kernel", sim=torch.bfloat16, dist=torch.float16) == "long"


def test_module_decides_with_the_route_function(monkeypatch):
    """CPU tensors: the module asks rnc_route (with the knob of this call) and takes torch."""
    from notorch_amd.nn.loss import rnc

    seen = []
    real = rnc.rnc_route

    def spy(n, device_type, sim_dtype, dist_dtype, knob):
        seen.append((n, device_type, sim_dtype, dist_dtype, knob))
        return real(n, device_type, sim_dtype, dist_dtype, knob)

    monkeypatch.setattr(rnc, "rnc_route", spy)
    monkeypatch.setenv("NT_RNC", "kernel")
    gen = torch.Generator().manual_seed(3)
    out = rnc.RankNContrastLoss()(torch.randn(9, 4, generator=gen), torch.randn(9, 1, generator=gen))
    assert seen == [(9, "cpu", F32, F32, "kernel")] and torch.isfinite(out).item()
