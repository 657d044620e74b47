"""CPU: the pairwise p-norm entry points (include/notorch_amd_train.h, csrc/pairwise.hip) are exported and
bound, validate on the host before any device call (fake, aligned pointers only: a launch here would answer
NT_EHIP = 2, never the statuses asserted), and PNorm's routing decision is the documented truth table."""
import ctypes
import itertools

import pytest
import torch

OK, EINVAL, EUNSUPPORTED = 0, 1, 3
F32, BF16 = 0, 1
A, B, X, G, DA = (ctypes.c_void_p(0x1000 * (i + 1)) for i in range(5))


def _lib():
    from notorch_amd import _lib

    return _lib.load()


def test_entry_points_are_bound_and_exported():
    from notorch_amd import _lib

    lib = _lib.load()
    for name in ("nt_pairwise_pnorm", "nt_pairwise_pnorm_backward_workspace", "nt_pairwise_pnorm_backward"):
        assert name in _lib.EXT_SIGNATURES and name not in _lib.SIGNATURES
        assert list(getattr(lib, name).argtypes) == list(_lib.EXT_SIGNATURES[name][1])
    assert lib.nt_abi_version() == _lib.ABI_VERSION == 8


# (overrides of n, m, d, dtype, p), status, a word of the rule in nt_last_error
REFUSALS = ((dict(p=3), EUNSUPPORTED, b"p must be 1 or 2"), (dict(p=0), EUNSUPPORTED, b"p must be 1 or 2"),
            (dict(dtype=2), EUNSUPPORTED, b"NT_F32 or NT_BF16"), (dict(n=-1), EINVAL, b"bad sizes"),
            (dict(m=-1), EINVAL, b"bad sizes"), (dict(d=-1), EINVAL, b"bad sizes"))


@pytest.mark.parametrize("over,status,word", REFUSALS)
def test_host_side_refusals(over, status, word):
    lib = _lib()
    a = dict(n=64, m=64, d=8, dtype=F32, p=2)
    a.update(over)
    assert lib.nt_pairwise_pnorm(A, B, a["n"], a["m"], a["d"], a["dtype"], a["p"], 0, X, None) == status
    assert word in lib.nt_last_error()
    assert lib.nt_pairwise_pnorm_backward(A, B, X, G, a["n"], a["m"], a["d"], a["dtype"], a["p"], 0, 1, 0, DA, None,
                                          0, None) == status
    assert word in lib.nt_last_error()


def test_null_pointers_flags_workspace_and_empty_shapes():
    lib = _lib()
    assert lib.nt_pairwise_pnorm(None, B, 4, 4, 2, F32, 2, 0, X, None) == EINVAL and b"NULL" in lib.nt_last_error()
    assert lib.nt_pairwise_pnorm(A, None, 4, 5, 2, F32, 2, 0, X, None) == EINVAL and b"m == n" in lib.nt_last_error()
    bwd = lib.nt_pairwise_pnorm_backward
    assert bwd(A, None, X, G, 4, 4, 2, F32, 2, 0, 1, 0, DA, None, 0, None) == EINVAL and b"NULL" in lib.nt_last_error()
    assert bwd(A, B, X, G, 4, 4, 2, F32, 2, 0, 0, 0, DA, None, 0, None) == EINVAL
    assert b"neither" in lib.nt_last_error()
    assert bwd(A, B, X, G, 4, 5, 2, F32, 2, 0, 1, 1, DA, None, 0, None) == EINVAL and b"m == n" in lib.nt_last_error()
    # 64 x 4096 x 8 is one (row, k) tile: j is split and the partial sums need the caller's workspace
    need = lib.nt_pairwise_pnorm_backward_workspace(64, 4096, 8)
    assert need > 0 and need % (64 * 8 * 4) == 0 and lib.nt_pairwise_pnorm_backward_workspace(-1, 4, 4) == -1
    assert lib.nt_pairwise_pnorm_backward_workspace(16384, 16384, 300) == 0
    assert bwd(A, B, X, G, 64, 4096, 8, F32, 2, 0, 1, 0, DA, None, 0, None) == EINVAL
    assert b"workspace" in lib.nt_last_error()
    for n, m in ((0, 7), (7, 0)):  # nothing to do: no launch
        assert lib.nt_pairwise_pnorm(A, B, n, m, 3, BF16, 1, 1, X, None) == OK
        assert bwd(A, B, X, G, n, m, 3, BF16, 1, 1, 1, 0, DA, None, 0, None) == OK


def test_pnorm_route_truth_table(monkeypatch):
    from notorch_amd.nn.loss import rnc

    f32, bf16 = torch.float32, torch.bfloat16
    for listed in ((), (1,), (1, 2)):
        monkeypatch.setattr(rnc, "PNORM_KERNEL_P", listed)
        for p, knob, (da, db) in itertools.product((1, 2.0, 3, 0.5), ("", "kernel", "torch"),
                                                   ((f32, f32), (bf16, bf16), (f32, bf16))):
            want = "kernel" if da == db and p in (1, 2) and (knob == "kernel" or (knob == "" and p in listed)) \
                else "torch"
            assert rnc.pnorm_route(p, "cuda", da, db, True, knob) == want, (listed, p, knob, da, db)
            assert rnc.pnorm_route(p, "cpu", da, db, True, knob) == "torch"
            assert rnc.pnorm_route(p, "cuda", da, db, False, knob) == "torch"
    for dtype in (torch.float64, torch.float16):
        assert rnc.pnorm_route(2, "cuda", dtype, dtype, True, "kernel") == "torch"
