"""CPU: nt_dmpnn_update_fused_dropout (include/notorch_amd_train.h), the layer kernel with training-mode
dropout in its epilogue.  The symbol is an additive export bound from _lib.EXT_SIGNATURES; its host-side
validation (the dropout probability, then the rules of nt_dmpnn_update_fused, then the tile plan the
dropout instances need) ends before any device call, so fake aligned pointers reach every check."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = 0, 1
RELU, SUM = 1, 0
EINVAL, EUNSUPPORTED = 1, 3


def _lib():
    from notorch_amd import _lib

    return _lib.load()


def _fake(n=12):
    return [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(n)]


def _call(lib, *, data=None, h=64, dtype=F32, tile_ptr=None, ntiles=0, rows=64, perm=None, dsts=None, rt=None,
          amax_in=None, H_out=None, S_out=None, S_part=None, ld_in=0, ld_out=0, p=0.25, seed=1, offset=0):
    data = data or [None] * 6
    return lib.nt_dmpnn_update_fused_dropout(*data, 10, 20, h, 1, RELU, 0.0, tile_ptr, ntiles, rows, 4, perm, dsts,
                                             rt, SUM, RELU, 0.0, dtype, amax_in, None, H_out, S_out, S_part, ld_in,
                                             ld_out, p, seed, offset, None)


def test_symbol_is_an_additive_export():
    from notorch_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "nt_dmpnn_update_fused_dropout")
    assert "nt_dmpnn_update_fused_dropout" in _lib.EXT_SIGNATURES
    assert "nt_dmpnn_update_fused_dropout" not in _lib.SIGNATURES
    assert lib.nt_abi_version() == _lib.ABI_VERSION == 8
    # the plain entry's arguments, then (p, seed, offset), then the stream
    plain, drop = _lib.SIGNATURES["nt_dmpnn_update_fused"], _lib.EXT_SIGNATURES["nt_dmpnn_update_fused_dropout"]
    assert drop[0] is plain[0]
    assert drop[1] == plain[1][:-1] + [ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64] + plain[1][-1:]
    # declared in the training header, absent from the frozen one
    train = open(os.path.join(ROOT, "include", "notorch_amd_train.h")).read()
    base = open(os.path.join(ROOT, "include", "notorch_amd.h")).read()
    assert re.search(r"^NT_API\s+int\s+nt_dmpnn_update_fused_dropout\s*\(", train, flags=re.M)
    assert "nt_dmpnn_update_fused_dropout" not in base


@pytest.mark.parametrize("p", [-0.01, 1.5, float("nan")])
def test_bad_probability_is_rejected_first(p):
    lib = _lib()
    # even with everything else NULL / unsupported: the probability is checked before anything
    assert _call(lib, p=p, h=0, dtype=7) == EINVAL
    assert b"probability" in lib.nt_last_error()


def test_limits_of_p_reach_the_other_checks():
    lib = _lib()
    for p in (0.0, 1.0):
        assert _call(lib, p=p) == EINVAL and b"NULL" in lib.nt_last_error()


def test_dtype_and_shape_rules_of_the_plain_entry():
    lib = _lib()
    fake = _fake()
    assert _call(lib, dtype=2) == EUNSUPPORTED and b"dtype" in lib.nt_last_error()
    # bf16 with a padded pitch or hub partials: fp32 only
    assert _call(lib, data=fake[:6], h=512, dtype=BF16, H_out=fake[6], ld_in=520) == EUNSUPPORTED
    assert b"fp32 only" in lib.nt_last_error()
    assert _call(lib, data=fake[:6], h=512, dtype=BF16, H_out=fake[6], S_part=fake[7]) == EUNSUPPORTED
    # hidden sizes
    assert _call(lib, h=66, dtype=F32) == EUNSUPPORTED and b"h % 4 == 0" in lib.nt_last_error()
    assert _call(lib, h=8200, dtype=BF16) == EUNSUPPORTED
    assert _call(lib, h=0) == EINVAL and b"bad sizes" in lib.nt_last_error()
    # alignment of the feature pointers
    odd = [ctypes.c_void_p(0x1004)] + fake[1:6]
    assert _call(lib, data=odd, H_out=fake[6], tile_ptr=fake[7], S_out=fake[8]) == EINVAL
    assert b"aligned" in lib.nt_last_error()


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_plan_is_required(dtype):
    lib = _lib()
    fake = _fake()
    # S_out without a plan: the plain entry's pairing rule
    rc = _call(lib, data=fake[:6], dtype=dtype, H_out=fake[6], S_out=fake[7], amax_in=fake[8])
    assert rc == EINVAL and b"S_out must be given exactly with a tile plan" in lib.nt_last_error()
    # no plan at all: the dropout instances exist for fused plans only
    rc = _call(lib, data=fake[:6], dtype=dtype, H_out=fake[6], amax_in=fake[8])
    assert rc == EUNSUPPORTED and b"tile plan" in lib.nt_last_error()
    # a plan without S_out
    rc = _call(lib, data=fake[:6], dtype=dtype, H_out=fake[6], tile_ptr=fake[7], ntiles=1, perm=fake[9],
               dsts=fake[10], rt=fake[11], amax_in=fake[8])
    assert rc == EINVAL, lib.nt_last_error()


def test_fp32_plan_rules_before_any_launch():
    lib = _lib()
    fake = _fake()
    plan = dict(data=fake[:6], H_out=fake[6], tile_ptr=fake[7], ntiles=1, S_out=fake[8], perm=fake[9], dsts=fake[10])
    # no row table / no amax_in / rows above the layer's tile capacity (h = 400: 64-row tiles)
    assert _call(lib, **plan, amax_in=fake[11]) == EINVAL and b"row table" in lib.nt_last_error()
    assert _call(lib, **plan, rt=fake[11]) == EINVAL and b"amax_in" in lib.nt_last_error()
    assert _call(lib, **plan, rt=fake[11], amax_in=fake[5], h=400, rows=128) == EUNSUPPORTED
    assert b"tile plan rows" in lib.nt_last_error()
    # bf16: plans of at most 64 rows
    assert _call(lib, **plan, dtype=BF16, rows=128) == EUNSUPPORTED and b"64 rows" in lib.nt_last_error()


def test_python_binding_validates_before_the_library_is_loaded(monkeypatch):
    """kernels.dmpnn_update_fused(dropout=...) rejects a bad probability, a negative offset, a missing
    plan and a bf16 plan of more than 64 rows in Python; tensors off the device are refused as ever."""
    from notorch_amd import _lib
    from notorch_amd import kernels as K

    def boom():
        raise AssertionError("validation must not load the library")

    monkeypatch.setattr(_lib, "load", boom)
    H, S = torch.zeros(4, 8), torch.zeros(2, 8)
    idx = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        K.dmpnn_update_fused(H, S, idx, idx, torch.zeros(1), None, dropout=(0.25, 1, 0))
    monkeypatch.setattr(K, "_require_device", lambda *ts: torch.device("cpu"))
    for bad, msg in (((1.5, 1, 0), "probability"), ((-0.1, 1, 0), "probability"), ((0.25, 1, -1), "offset"),
                     ((0.25, 1, 0), "tile plan")):
        with pytest.raises(ValueError, match=msg):
            K.dmpnn_update_fused(H, S, idx, idx, torch.zeros(1), None, dropout=bad)
    plan = (torch.zeros(2, dtype=torch.int32), 1, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="64 rows"):
        K.dmpnn_update_fused(H.bfloat16(), S.bfloat16(), idx, idx, torch.zeros(1), None, plan=plan, tile_rows=128,
                             perm=torch.zeros(4, dtype=torch.int32), dropout=(0.25, 1, 0))


def test_engine_switches(monkeypatch):
    from notorch_amd.nn.gnn import _engine

    monkeypatch.delenv("NT_FUSED_DROPOUT", raising=False)
    assert _engine._fused_dropout_enabled()
    monkeypatch.setenv("NT_FUSED_DROPOUT", "0")
    assert not _engine._fused_dropout_enabled()
    monkeypatch.setenv("NT_FUSED_DROPOUT", "1")
    assert _engine._fused_dropout_enabled()
