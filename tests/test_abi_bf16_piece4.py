"""CPU: the hidden sizes nt_dmpnn_update_fused takes in bf16, as the C ABI and kernels.fused_supported
state them: rows of whole 16-byte pieces (h % 8 == 0 up to 8192) or of whole 8-byte pieces (h % 4 == 0
up to 512; the layer kernel's W = 4 instances, which have no dropout variant).  No device call is made:
every call passes NULL data pointers, so validation ends at the NULL check (status 1) or at the size
rule (status 3, NT_EUNSUPPORTED)."""
import pytest
import torch

BF16, F32 = 1, 0
RELU, SUM = 1, 0
EINVAL, EUNSUPPORTED = 1, 3


def _lib():
    from notorch_amd import _lib

    return _lib.load()


def _update_fused(lib, h, dtype=BF16):
    return lib.nt_dmpnn_update_fused(None, None, None, None, None, None, 4, 8, h, 1, RELU, 0.0, None, 0, 64, 4,
                                     None, None, None, SUM, RELU, 0.0, dtype, None, None, None, None, None, 0, 0,
                                     None)


def _update_fused_dropout(lib, h, dtype=BF16):
    return lib.nt_dmpnn_update_fused_dropout(None, None, None, None, None, None, 4, 8, h, 1, RELU, 0.0, None, 0, 64,
                                             4, None, None, None, SUM, RELU, 0.0, dtype, None, None, None, None,
                                             None, 0, 0, 0.25, 1, 0, None)


@pytest.mark.parametrize("h", [4, 36, 300, 508])
def test_eight_byte_piece_sizes_reach_the_null_check(h):
    lib = _lib()
    assert _update_fused(lib, h) == EINVAL and b"NULL" in lib.nt_last_error(), lib.nt_last_error()


@pytest.mark.parametrize("h", [2, 302, 510, 516, 1028])
def test_other_sizes_name_the_rule(h):
    lib = _lib()
    rc, msg = _update_fused(lib, h), lib.nt_last_error()
    assert rc == EUNSUPPORTED, (h, rc, msg)
    assert b"h % 8 == 0" in msg and b"8192" in msg and b"h % 4 == 0" in msg and b"512" in msg, msg


def test_sixteen_byte_piece_sizes_are_as_before():
    lib = _lib()
    for h in (8, 304, 512, 520, 8192):
        assert _update_fused(lib, h) == EINVAL and b"NULL" in lib.nt_last_error(), h
        assert _update_fused_dropout(lib, h) == EINVAL and b"NULL" in lib.nt_last_error(), h


def test_dropout_entry_refuses_eight_byte_piece_sizes():
    lib = _lib()
    for h in (4, 36, 300, 508):
        rc, msg = _update_fused_dropout(lib, h), lib.nt_last_error()
        assert rc == EUNSUPPORTED and b"h % 8 == 0" in msg and b"dropout" in msg, (h, rc, msg)
    # fp32 h % 4 == 0 is untouched
    assert _update_fused_dropout(lib, 300, F32) == EINVAL and b"NULL" in lib.nt_last_error()


def test_python_gate_tile_rows_and_abi_version():
    from notorch_amd import _lib as L
    from notorch_amd import kernels as K

    lib = _lib()
    for h in (4, 36, 300, 508):
        assert K.fused_supported(10, 20, h, torch.bfloat16), h
    for h in (2, 302, 516, 1028):
        assert not K.fused_supported(10, 20, h, torch.bfloat16), h
    assert not K.fused_supported(10, 2**31, 300, torch.bfloat16)
    assert lib.nt_dmpnn_fused_tile_rows(300, BF16, RELU, SUM, RELU) == 64
    assert lib.nt_abi_version() == L.ABI_VERSION == 8


def test_engine_keeps_the_backward_rule_and_has_the_gate():
    from notorch_amd.nn.gnn import _engine

    assert _engine.BF16_FUSED_PIECE4 in (True, False)
    # dA / dW stay off the kernels at h % 8 == 4 (the forward's rule widened, the backward's did not)
    assert not _engine._bf16_backward_kernels(10, 20, 300) and not _engine._bf16_backward_kernels(10, 20, 36)
    assert _engine._bf16_backward_kernels(10, 20, 304) and _engine._bf16_backward_kernels(10, 20, 8192)
    assert not _engine._bf16_backward_kernels(10, 2**31, 304)
