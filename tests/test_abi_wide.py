"""CPU: the hidden-size limits of the bf16 layer kernel's column-pass variant (h > 512) and of the
fp32 plain update, as the C ABI and kernels.fused_supported state them.  No device call is made: every
call passes NULL data pointers, so validation ends at the NULL check (status 1) or at the size rule
(status 3, NT_EUNSUPPORTED)."""
import torch

BF16, F32 = 1, 0
RELU, SUM = 1, 0


def _lib():
    from notorch_amd import _lib

    return _lib.load()


def _update(lib, h, dtype):
    return lib.nt_dmpnn_update(None, None, None, None, None, None, 4, 8, h, 1, RELU, 0.0, dtype, None, None, None)


def _update_fused(lib, h, dtype):
    return lib.nt_dmpnn_update_fused(None, None, None, None, None, None, 4, 8, h, 1, RELU, 0.0, None, 0, 64, 4,
                                     None, None, None, SUM, RELU, 0.0, dtype, None, None, None, None, None, 0, 0,
                                     None)


def test_bf16_wide_sizes_reach_the_null_check():
    lib = _lib()
    for rc in (lib.nt_dmpnn_pack_weight(None, 1, 1024, BF16, None, None), _update(lib, 1024, BF16),
               _update_fused(lib, 1024, BF16),
               lib.nt_dmpnn_dense_matmul(None, 8, 1024, None, BF16, None, None, None, None)):
        assert rc == 1 and b"NULL" in lib.nt_last_error(), lib.nt_last_error()
    for h in (520, 2400, 8192):
        assert _update(lib, h, BF16) == 1 and b"NULL" in lib.nt_last_error(), h


def test_fp32_plain_update_above_512_reaches_the_null_check():
    lib = _lib()
    assert _update(lib, 640, F32) == 1 and b"NULL" in lib.nt_last_error()
    assert _update(lib, 8192, F32) == 1 and b"NULL" in lib.nt_last_error()
    # h % 4 != 0 stays on the exact fp32 tile kernel, h <= 512
    assert _update(lib, 642, F32) == 3 and b"h % 4 == 0" in lib.nt_last_error()
    assert _update(lib, 8196, F32) == 3


def test_bf16_unsupported_sizes_name_the_rule():
    lib = _lib()
    for h in (1028, 8200):
        for rc in (lib.nt_dmpnn_pack_weight(None, 1, h, BF16, None, None), _update(lib, h, BF16),
                   _update_fused(lib, h, BF16),
                   lib.nt_dmpnn_dense_matmul(None, 8, h, None, BF16, None, None, None, None)):
            msg = lib.nt_last_error()
            assert rc == 3 and b"h % 8 == 0" in msg and b"8192" in msg, (h, rc, msg)


def test_h_zero_still_answers_bad_sizes():
    lib = _lib()
    for dtype in (F32, BF16):
        assert _update(lib, 0, dtype) == 1 and b"bad sizes" in lib.nt_last_error()
        assert lib.nt_dmpnn_pack_weight(None, 1, 0, dtype, None, None) == 1 and b"bad sizes" in lib.nt_last_error()


def test_python_gate_tile_rows_and_image_size():
    from notorch_amd import kernels as K

    lib = _lib()
    assert K.fused_supported(10, 20, 1024, torch.bfloat16)
    assert K.fused_supported(10, 20, 8192, torch.bfloat16)
    assert not K.fused_supported(10, 20, 1028, torch.bfloat16)
    assert not K.fused_supported(10, 20, 8200, torch.bfloat16)
    assert lib.nt_dmpnn_fused_tile_rows(1024, BF16, RELU, SUM, RELU) == 64
    assert lib.nt_dmpnn_packed_weight_bytes(1024, BF16) == 32 * 64 * 64 * 16


def test_fp32_wide_tile_rows_and_image_size():
    """fp32 above hidden 384 (more than 24 column tiles): 64-row tiles for every layer, relu / sum
    included; the packed image holds the fk image of a width that fills neither its last column tile
    nor its last k-step (256-byte header + ks x nt fragment blocks of two 1 KiB parts)."""
    lib = _lib()
    for h in (388, 516, 8192):
        assert lib.nt_dmpnn_fused_tile_rows(h, F32, RELU, SUM, RELU) == 64, h
    assert lib.nt_dmpnn_fused_tile_rows(384, F32, RELU, SUM, RELU) == 128
    for h in (516, 1028):
        ks, nt = (h + 31) // 32, (h + 15) // 16
        assert lib.nt_dmpnn_packed_weight_bytes(h, F32) >= 256 + ks * nt * 2048, h
