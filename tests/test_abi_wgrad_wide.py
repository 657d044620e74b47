"""CPU: nt_dmpnn_weight_grad's size rule for bf16 storage (pure host validation, no launch).

bf16 takes an even h <= 512 (wgrad_bf16_kernel) or h % 8 == 0 up to 8192 (wgrad_bf16_wide_kernel), with
src and rev given.  Every call below passes E = 0 and dW_out = NULL, so an accepted shape ends at the
dW_out check (status 1) before anything touches a device."""
import ctypes

import pytest

NT_EINVAL, NT_EUNSUPPORTED = 1, 3
NT_BF16 = 1


def _call(h, with_index=True):
    from notorch_amd import _lib

    lib = _lib.load()
    idx = (ctypes.c_int64 * 1)(0)  # never read: E = 0
    p = ctypes.cast(idx, ctypes.c_void_p) if with_index else None
    rc = lib.nt_dmpnn_weight_grad(None, None, None, p, p, 4, 0, h, 1, 0.0, NT_BF16, None, 0, None, None, None)
    return rc, lib.nt_last_error()


@pytest.mark.parametrize("h", [640, 1024, 8192])
def test_wide_sizes_pass_the_size_rule(h):
    rc, msg = _call(h)
    assert rc == NT_EINVAL and b"dW_out" in msg, (rc, msg)


@pytest.mark.parametrize("h", [510, 512])
def test_narrow_sizes_unchanged(h):
    rc, msg = _call(h)
    assert rc == NT_EINVAL and b"dW_out" in msg, (rc, msg)


@pytest.mark.parametrize("h", [644, 8200])
def test_unsupported_sizes_name_the_rule(h):
    rc, msg = _call(h)
    assert rc == NT_EUNSUPPORTED, (rc, msg)
    assert b"h % 8 == 0" in msg and b"8192" in msg, msg


def test_wide_still_needs_src_and_rev():
    rc, _ = _call(640, with_index=False)
    assert rc == NT_EUNSUPPORTED


def test_workspace_query_covers_the_wide_plan():
    from notorch_amd import _lib

    lib = _lib.load()
    assert lib.nt_dmpnn_weight_grad_workspace(4097, 640) > 0
    assert lib.nt_dmpnn_weight_grad_workspace(33, 8192) > 0
    assert lib.nt_dmpnn_weight_grad_workspace(-1, 640) == -1
