"""CPU: nt_dmpnn_weight_grad_fk's size rule (pure host validation, no launch) and the workspace query.

The entry takes h <= 320 (wgrad_fk_kernel) or h % 4 == 0 up to 8192 (wgrad_fk_wide_kernel).  Every call
below passes NULL pointers, V = 4 and E = 8, so an accepted shape ends at the dW_out check (status 1)
before anything touches a device.  nt_dmpnn_weight_grad_workspace is compared with the values the library
returned before the wide kernel existed (recorded without a GPU: the CU count falls back to 256, which
is also an MI355X's): the wide kernel's split-K plan never asks for more chunks than the plans already
in that maximum."""
import pytest

NT_EINVAL, NT_EUNSUPPORTED = 1, 3
NT_F32 = 0


def _call(h):
    from notorch_amd import _lib

    lib = _lib.load()
    rc = lib.nt_dmpnn_weight_grad_fk(None, None, None, None, None, 4, 8, h, 1, 0.0, None, None, NT_F32, None, 0,
                                     None, None, None)
    return rc, lib.nt_last_error()


@pytest.mark.parametrize("h", [324, 512, 8192])
def test_wide_sizes_pass_the_size_rule(h):
    rc, msg = _call(h)
    assert rc == NT_EINVAL and b"dW_out" in msg, (rc, msg)


@pytest.mark.parametrize("h", [322, 518, 8196])
def test_unsupported_sizes_name_the_rule(h):
    rc, msg = _call(h)
    assert rc == NT_EUNSUPPORTED, (rc, msg)
    assert b"h % 4" in msg, msg


@pytest.mark.parametrize("h", [4, 299, 320])
def test_narrow_sizes_unchanged(h):
    rc, msg = _call(h)
    assert rc == NT_EINVAL and msg == b"nt_dmpnn_weight_grad_fk: NULL dW_out", (rc, msg)


# (E, h) -> bytes
_WORKSPACE = {
    (1, 300): 361200, (1, 324): 421200, (1, 512): 1050624, (1, 1024): 4198400, (1, 2048): 16785408,
    (1, 8192): 268468224,
    (33, 300): 722400, (33, 324): 842400, (33, 512): 2101248, (33, 1024): 8396800, (33, 2048): 33570816,
    (33, 8192): 536936448,
    (4097, 300): 23478000, (4097, 324): 27378000, (4097, 512): 45176832, (4097, 1024): 109158400,
    (4097, 2048): 251781120, (4097, 8192): 2147745792,
    (204_130, 300): 30340800, (204_130, 324): 35380800, (204_130, 512): 67239936, (204_130, 1024): 134348800,
    (204_130, 2048): 268566528, (204_130, 8192): 2147745792,
}


def test_workspace_query_unchanged():
    from notorch_amd import _lib

    lib = _lib.load()
    got = {k: lib.nt_dmpnn_weight_grad_workspace(*k) for k in _WORKSPACE}
    assert got == _WORKSPACE
