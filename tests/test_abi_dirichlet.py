"""CPU: nt_dirichlet_loss and nt_dirichlet_loss_workspace (include/notorch_amd_train.h) are bound and validate on
the host before any device call, in the style of tests/test_abi_task_loss.py: fake, aligned pointers only."""
import ctypes

from test_abi_task_loss import DPREDS, EINVAL, EUNSUPPORTED, LOSS, MASK, OK, PREDS, TARGETS, WEIGHTS, WS, _lib


def _loss(lib, b=8, t=2, k=3, dtype=0, **over):
    a = dict(preds=PREDS, targets=TARGETS, mask=None, weights=None, loss=LOSS, dpreds=None, ws=None, ws_bytes=0)
    a.update(over)
    return lib.nt_dirichlet_loss(a["preds"], dtype, a["targets"], a["mask"], a["weights"], b, t, k, 0.2, a["loss"],
                                 a["dpreds"], a["ws"], a["ws_bytes"], None)


def test_workspace_query_counts_lane_slots():
    from notorch_amd import _lib as L

    ws = _lib().nt_dirichlet_loss_workspace
    assert len(L.LOSS_CODES) == 7 and "nt_dirichlet_loss" in L.EXT_SIGNATURES  # no eighth kind of nt_task_loss
    assert ws(-1, 1, 2) == -1 and ws(1, -1, 2) == -1 and ws(1, 1, 0) == -1 and ws(1 << 30, 1 << 30, 2) == -1
    assert ws(1 << 20, 1 << 10, 1 << 11) == -1  # more than 2^40 logits
    # W = 1 for k = 1, 2 for 2, 4 for 3, 64 from k = 33 on: 8192 slots are one launch
    assert ws(0, 5, 2) == ws(4096, 1, 2) == ws(2048, 1, 3) == ws(128, 1, 64) == ws(128, 1, 999) == ws(8192, 1, 1) == 0
    assert ws(4097, 1, 2) == ws(2049, 1, 4) == ws(8193, 1, 1) == 16 + 16 * 2 and ws(129, 2, 33) == 16 + 16 * 3


def test_dirichlet_loss_validates_on_the_host():
    lib = _lib()
    for null in ("preds", "targets", "loss"):
        assert _loss(lib, **{null: None}) == EINVAL and b"NULL" in lib.nt_last_error(), null
    assert _loss(lib, dtype=5) == EUNSUPPORTED and b"dtype" in lib.nt_last_error()
    for bad in (dict(b=-1), dict(t=-1), dict(k=0), dict(k=-3), dict(b=1 << 41), dict(b=1 << 30, t=1 << 30)):
        assert _loss(lib, **bad) == EINVAL and b"bad sizes" in lib.nt_last_error(), bad
    need = lib.nt_dirichlet_loss_workspace(2049, 1, 3)  # above the one-launch size: required, whole and aligned
    assert need > 0 and _loss(lib, b=2049, t=1) == EINVAL and b"workspace" in lib.nt_last_error()
    assert _loss(lib, b=2049, t=1, ws=WS, ws_bytes=need - 1) == EINVAL and b"workspace" in lib.nt_last_error()
    assert _loss(lib, b=2049, t=1, ws=ctypes.c_void_p(0x9008), ws_bytes=need) == EINVAL
    assert _loss(lib, b=0, t=3, mask=MASK, weights=WEIGHTS, dpreds=DPREDS) == OK  # nothing to do: no launch
    assert _loss(lib, b=3, t=0, k=65, dtype=1) == OK
