"""CPU: nt_task_loss* and nt_rank_metric* (include/notorch_amd_train.h, csrc/task_loss.hip, csrc/rank_metric.hip)
are exported and bound, and validate on the host before any device call.  Fake, aligned pointers only: no
device call is reached (a launch on this CPU-only path would answer NT_EHIP = 2, never the statuses asserted
here)."""
import ctypes

import pytest
import torch

OK, EINVAL, EUNSUPPORTED = 0, 1, 3
NAMES = ("nt_task_loss_single_max", "nt_task_loss_workspace", "nt_task_loss", "nt_rank_metric_max_n",
         "nt_rank_metric")
MSE, MAE, RMSE, BCE, MVE, EVIDENTIAL, XENT = range(7)


def _lib():
    from notorch_amd import _lib

    return _lib.load()


def _p(i):
    return ctypes.c_void_p(0x1000 * (i + 1))


PREDS, TARGETS, MASK, WEIGHTS, LT, GT, LOSS, DPREDS, WS = (_p(i) for i in range(9))


def _loss(lib, kind=MSE, b=8, t=2, c=1, dtype=0, **over):
    a = dict(preds=PREDS, targets=TARGETS, mask=None, weights=None, lt=None, gt=None, loss=LOSS, dpreds=None,
             ws=None, ws_bytes=0)
    a.update(over)
    return lib.nt_task_loss(a["preds"], dtype, a["targets"], a["mask"], a["weights"], a["lt"], a["gt"], b, t, c,
                            kind, 0.2, 1e-8, a["loss"], a["dpreds"], a["ws"], a["ws_bytes"], None)


def test_entry_points_are_bound_and_exported():
    from notorch_amd import _lib

    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXT_SIGNATURES and name not in _lib.SIGNATURES
        assert hasattr(lib, name)
        assert list(getattr(lib, name).argtypes) == list(_lib.EXT_SIGNATURES[name][1])
    assert lib.nt_abi_version() == _lib.ABI_VERSION == 8
    assert (_lib.NT_LOSS_MSE, _lib.NT_LOSS_MAE, _lib.NT_LOSS_RMSE, _lib.NT_LOSS_BCE, _lib.NT_LOSS_MVE,
            _lib.NT_LOSS_EVIDENTIAL, _lib.NT_LOSS_XENT) == (MSE, MAE, RMSE, BCE, MVE, EVIDENTIAL, XENT)


def test_limits_and_workspace_query():
    from notorch_amd import kernels as K

    lib = _lib()
    single = lib.nt_task_loss_single_max()
    assert single >= 4096 and K.task_loss_single_max() == single  # the bench batch is one launch
    ws = lib.nt_task_loss_workspace
    assert ws(-1, 1) == -1 and ws(1, -1) == -1 and ws(1 << 41, 1) == -1 and ws(1 << 30, 1 << 30) == -1
    assert ws(0, 5) == 0 and ws(single, 1) == 0 and ws(single // 2, 2) == 0
    assert ws(single + 1, 1) == 16 + 16 * 2 and ws(single, 3) == 16 + 16 * 3
    assert lib.nt_rank_metric_max_n() >= 4096 and K.rank_metric_max_n() == lib.nt_rank_metric_max_n()


def test_task_loss_validates_on_the_host():
    lib = _lib()
    for null in ("preds", "targets", "loss"):
        assert _loss(lib, **{null: None}) == EINVAL and b"NULL" in lib.nt_last_error(), null
    assert _loss(lib, kind=7) == EUNSUPPORTED and b"kind" in lib.nt_last_error()
    assert _loss(lib, kind=-1) == EUNSUPPORTED and b"kind" in lib.nt_last_error()
    assert _loss(lib, dtype=5) == EUNSUPPORTED and b"dtype" in lib.nt_last_error()
    for bad in (dict(b=-1), dict(t=-1), dict(c=0), dict(b=1 << 41), dict(b=1 << 30, t=1 << 30)):
        assert _loss(lib, **bad) == EINVAL and b"bad sizes" in lib.nt_last_error(), bad
    # a c that does not fit the kind
    for kind, c in ((MSE, 2), (MAE, 2), (RMSE, 3), (BCE, 2), (MVE, 1), (MVE, 3), (EVIDENTIAL, 2), (EVIDENTIAL, 5)):
        assert _loss(lib, kind=kind, c=c) == EINVAL and b"does not fit the kind" in lib.nt_last_error(), (kind, c)
    # bounds belong to MSE / MAE / RMSE
    for kind, c in ((BCE, 1), (MVE, 2), (EVIDENTIAL, 4), (XENT, 3)):
        assert _loss(lib, kind=kind, c=c, lt=LT) == EINVAL and b"lt_mask" in lib.nt_last_error()
        assert _loss(lib, kind=kind, c=c, gt=GT) == EINVAL
    # above the one-launch size the workspace is required, whole and aligned
    big = lib.nt_task_loss_single_max() + 1
    need = lib.nt_task_loss_workspace(big, 1)
    assert _loss(lib, b=big, t=1) == EINVAL and b"workspace" in lib.nt_last_error()
    assert _loss(lib, b=big, t=1, ws=WS, ws_bytes=need - 1) == EINVAL and b"workspace" in lib.nt_last_error()
    assert _loss(lib, b=big, t=1, ws=ctypes.c_void_p(0x9008), ws_bytes=need) == EINVAL
    # nothing to do: no launch, whatever else is passed
    for kind, c in ((MSE, 1), (MVE, 2), (EVIDENTIAL, 4), (XENT, 5)):
        assert _loss(lib, kind=kind, b=0, t=3, c=c, mask=MASK, weights=WEIGHTS, dpreds=DPREDS) == OK
        assert _loss(lib, kind=kind, b=3, t=0, c=c, dtype=1) == OK


def test_rank_metric_validates_on_the_host():
    lib = _lib()
    scores, targets, out = _p(0), _p(1), _p(2)
    for args in ((None, targets, None, 8, 1, out), (scores, None, None, 8, 1, out), (scores, targets, None, 8, 1, None)):
        assert lib.nt_rank_metric(*args, None) == EINVAL and b"NULL" in lib.nt_last_error()
    for n, t in ((-1, 1), (8, -1), (8, 1 << 31)):
        assert lib.nt_rank_metric(scores, targets, None, n, t, out, None) == EINVAL
        assert b"bad sizes" in lib.nt_last_error()
    too_many = lib.nt_rank_metric_max_n() + 1
    assert lib.nt_rank_metric(scores, targets, None, too_many, 1, out, None) == EUNSUPPORTED
    assert b"nt_rank_metric_max_n" in lib.nt_last_error() and str(too_many - 1).encode() in lib.nt_last_error()
    assert lib.nt_rank_metric(scores, targets, _p(3), 64, 0, out, None) == OK  # no columns: no launch


def test_bindings_validate_before_the_library(monkeypatch):
    from notorch_amd import _lib
    from notorch_amd import kernels as K

    def _fail():
        raise AssertionError("the binding reached the library")

    monkeypatch.setattr(_lib, "load", _fail)
    p, y = torch.zeros(6, 2), torch.zeros(6, 2)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        K.task_loss(p, y, "mse", need_grad=True)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        K.task_loss(p, y, "mae", mask=torch.ones(6, 2, dtype=torch.bool), sample_weights=torch.ones(6))
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        K.rank_metric(p, y)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        K.rank_metric(p, y, torch.ones(6, 2, dtype=torch.bool))
