"""GPU: AUROC and average precision on the sort-and-scan kernel nt_rank_metric (csrc/rank_metric.hip).

The yardstick is the torch route (rank_metric_torch) on the same scores in fp64 on the CPU; tests/test_task_loss.py
ties that route to the O(n^2) pairwise definition and to the per-threshold average precision.  AUROC and AP
must agree within 1e-5 absolute and lie in [0, 1]; P and N must be exact; two calls must return the same
bits.  Every case prints ``RANKERR <metric> <value> <case>``."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-5
# (n, scores): degenerate scans; the wave edge; padding to 256 and over several waves; groups of ~200 equal
# scores that cross waves; one group (the largest n runs once, below)
CASES = ((2, "distinct"), (3, "distinct"), (63, "distinct"), (64, "distinct"), (65, "distinct"),
         (257, "distinct"), (1000, "five"), (1000, "equal"))


def _K():
    from notorch_amd import kernels

    return kernels


def _M():
    from notorch_amd.nn import metrics

    return metrics


@functools.lru_cache(maxsize=None)
def _inputs(n, kind, t):
    gen = torch.Generator().manual_seed(1000 * n + 10 * t + len(kind))
    if kind == "distinct":
        s = torch.randn(n, t, generator=gen)
    elif kind == "five":
        s = torch.randint(0, 5, (n, t), generator=gen).float() / 4 - 0.5
        s[0, 0] = -0.0  # ties with +0
    else:
        s = torch.full((n, t), 0.25)
    y = (torch.rand(n, t, generator=gen) < 0.4).float()
    y[0], y[1] = 1.0, 0.0  # both classes in every column
    mask = torch.rand(n, t, generator=gen) < 0.7
    mask[:2] = True
    return s, y, mask


def _compare(res, s, y, mask, case):
    want = _M().rank_metric_torch(s.double(), y.double(), mask)
    res = res.cpu()
    assert res.shape == want.shape and res.dtype == torch.float32
    assert torch.equal(res[:, 2:].double(), want[:, 2:])  # P and N: exact
    live = ~torch.isnan(want[:, 0])
    assert torch.equal(torch.isnan(res[:, 0]), ~live) and torch.equal(torch.isnan(res[:, 1]), ~live)
    for col, name in ((0, "auroc"), (1, "ap")):
        err = (res[live, col].double() - want[live, col]).abs().max().item() if live.any() else 0.0
        print(f"RANKERR {name} {err:.3e} {case}")
        assert err <= TOL
        assert ((res[live, col] >= 0) & (res[live, col] <= 1)).all().item()


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("t", (1, 3))
@pytest.mark.parametrize("n,kind", CASES)
def test_kernel_matches_the_fp64_torch_route(n, kind, t, masked):
    s, y, mask = _inputs(n, kind, t)
    mask = mask if masked else None
    res = _K().rank_metric(s.to(DEV), y.to(DEV), None if mask is None else mask.to(DEV))
    _compare(res, s, y, mask, f"n={n} {kind} t={t} masked={masked}")


def test_largest_n_once():
    n = _K().rank_metric_max_n()
    assert n == 4096
    s, y, mask = _inputs(n, "distinct", 3)
    _compare(_K().rank_metric(s.to(DEV), y.to(DEV), mask.to(DEV)), s, y, mask, f"n={n} distinct t=3 masked=True")


def test_columns_without_both_classes():
    n = 300
    s, y, _ = _inputs(n, "distinct", 3)
    y = y.clone()
    y[:, 0] = 1.0  # no negatives
    y[:, 2] = 0.0  # no positives
    res = _K().rank_metric(s.to(DEV), y.to(DEV))
    _compare(res, s, y, None, "n=300 t=3, a column without negatives and one without positives")
    assert torch.isnan(res[0, :2]).all().item() and res[0, 2].item() == n and res[0, 3].item() == 0
    assert torch.isnan(res[2, :2]).all().item() and res[2, 2].item() == 0 and res[2, 3].item() == n
    M = _M()
    for cls, col in ((M.AUROC, 0), (M.AUPRC, 1)):
        out = cls("multilabel")(s.to(DEV), y.to(DEV))
        assert out.item() == res[1, col].item()  # the mean over the one column with both classes
        assert torch.isnan(cls("multilabel")(s[:, :1].to(DEV), y[:, :1].to(DEV))).item()
    # targets that are neither 0 nor 1 are ignored, like masked entries
    y2, mask = _inputs(n, "distinct", 3)[1].clone(), torch.ones(n, 3, dtype=torch.bool)
    y2[5:40] = 2.0
    mask[5:40] = False
    a = _K().rank_metric(s.to(DEV), y2.to(DEV))
    b = _K().rank_metric(s.to(DEV), _inputs(n, "distinct", 3)[1].to(DEV), mask.to(DEV))
    assert torch.equal(a, b)


def test_two_calls_return_the_same_bits():
    for n, kind in ((1000, "five"), (257, "distinct")):
        s, y, mask = (x.to(DEV) for x in _inputs(n, kind, 3))
        a, b = _K().rank_metric(s, y, mask), _K().rank_metric(s, y, mask)
        assert torch.equal(a, b) and torch.isfinite(a).all().item()


def test_modules_route_by_size_and_agree(monkeypatch):
    K, M = _K(), _M()
    real, seen = K.rank_metric, []

    def counted(*args):
        seen.append(tuple(args[0].shape))
        return real(*args)

    monkeypatch.setattr(K, "rank_metric", counted)
    monkeypatch.delenv("NT_LOSS", raising=False)
    big = K.rank_metric_max_n() + 1  # 4097 rows: the torch route on the device
    s, y, mask = _inputs(big, "distinct", 1)
    for cls, col in ((M.AUROC, 0), (M.AUPRC, 1)):
        want = M.rank_metric_torch(s.double(), y.double(), mask)[0, col].item()
        out = cls("multilabel")(s.to(DEV), y.to(DEV), mask=mask.to(DEV))
        assert seen == [] and abs(out.item() - want) <= TOL
    # binary pools the b x t entries into one ranking: 1365 x 3 = 4095 rows take the kernel, 4098 do not
    s3, y3, m3 = _inputs(1366, "five", 3)
    for rows in (1365, 1366):
        seen.clear()
        a, b, c = s3[:rows], y3[:rows], m3[:rows]
        want = M.rank_metric_torch(a.reshape(-1, 1).double(), b.reshape(-1, 1).double(), c.reshape(-1, 1))[0, 0].item()
        out = M.AUROC("binary")(a.to(DEV), b.to(DEV), mask=c.to(DEV))
        assert seen == ([(3 * rows, 1)] if rows == 1365 else []) and abs(out.item() - want) <= TOL
    # bf16 scores are widened; the knob, read per call, keeps the metric on torch ops
    seen.clear()
    s, y, mask = _inputs(257, "distinct", 3)
    sb = s.bfloat16()
    out = M.AUPRC("multilabel")(sb.to(DEV), y.to(DEV), mask=mask.to(DEV))
    want = M.rank_metric_torch(sb.double(), y.double(), mask)[:, 1].mean().item()
    assert seen == [(257, 3)] and abs(out.item() - want) <= TOL
    monkeypatch.setenv("NT_LOSS", "torch")
    again = M.AUPRC("multilabel")(sb.to(DEV), y.to(DEV), mask=mask.to(DEV))
    assert seen == [(257, 3)] and abs(again.item() - want) <= TOL  # half-precision scores: counted in fp32
