"""GPU: AUROC and average precision above 4096 rows on nt_rank_metric_long (csrc/rank_metric_long.hip): sorted
runs of 4096 rows, merge-path passes and a tiled scan.

The scheme is that of tests/test_gpu_rank_metric.py: the yardstick is the torch route (rank_metric_torch) on the
same scores in fp64 on the CPU; AUROC and AP must agree within 1e-5 absolute and lie in [0, 1]; P and N must
be exact and the NaN pattern equal; two calls must return the same bits.  Every case prints
``RANKERR <metric> <value> <case>``.  The shapes are the smallest at which a tile boundary, an odd run or a
carry can go wrong:
  4097   one real entry in the second run
  8192   no padding
  8193   three runs: one copied through the first pass, then an unequal merge
  12288  three whole tiles
  20480  five runs, three passes; with five score values groups of ~4000 equal scores cross tiles, with equal
         scores one group covers all tiles
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-5
SIZES = (4097, 8192, 8193, 12288, 20480)
KINDS = ("distinct", "five", "equal")


def _K():
    from notorch_amd import kernels

    return kernels


def _M():
    from notorch_amd.nn import metrics

    return metrics


@functools.lru_cache(maxsize=None)
def _inputs(n, kind, t):
    gen = torch.Generator().manual_seed(1000 * n + 10 * t + len(kind))
    if kind == "five":
        s = torch.randint(0, 5, (n, t), generator=gen).float() / 4 - 0.5
        s[0, 0] = -0.0  # ties with +0
    elif kind == "equal":
        s = torch.full((n, t), 0.25)
    else:
        s = torch.randn(n, t, generator=gen)
        if kind == "ascending":
            s = s.sort(0).values
        elif kind == "descending":
            s = s.sort(0, descending=True).values
    y = (torch.rand(n, t, generator=gen) < 0.4).float()
    y[0], y[1] = 1.0, 0.0  # both classes in every column
    mask = torch.rand(n, t, generator=gen) < 0.7
    mask[:2] = True
    return s, y, mask


@functools.lru_cache(maxsize=None)
def _want(n, kind, t, masked):
    s, y, mask = _inputs(n, kind, t)
    return _M().rank_metric_torch(s.double(), y.double(), mask if masked else None)


def _compare(res, want, case):
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


def _run(n, kind, t, masked):
    s, y, mask = _inputs(n, kind, t)
    res = _K().rank_metric_long(s.to(DEV), y.to(DEV), mask.to(DEV) if masked else None)
    _compare(res, _want(n, kind, t, masked), f"n={n} {kind} t={t} masked={masked}")


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("t", (1, 3))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_the_fp64_torch_route(n, kind, t, masked):
    _run(n, kind, t, masked)


@pytest.mark.parametrize("kind", ("ascending", "descending"))
def test_sorted_scores_split_at_the_ends_of_the_ranges(kind):
    """Every merge-path split falls at an end of its range: a tile takes all of one sequence or none of it."""
    _run(8193, kind, 1, False)
    _run(8193, kind, 3, True)


def test_a_whole_run_of_ignored_entries():
    n = 12288
    s, y, mask = (x.clone() for x in _inputs(n, "distinct", 3))
    mask[:4096] = False
    y[4096], y[4097] = 1.0, 0.0
    mask[4096:4098] = True
    res = _K().rank_metric_long(s.to(DEV), y.to(DEV), mask.to(DEV))
    want = _M().rank_metric_torch(s.double(), y.double(), mask)
    assert (want[:, 2] + want[:, 3] <= n - 4096).all().item()
    _compare(res, want, f"n={n} distinct t=3, the first 4096 rows masked out")


def test_columns_without_both_classes():
    n = 8193
    s, y, _ = _inputs(n, "distinct", 3)
    y = y.clone()
    y[:, 0] = 1.0  # no negatives
    y[:, 2] = 0.0  # no positives
    res = _K().rank_metric_long(s.to(DEV), y.to(DEV))
    _compare(res, _M().rank_metric_torch(s.double(), y.double()),
             f"n={n} t=3, a column without negatives and one without positives")
    assert torch.isnan(res[0, :2]).all().item() and res[0, 2].item() == n and res[0, 3].item() == 0
    assert torch.isnan(res[2, :2]).all().item() and res[2, 2].item() == 0 and res[2, 3].item() == n
    # targets that are neither 0 nor 1 are ignored, like masked entries
    y2, mask = _inputs(n, "distinct", 3)[1].clone(), torch.ones(n, 3, dtype=torch.bool)
    y2[5:40], y2[4090:4200] = 2.0, -1.0
    mask[5:40], mask[4090:4200] = False, False
    a = _K().rank_metric_long(s.to(DEV), y2.to(DEV))
    b = _K().rank_metric_long(s.to(DEV), _inputs(n, "distinct", 3)[1].to(DEV), mask.to(DEV))
    assert torch.equal(a, b) and torch.isfinite(a).all().item()


def test_33_runs_six_passes_once():
    n = (1 << 17) + 1
    _run(n, "distinct", 1, True)


@pytest.mark.parametrize("n", (2, 257, 4096))
def test_short_columns_through_the_long_entry(n):
    """AUROC, P and N: the integer sum is exact and divided once, so the bits are the short kernel's.  AP: both
    are fp64 sums of at most n terms (relative error at most n 2^-53), each rounded once to fp32: one ulp."""
    K = _K()
    s, y, mask = (x.to(DEV) for x in _inputs(n, "distinct" if n != 257 else "five", 3))
    short, long_ = K.rank_metric(s, y, mask), K.rank_metric_long(s, y, mask)
    assert torch.isfinite(short).all().item()
    assert torch.equal(short[:, [0, 2, 3]], long_[:, [0, 2, 3]])
    ap, other = short[:, 1], long_[:, 1]
    up, down = torch.nextafter(ap, torch.ones_like(ap)), torch.nextafter(ap, torch.zeros_like(ap))
    print(f"RANKERR ap-vs-short {(ap.double() - other.double()).abs().max().item():.3e} n={n}")
    assert ((other == ap) | (other == up) | (other == down)).all().item()


def test_two_calls_and_a_dirty_workspace_return_the_same_bits():
    K = _K()
    from notorch_amd import _lib

    for n, kind in ((20480, "five"), (8193, "distinct")):
        s, y, mask = (x.to(DEV) for x in _inputs(n, kind, 3))
        a, b = K.rank_metric_long(s, y, mask), K.rank_metric_long(s, y, mask)
        assert torch.equal(a, b) and torch.isfinite(a).all().item()
        need = _lib.load().nt_rank_metric_long_workspace(n, 3)
        dirty = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
        clean = torch.zeros(need, dtype=torch.uint8, device=DEV)
        assert torch.equal(K.rank_metric_long(s, y, mask, dirty), a)
        assert torch.equal(K.rank_metric_long(s, y, mask, clean), a)
        with pytest.raises(_lib.NativeLibraryError, match="workspace"):
            K.rank_metric_long(s, y, mask, clean[: need - 16])


def test_modules_route_by_size_and_agree(monkeypatch):
    K, M = _K(), _M()
    real, seen = K.rank_metric_long, []

    def counted(*args):
        seen.append(tuple(args[0].shape))
        return real(*args)

    monkeypatch.setattr(K, "rank_metric_long", counted)
    # binary pools the b x t entries into one ranking: 1366 x 3 = 4098 rows
    s3, y3, m3 = _inputs(1366, "five", 3)
    want = M.rank_metric_torch(s3.reshape(-1, 1).double(), y3.reshape(-1, 1).double(), m3.reshape(-1, 1))[0, 0].item()
    s8, y8, m8 = _inputs(8193, "distinct", 3)
    want8 = M.rank_metric_torch(s8.double(), y8.double(), m8)[:, 1].mean().item()
    by_default = {rows: [(rows, t)] if rows <= M.RANK_LONG_DEFAULT_MAX_N else [] for rows, t in ((4098, 1), (8193, 3))}
    for knob, hit in (("kernel", True), ("torch", False), (None, None)):
        if knob is None:
            monkeypatch.delenv("NT_LOSS", raising=False)
        else:
            monkeypatch.setenv("NT_LOSS", knob)
        seen.clear()
        out = M.AUROC("binary")(s3.to(DEV), y3.to(DEV), mask=m3.to(DEV))
        assert seen == ([(4098, 1)] if hit else [] if hit is False else by_default[4098]), knob
        assert abs(out.item() - want) <= TOL
        seen.clear()
        out = M.AUPRC("multilabel")(s8.to(DEV), y8.to(DEV), mask=m8.to(DEV))
        assert seen == ([(8193, 3)] if hit else [] if hit is False else by_default[8193]), knob
        assert abs(out.item() - want8) <= TOL
    # bf16 scores are widened as on the short route; CPU and fp64 inputs never reach the kernel
    monkeypatch.setenv("NT_LOSS", "kernel")
    seen.clear()
    sb = s8.bfloat16()
    out = M.AUPRC("multilabel")(sb.to(DEV), y8.to(DEV), mask=m8.to(DEV))
    wantb = M.rank_metric_torch(sb.double(), y8.double(), m8)[:, 1].mean().item()
    assert seen == [(8193, 3)] and abs(out.item() - wantb) <= TOL
    seen.clear()
    cpu = M.AUPRC("multilabel")(s8, y8, mask=m8)
    f64 = M.AUPRC("multilabel")(s8.double().to(DEV), y8.double().to(DEV), mask=m8.to(DEV))
    assert seen == [] and abs(cpu.item() - want8) <= TOL and abs(f64.item() - want8) <= 1e-12
