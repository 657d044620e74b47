"""GPU: the ranking kernels where tests/test_gpu_rank_metric.py and tests/test_gpu_rank_metric_long.py stop.

The scheme is theirs: rank_metric_torch in fp64 on the CPU as yardstick, AUROC and AP within 1e-5 absolute and
in [0, 1], P and N exact, ``RANKERR <metric> <value> <case>`` lines.  Added here:
  * nt_rank_metric_long above 1024 tiles, where rank_long_carries_kernel and rank_long_finish_kernel take a
    second step of their 1024-tile loops and the running carries (run_pre, run_prev) are first used:
      n = 1024 * 4096 + 1 (1025 tiles), no mask, so that every row is live and the sorted live rows reach into
          tile 1024, the only tile of the second step: with distinct scores and with five score values, whose
          lowest tie group (~839k rows) runs from about tile 819 through sorted position 1024 * 4096 and closes
          there, taking the counts at the group end before it from run_prev (the test asserts where the
          groups lie);
      n = 2049 * 4096 (three steps): all scores equal, where no tile but the last has a group end (run_pre is
          carried, run_prev stays 0), and five score values, whose group ends near tiles 1229 and 1639 make the
          later tiles of the second step compare a group end of their own step with the carried one;
  * special scores on both entries: runs of +inf and -inf, of -0.0 mixed with +0.0 under both labels, the
    smallest and largest denormals and +-3.4e38 planted in randn columns (on the long entry the +-0 group and
    the -inf group straddle row 4096), and a column whose every score is -inf, one group whose key sits next
    to the key of ignored entries.  No NaN scores: the torch route defines no order for them.
"""
import time

import pytest
import torch

from test_gpu_rank_metric_long import DEV, _compare, _inputs, _K, _M, _want

pytestmark = pytest.mark.gpu

DENORM_MIN, DENORM_MAX = 2.0 ** -149, 2.0 ** -126 - 2.0 ** -149
WINDOW = 48  # rows of the +-0 / -inf plant


def _timed_long(s, y, mask, case):
    K = _K()
    s, y, mask = s.to(DEV), y.to(DEV), None if mask is None else mask.to(DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = K.rank_metric_long(s, y, mask)
    torch.cuda.synchronize()
    print(f"RANKTIME {1e3 * (time.perf_counter() - t0):.3f} ms first call {case}")
    return res, K.rank_metric_long(s, y, mask)


def _end_tiles(s):
    """The tiles (of 4096 sorted positions) in which a group of equal scores ends; every row is live."""
    d = s[:, 0].sort(descending=True).values
    ends = torch.cat([(d[1:] != d[:-1]).nonzero().flatten(), torch.tensor([d.numel() - 1])])
    return d, ends // 4096


@pytest.mark.parametrize("kind", ("distinct", "five"))
def test_1025_tiles(kind):
    """No mask: all 1024 * 4096 + 1 rows are live, so the one live row of tile 1024, the only tile of the second
    step, closes a group there and takes the counts at the group end before it from run_prev."""
    n = 1024 * 4096 + 1
    s, y, _ = _inputs(n, kind, 1)
    d, end_tiles = _end_tiles(s)
    assert end_tiles[-1].item() == 1024 and (end_tiles < 1024).any().item()
    if kind == "five":  # the lowest group runs from about tile 819 through sorted position 1024 * 4096
        assert d[1024 * 4096].item() == d[1024 * 4096 - 1].item() == d[820 * 4096].item() == -0.5
        assert len(end_tiles) == 5
    t0 = time.perf_counter()
    want = _want(n, kind, 1, False)
    print(f"RANKTIME {time.perf_counter() - t0:.3f} s the fp64 torch route on the CPU, n={n}")
    res, again = _timed_long(s, y, None, f"n={n} {kind}")
    _compare(res, want, f"n={n} {kind} t=1 masked=False (1025 tiles)")
    assert torch.equal(res, again)


@pytest.mark.parametrize("kind", ("equal", "five"))
def test_2049_tiles(kind):
    """Three steps of the carry loop.  equal: one group, no group end before the last tile, so run_prev stays 0 and
    only run_pre is carried.  five: groups of ~1.68M rows end near tiles 410, 820, 1229, 1639 and in 2048; in
    the second step the tiles behind 1229 compare a group end of their own step with the carried one, both non-zero."""
    n = 2049 * 4096
    s, y, _ = _inputs(n, kind, 1)
    _, end_tiles = _end_tiles(s)
    if kind == "equal":
        assert end_tiles.tolist() == [2048]
    else:
        in_second = ((end_tiles >= 1024) & (end_tiles < 2047)).sum().item()
        assert len(end_tiles) == 5 and (end_tiles < 1024).any().item() and in_second >= 1 and end_tiles[-1].item() == 2048
    want = _want(n, kind, 1, False)
    res, again = _timed_long(s, y, None, f"n={n} {kind}")
    _compare(res, want, f"n={n} {kind} t=1 masked=False (2049 tiles)")
    assert torch.equal(res, again)
    if kind == "equal":
        assert res[0, 0].item() == 0.5 and want[0, 0].item() == 0.5


def _special(n, t=3):
    """randn columns 0 and 1 with the planted runs, column 2 all -inf; random labels and mask, the planted rows
    live.  Returns (scores, targets, mask, rows of the -0, +0 and -inf plants)."""
    gen = torch.Generator().manual_seed(77 * n + t)
    s = torch.randn(n, t, generator=gen)
    y = (torch.rand(n, t, generator=gen) < 0.4).float()
    mask = torch.rand(n, t, generator=gen) < 0.7
    s[3:10, :2] = float("inf")
    for k, v in enumerate((DENORM_MIN, -DENORM_MIN, DENORM_MAX, -DENORM_MAX)):
        s[12 + 2 * k: 14 + 2 * k, :2] = v
    s[22:25, :2], s[25:28, :2] = 3.4e38, -3.4e38
    mask[:28] = True
    y[0], y[1] = 1.0, 0.0
    # a window that straddles row 4096 of the long entry (n = 4097 has one row past it): zeros and -inf
    # alternate, column 1 one row out of step with column 0, so that row 4096 is a -inf in one and a zero in the other
    lo = min((4096 if n > 4096 else n // 2) - WINDOW // 2, n - WINDOW)
    idx = torch.arange(WINDOW)
    rows = lo + idx
    neg = (idx // 2) % 2 == 1
    plants = []
    for col in (0, 1):
        zero = idx % 2 == col
        s[rows[zero & neg], col], s[rows[zero & ~neg], col] = -0.0, 0.0
        s[rows[~zero], col] = float("-inf")
        plants.append((rows[zero & neg], rows[zero & ~neg], rows[~zero]))
    y[rows] = ((idx // 4) % 2).float().unsqueeze(1).expand(WINDOW, t)
    mask[rows] = True
    s[:, 2] = float("-inf")
    return s, y, mask, plants


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("n", (257, 4096, 4097, 8193))
def test_special_scores(n, masked):
    K, M = _K(), _M()
    s, y, mask, plants = _special(n)
    straddles = []
    for col, (m0, p0, ninf) in enumerate(plants):
        for rows in (m0, p0):  # at least ten of each zero, labelled both ways
            assert len(rows) >= 10 and set(y[rows, col].tolist()) == {0.0, 1.0}
        assert torch.signbit(s[m0, col]).all().item() and not torch.signbit(s[p0, col]).any().item()
        assert (s[m0, col] == 0).all().item() and (s[p0, col] == 0).all().item()
        assert (s[ninf, col] == float("-inf")).all().item() and len(ninf) == WINDOW // 2
        zeros = torch.cat([m0, p0])
        straddles.append((zeros.min().item() < 4096 <= zeros.max().item(), ninf.min().item() < 4096 <= ninf.max().item()))
    if n > 4096:  # each group straddles row 4096 in some column (in both from n = 4096 + WINDOW / 2 on)
        assert any(z for z, _ in straddles) and any(i for _, i in straddles)
        assert n == 4097 or all(z and i for z, i in straddles)
    assert (s[:, 0] == DENORM_MIN).sum().item() == 2 and (s[:, 0] == -DENORM_MAX).sum().item() == 2 and DENORM_MIN > 0
    mask = mask if masked else None
    want = M.rank_metric_torch(s.double(), y.double(), mask)
    entry = K.rank_metric if n <= K.rank_metric_max_n() else K.rank_metric_long
    res = entry(s.to(DEV), y.to(DEV), None if mask is None else mask.to(DEV))
    _compare(res, want, f"n={n} t=3 special scores masked={masked} ({entry.__name__})")
    assert res[2, 0].item() == 0.5 and want[2, 0].item() == 0.5  # the all -inf column: one group
    assert torch.equal(res, entry(s.to(DEV), y.to(DEV), None if mask is None else mask.to(DEV)))
