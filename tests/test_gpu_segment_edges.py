"""nt_segment_reduce, nt_segment_reduce_chunked and nt_segment_arg at their seams, each against the
plain CPU references of tests/segment_ref.py (fp64 truth; the same loop in fp32 where the kernel
claims the CPU's order bit for bit).

Branch -> test
  segment_reduce fp32 scalar kernel (h % 4 != 0)            test_reduce_f32[13-*]
  scalar kernel by pointer alignment                        test_reduce_f32_unaligned_pointer
  vec4 kernel (h / 4 < 32), 31 pieces                       test_reduce_f32[124-*]
  wave kernel PPL = 1, 32 / 64 pieces                       test_reduce_f32[128-*], [256-*]
  wave kernel PPL = 2, 65 / 128 pieces                      test_reduce_f32[260-*], [512-*]
  wave kernel second c0 pass (129 pieces)                   test_reduce_f32[516-*]
  four-row unroll: segment lengths 3, 4, 5, 8, 9, 37        every test_reduce_* (one CSR)
  vec4 grid stride (> 256 * 32 * 256 lanes)                 test_reduce_f32_grid_stride[70001-124]
  wave grid stride (> 8192 waves)                           test_reduce_f32_grid_stride[8229-128]
  runtime-activation instance                               SiLU in test_reduce_f32 / test_reduce_bf16
  +-inf rows, all-negative column                           test_reduce_f32_inf_and_negative
  segment_reduce bf16 pieces 1 / 4 / 8 / 4                  test_reduce_bf16[13], [36], [64], [300]
  chunked fp32 scalar / vector, bf16 scalar / vector        test_chunked[13 | 36 | 40 | 132 x dtype]
  chunks 31 / 32 / 33 / 64 / 65 rows; < = > 32 chunks       test_chunked (lengths 1023, 1024, 1025, 1281)
  pass 2 slab tail (33 pieces)                              test_chunked[132-float32]
  pass 2 at 1024 and 256 threads                            test_chunked_block_sizes_same_bits
  pass 2 grid stride (> 4096 blocks)                        test_chunked_pass2_grid_stride
  chunked scalar instance by pointer alignment              test_chunked_unaligned_pointer
  chunked amax, both passes                                 test_chunked_amax
  segment_arg fp32 / bf16, ties, +-0, empty                 test_segment_arg

NaN ordering in max / min is out of scope: no input here holds a NaN, and no segment column sums
+inf with -inf.
"""
import functools

import pytest
import torch

import segment_ref as R
from helpers import assert_parity, norm_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
ULP = 2.0 ** -8
REDUCES = ("sum", "mean", "max", "min")
COUNTS = [0, 1, 3, 4, 5, 8, 9, 0, 37, 2] * 20  # 200 segments, 1380 rows
LONG_COUNTS = [0, 1, 31, 32, 33, 64, 65, 1023, 1024, 1025, 1281, 5]


def _K():
    from notorch_amd import kernels

    return kernels


def _code(name):
    return _K().act_code(R.ACTS[name])


def _device_csr(idx, nseg, shuffled):
    """The CSR through K.csr_build; perm = None for rows stored segment by segment."""
    seg_ptr, perm = _K().csr_build(idx.to(DEV), nseg)
    return seg_ptr, (perm if shuffled else None)


@functools.lru_cache(maxsize=None)
def _short_case(h, shuffled, dtype=torch.float32):
    idx = R.index_from_counts(COUNTS, shuffle_seed=h if shuffled else None)
    X = torch.randn(len(idx), h, generator=torch.Generator().manual_seed(h)).to(dtype)
    seg_ptr, perm = R.csr(idx, len(COUNTS))
    return idx, X, seg_ptr, (perm if shuffled else None)


# ------------------------------------------------------------------ 1. segment_reduce, fp32
@pytest.mark.parametrize("shuffled", [True, False], ids=["perm", "contiguous"])
@pytest.mark.parametrize("h", [13, 124, 128, 256, 260, 512, 516])
def test_reduce_f32(h, shuffled):
    """Sum / mean: the sequential fp32 sum in ascending CSR position, bit for bit (Identity, ReLU), and
    the fp64 reference at 1e-6 normalised (every activation).  Max / min: exact (Identity, ReLU)."""
    K = _K()
    idx, X, seg_ptr, perm = _short_case(h, shuffled)
    d_ptr, d_perm = _device_csr(idx, len(COUNTS), shuffled)
    Xd = X.to(DEV)
    for act in ("Identity", "ReLU", "SiLU"):
        for reduce in REDUCES:
            got = K.segment_reduce(Xd, d_ptr, d_perm, len(COUNTS), reduce=reduce, act=_code(act)).cpu()
            what = f"segment_reduce {reduce} {act} h={h}"
            assert_parity(got, R.segment_reduce_ref(X, seg_ptr, perm, reduce, R.ACTS[act]), 1e-6, what)
            if act != "SiLU":
                ref32 = R.segment_reduce_ref(X, seg_ptr, perm, reduce, R.ACTS[act], dtype=torch.float32)
                assert torch.equal(got, ref32), what


def test_reduce_f32_unaligned_pointer():
    """X and out one float into their buffers (data_ptr % 16 == 4): the scalar kernel, same bits."""
    K = _K()
    h, nseg = 128, len(COUNTS)
    idx, X, _, _ = _short_case(h, True)
    d_ptr, d_perm = _device_csr(idx, nseg, True)
    Xd = X.to(DEV)
    xbuf = torch.empty(X.numel() + 4, device=DEV)
    Xu = xbuf[1:1 + X.numel()].view(X.shape).copy_(Xd)
    obuf = torch.zeros(nseg * h + 4, device=DEV)
    out_u = obuf[1:1 + nseg * h].view(nseg, h)
    assert Xu.data_ptr() % 16 == 4 and out_u.data_ptr() % 16 == 4 and Xd.data_ptr() % 16 == 0
    for act in ("Identity", "ReLU"):
        for reduce in REDUCES:
            want = K.segment_reduce(Xd, d_ptr, d_perm, nseg, reduce=reduce, act=_code(act))
            got = K.segment_reduce(Xu, d_ptr, d_perm, nseg, reduce=reduce, act=_code(act), out=out_u)
            assert got.data_ptr() == out_u.data_ptr()
            assert torch.equal(got, want), f"{reduce} {act}"
    assert obuf[0] == 0 and (obuf[1 + nseg * h:] == 0).all()  # nothing written outside the view


@pytest.mark.parametrize("nseg,h", [(70_001, 124), (8192 + 37, 128)])
def test_reduce_f32_grid_stride(nseg, h):
    """More lanes than the vec4 grid holds (70 001 x 31 pieces > 256 * 32 * 256) and more segments than
    the wave grid has waves (8192): every segment still reduced, in order."""
    K = _K()
    counts = ([1, 2, 0, 3] * (nseg // 4 + 1))[:nseg]
    idx = R.index_from_counts(counts, shuffle_seed=nseg)
    X = torch.randn(len(idx), h, generator=torch.Generator().manual_seed(nseg))
    seg_ptr, perm = R.csr(idx, nseg)
    d_ptr, d_perm = _device_csr(idx, nseg, True)
    Xd = X.to(DEV)
    for reduce in ("sum", "max"):
        got = K.segment_reduce(Xd, d_ptr, d_perm, nseg, reduce=reduce).cpu()
        assert torch.equal(got, R.segment_reduce_ref(X, seg_ptr, perm, reduce, dtype=torch.float32)), reduce


@pytest.mark.parametrize("h", [13, 124, 128, 260, 516])
def test_reduce_f32_inf_and_negative(h):
    """Max / min pass +-inf through (a column of -inf alone gives -inf, not -FLT_MAX) and an
    all-negative column keeps its sign under max / Identity; ReLU maps -inf to 0 and keeps +inf."""
    K = _K()
    idx, X, seg_ptr, perm = _short_case(h, True)
    X = X.clone()
    inf = float("inf")
    X[:, 0] = -X[:, 0].abs() - 0.25                       # all negative
    rows3 = perm[seg_ptr[2]:seg_ptr[3]]                   # a 3-row segment: every row -inf / +inf
    X[rows3, 1], X[rows3, 2] = -inf, inf
    rows37 = perm[seg_ptr[8]:seg_ptr[9]]                  # a 37-row segment: one of each among finite values
    X[rows37[5], 3], X[rows37[36], 4] = -inf, inf
    X[rows37[0], 5], X[rows37[17], 6] = inf, -inf
    d_ptr, d_perm = _device_csr(idx, len(COUNTS), True)
    for act in ("Identity", "ReLU"):
        for reduce in ("max", "min"):
            got = K.segment_reduce(X.to(DEV), d_ptr, d_perm, len(COUNTS), reduce=reduce, act=_code(act)).cpu()
            ref = R.segment_reduce_ref(X, seg_ptr, perm, reduce, R.ACTS[act], dtype=torch.float32)
            assert torch.equal(got, ref), f"{reduce} {act}"
    got = K.segment_reduce(X.to(DEV), d_ptr, d_perm, len(COUNTS), reduce="max").cpu()
    nonempty = torch.tensor(COUNTS) > 0
    assert (got[nonempty, 0] < 0).all() and (got[~nonempty] == 0).all()
    assert got[2, 1] == -inf and got[2, 2] == inf and got[8, 4] == inf and got[8, 5] == inf
    got = K.segment_reduce(X.to(DEV), d_ptr, d_perm, len(COUNTS), reduce="min").cpu()
    assert got[2, 1] == -inf and got[2, 2] == inf and got[8, 3] == -inf and got[8, 6] == -inf


# ------------------------------------------------------------------ 2. segment_reduce, bf16
@pytest.mark.parametrize("shuffled", [True, False], ids=["perm", "contiguous"])
@pytest.mark.parametrize("h", [13, 36, 64, 300])  # pieces of 1, 4, 8, 4 elements
def test_reduce_bf16(h, shuffled):
    """fp32 accumulation of the exactly widened inputs, one rounding: max / min exact, sum / mean
    within one bf16 ulp (normalised) of the fp32 sequential sum rounded once."""
    K = _K()
    idx, X, seg_ptr, perm = _short_case(h, shuffled, BF16)
    d_ptr, d_perm = _device_csr(idx, len(COUNTS), shuffled)
    for act in ("Identity", "ReLU", "SiLU"):
        for reduce in REDUCES:
            got = K.segment_reduce(X.to(DEV), d_ptr, d_perm, len(COUNTS), reduce=reduce, act=_code(act)).cpu()
            assert got.dtype == BF16
            ref = R.segment_reduce_ref(X.float(), seg_ptr, perm, reduce, R.ACTS[act], dtype=torch.float32)
            what = f"segment_reduce bf16 {reduce} {act} h={h}"
            if reduce in ("max", "min") and act != "SiLU":
                assert torch.equal(got, ref.to(BF16)), what
            else:  # the kernel's one rounding of that fp32 value
                assert_parity(got.float(), ref, ULP, what)


# ------------------------------------------------------------------ 3. segment_reduce_chunked
@functools.lru_cache(maxsize=None)
def _long_case(h, dtype):
    idx = R.index_from_counts(LONG_COUNTS, shuffle_seed=h)
    X = (torch.randn(len(idx), h, generator=torch.Generator().manual_seed(h + 1)) + 0.25).to(dtype)
    seg_ptr, perm = R.csr(idx, len(LONG_COUNTS))
    return idx, X, seg_ptr, perm


def _err32_sum(X, idx, nseg, act, reduce, ref):
    """Normalised error of a plain fp32 CPU index_add_ against the fp64 reference."""
    s = torch.zeros(nseg, X.shape[1]).index_add_(0, idx, act(X.float()))
    if reduce == "mean":
        s = s / R.counts(idx, nseg, torch.float32)[:, None]
    return norm_err(s, ref)


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("h", [13, 36, 40, 132])
def test_chunked(h, dtype):
    """Segments of 0 .. 1281 rows (1 .. 41 chunks of 32; pass 2's 32 sub-ranges partly empty, full,
    and holding two chunks).  Max / min: the bits of the unchunked kernel.  Sum / mean: regrouped
    fp32 sums, within max(1e-6, 4 x err32) of fp64 (err32: a plain fp32 index_add_ on the CPU);
    bf16 within one ulp.

    Measured on an MI355X (normalised, against fp64; the range over h and the two activations):
    sum  err32 7.0e-7 .. 1.5e-6 (worst h = 36, Identity), kernel 1.6e-7 .. 2.4e-7;
    mean err32 1.1e-7 .. 3.3e-7 (worst h = 36, ReLU),     kernel 3.7e-8 .. 8.7e-8.
    The regrouped sums sit below the serial fp32 order: 41 partial sums of 32 rows carry less rounding
    than one 1281-term chain."""
    K = _K()
    nseg = len(LONG_COUNTS)
    idx, X, seg_ptr, perm = _long_case(h, dtype)
    d_ptr, d_perm = _device_csr(idx, nseg, True)
    plan = K.chunk_plan(d_ptr)
    assert plan[1] == sum((c + 31) // 32 for c in LONG_COUNTS)
    Xd = X.to(DEV)
    for act in ("Identity", "ReLU"):
        for reduce in REDUCES:
            got = K.segment_reduce_chunked(Xd, d_ptr, d_perm, nseg, plan, reduce=reduce, act=_code(act))
            what = f"chunked {reduce} {act} h={h} {dtype}"
            ref = R.segment_reduce_ref(X, seg_ptr, perm, reduce, R.ACTS[act])
            if reduce in ("max", "min"):
                plain = K.segment_reduce(Xd, d_ptr, d_perm, nseg, reduce=reduce, act=_code(act))
                assert torch.equal(got, plain), what
                assert torch.equal(got.cpu().double(), ref), what
            elif dtype == BF16:
                assert_parity(got.float(), ref, ULP, what)
            else:
                err32 = _err32_sum(X, idx, nseg, R.ACTS[act], reduce, ref)
                err = norm_err(got, ref)
                print(f"{what}: err32 {err32:.3e} kernel {err:.3e}")
                assert err <= max(1e-6, 4 * err32), f"{what}: {err:.3e} vs err32 {err32:.3e}"


@pytest.mark.parametrize("h,dtype", [(40, torch.float32), (13, torch.float32), (132, torch.float32), (40, BF16)])
def test_chunked_block_sizes_same_bits(h, dtype):
    """Pass 2 runs 1024-thread blocks below 1024 blocks and 256-thread blocks from there: the 1281-
    and 65-row segments reduced alone and ahead of 1100 two-chunk segments give the same bits."""
    K = _K()
    small, big = [1281, 65], [1281, 65] + [33] * 1100
    X = torch.randn(sum(big), h, generator=torch.Generator().manual_seed(h)).to(dtype).to(DEV)
    outs = []
    for counts in (small, big):
        idx = R.index_from_counts(counts)
        d_ptr, _ = _device_csr(idx, len(counts), False)
        plan = K.chunk_plan(d_ptr)
        piece = 4 if dtype == torch.float32 else 8
        nslab = (h // (piece if h % piece == 0 else 1) + 31) // 32  # pass 2: a block per 32 pieces
        assert (plan[4].numel() * nslab < 1024) == (counts is small)
        outs.append([K.segment_reduce_chunked(X[:len(idx)], d_ptr, None, len(counts), plan, reduce=r,
                                              act=_code("ReLU")) for r in REDUCES])
    for r, a, b in zip(REDUCES, *outs):
        assert torch.equal(a, b[:2]), r


def test_chunked_pass2_grid_stride():
    """4200 two-chunk segments: more pass-2 blocks than its grid (4096).  Against fp64, and the first
    and last segments bit-equal to a launch of six segments.
    Measured on an MI355X: err32 2.567e-7, kernel 2.567e-7 (33-row segments: the same worst element)."""
    K = _K()
    h, nseg, rows = 40, 4200, 33
    X = torch.randn(nseg * rows, h, generator=torch.Generator().manual_seed(7))
    idx = R.index_from_counts([rows] * nseg)
    seg_ptr, _ = R.csr(idx, nseg)
    d_ptr, _ = _device_csr(idx, nseg, False)
    got = K.segment_reduce_chunked(X.to(DEV), d_ptr, None, nseg, K.chunk_plan(d_ptr), reduce="sum").cpu()
    ref = R.segment_reduce_ref(X, seg_ptr, None, "sum")
    err32 = _err32_sum(X, idx, nseg, R.ACTS["Identity"], "sum", ref)
    err = norm_err(got, ref)
    print(f"pass-2 grid stride: err32 {err32:.3e} kernel {err:.3e}")
    assert err <= max(1e-6, 4 * err32)
    Xs = torch.cat([X[:3 * rows], X[-3 * rows:]])
    s_ptr, _ = _device_csr(R.index_from_counts([rows] * 6), 6, False)
    few = K.segment_reduce_chunked(Xs.to(DEV), s_ptr, None, 6, K.chunk_plan(s_ptr), reduce="sum").cpu()
    assert torch.equal(torch.cat([got[:3], got[-3:]]), few)


def test_chunked_unaligned_pointer():
    """h = 40 fp32 with X and out one float into their buffers: the scalar instances, same bits."""
    K = _K()
    h, nseg = 40, len(LONG_COUNTS)
    idx, X, _, _ = _long_case(h, torch.float32)
    d_ptr, d_perm = _device_csr(idx, nseg, True)
    plan = K.chunk_plan(d_ptr)
    Xd = X.to(DEV)
    Xu = torch.empty(X.numel() + 4, device=DEV)[1:1 + X.numel()].view(X.shape).copy_(Xd)
    obuf = torch.zeros(nseg * h + 4, device=DEV)
    out_u = obuf[1:1 + nseg * h].view(nseg, h)
    assert Xu.data_ptr() % 16 == 4 and out_u.data_ptr() % 16 == 4
    for reduce in REDUCES:
        want = K.segment_reduce_chunked(Xd, d_ptr, d_perm, nseg, plan, reduce=reduce, act=_code("ReLU"))
        got = K.segment_reduce_chunked(Xu, d_ptr, d_perm, nseg, plan, reduce=reduce, act=_code("ReLU"), out=out_u)
        assert torch.equal(got, want), reduce
    assert obuf[0] == 0 and (obuf[1 + nseg * h:] == 0).all()


@pytest.mark.parametrize("h", [13, 40])
@pytest.mark.parametrize("reduce", REDUCES)
def test_chunked_amax(h, reduce):
    """amax = max|out| exactly, over the rows pass 1 stores (single-chunk segments) and pass 2's."""
    K = _K()
    nseg = len(LONG_COUNTS)
    idx, X, _, _ = _long_case(h, torch.float32)
    X = X.clone()
    X[idx == 1] *= 50  # the largest row belongs to a single-chunk segment for max; pass 2 holds the sums'
    d_ptr, d_perm = _device_csr(idx, nseg, True)
    amax = torch.zeros(1, device=DEV)
    out = K.segment_reduce_chunked(X.to(DEV), d_ptr, d_perm, nseg, K.chunk_plan(d_ptr), reduce=reduce, amax=amax)
    assert amax.item() == out.abs().max().item() and amax.item() > 0


# ------------------------------------------------------------------ 4. segment_arg
ARG_COUNTS = [0, 1, 2, 7, 40] * 3


@pytest.mark.parametrize("shuffled", [True, False], ids=["perm", "contiguous"])
@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("h", [13, 32])
def test_segment_arg(h, dtype, shuffled):
    """Integer inputs -3 .. 3 (ties in most columns), a segment of (-0.0, +0.0) alone, a column that
    is 0 everywhere after ReLU: the first row in CSR order wins, empty segments give -1; and the
    forward's max / min is act(X) at that row, bit for bit."""
    K = _K()
    nseg = len(ARG_COUNTS)
    idx = R.index_from_counts(ARG_COUNTS, shuffle_seed=h if shuffled else None)
    seg_ptr, perm = R.csr(idx, nseg)
    X = torch.randint(-3, 4, (len(idx), h), generator=torch.Generator().manual_seed(h)).float()
    X[:, 0] = -1.0 - X[:, 0].abs()                        # negative: ReLU makes the column one long tie
    pair = perm[seg_ptr[2]:seg_ptr[3]]
    X[pair[0]], X[pair[1]] = -0.0, 0.0                    # equal under > and <: the first row
    seven = perm[seg_ptr[3]:seg_ptr[4]]
    X[seven[2], 1:] = 0.0
    X[seven[4], 1:] = -0.0
    X = X.to(dtype)
    d_ptr, d_perm = _device_csr(idx, nseg, shuffled)
    r_perm = perm if shuffled else None
    Xd = X.to(DEV)
    rows_ptr = torch.arange(len(idx) + 1, dtype=torch.int32, device=DEV)
    for act in ("Identity", "ReLU", "Tanh"):
        Y = R.ACTS[act](X.double())
        # act(X) as the device evaluates it: one row per segment
        Yd = K.segment_reduce(Xd, rows_ptr, None, len(idx), reduce="max", act=_code(act))
        if act != "Tanh":
            assert torch.equal(Yd.cpu().double(), Y)
        for reduce in ("max", "min"):
            what = f"segment_arg {reduce} {act} h={h}"
            arg = K.segment_arg(Xd, d_ptr, d_perm, nseg, reduce, act=_code(act))
            assert arg.dtype == torch.int32 and arg.shape == (nseg, h)
            want = R.segment_arg_ref(Y, seg_ptr, r_perm, reduce)
            assert torch.equal(arg.cpu(), want), what
            val = K.segment_reduce(Xd, d_ptr, d_perm, nseg, reduce=reduce, act=_code(act))
            live = torch.tensor(ARG_COUNTS, device=DEV) > 0
            picked = Yd.gather(0, arg[live].long())
            assert torch.equal(val[live], picked), what
            assert (arg[~live] == -1).all() and (val[~live] == 0).all(), what
