"""csrc/backward.hip kernel by kernel (message, edge backward, gather rows and their max / min arg
versions, fp32 and bf16) against the index-expression references of tests/segment_ref.py, and the
argument checks of the Python wrappers around them.

Branch -> test
  message_kernel<float4> / <float>, message_bf16<VEC> / <scalar>      test_message[16 | 64, 13 | 36 x dtype]
  edge_backward_kernel<float4> / <float>, sum and mean                test_edge_backward[16 | 64, 13 | 36 -float32-*]
  edge_backward_bf16<VEC> (64) / <scalar> (13, 16, 36)                test_edge_backward[*-bfloat16-*]
  gather_rows_kernel<float4> / <float>, gather_rows_bf16              test_gather_rows
  runtime activation, each of the eight codes (act_grad)              test_message, test_edge_backward (loop)
  residual off with G = None; rows 0 / 1 / several rows reverse into  test_edge_backward ("nodes" collate)
  isolated node, in-degree 1, in-degree 0 under mean                  _graph()'s two added nodes
  grid stride of edge backward / gather rows                          test_grid_stride
  amax of edge backward / gather rows                                 test_edge_backward, test_gather_rows (fp32)
  edge_backward_arg_kernel<float4, int4> / <float, int> / bf16        test_edge_backward_arg[16 | 64, 13 x dtype]
  gather_rows_arg_kernel<float4, int4> / <float, int> / bf16          test_gather_rows_arg
  scalar arg instances by arg's alignment                             test_arg_unaligned
  amax of the arg kernels                                             test_edge_backward_arg, test_gather_rows_arg
  wrapper argument checks (no library call)                           test_*_rejects, test_amax_is_fp32_only
"""
import functools

import pytest
import torch

import segment_ref as R
from helpers import assert_parity, norm_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
F32 = torch.float32
ULP = 2.0 ** -8
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
COLLATES = pytest.mark.parametrize("collate", ["nodes", "edges"])
PLANT = [-100.0, -20.0, -0.0, 0.0, 20.0, 100.0]  # saturated ends, and the x = 0 conventions


def _K():
    from notorch_amd import kernels

    return kernels


def _code(name):
    return _K().act_code(R.ACTS[name])


@functools.lru_cache(maxsize=None)
def _graph(collate):
    """(src, dst, rev, V, E) of eight QM9-like molecules plus an isolated node (V - 2) and a node of
    in-degree 1 (V - 1, reached by one extra edge from node 0 whose reverse entry points at row 0).
    collate = "nodes": rev is not a permutation (rows receive 0, 1 or several reversed rows)."""
    from notorch_amd.data.synth import make_batch

    G = make_batch("qm9", 8, seed=3).collate(collate)
    V, E = G.num_nodes, G.num_edges
    src = torch.cat([G.edge_index[0], torch.tensor([0])])
    dst = torch.cat([G.edge_index[1], torch.tensor([V + 1])])
    rev = torch.cat([G.rev_index, torch.tensor([0])])
    return src.contiguous(), dst.contiguous(), rev.contiguous(), V + 2, E + 1


def test_graph_shapes_cover_the_cases():
    src, dst, rev, V, E = _graph("nodes")
    into = torch.bincount(rev, minlength=E)
    assert (into == 0).any() and (into == 1).any() and (into > 1).any()
    deg = torch.bincount(dst, minlength=V)
    assert deg[V - 2] == 0 and deg[V - 1] == 1 and not (src == V - 2).any()
    into = torch.bincount(_graph("edges")[2], minlength=E)
    assert into[0] == 2 and (into[1:-1] == 1).all()


def _rand(n, h, dtype, seed, scale=1.0):
    return (torch.randn(n, h, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _hidden(E, h, dtype, seed):
    H = _rand(E, h, F32, seed, 3.0)
    H[:, 1] = torch.tensor(PLANT).repeat(E // len(PLANT) + 1)[:E]
    return H.to(dtype)


def _device_csrs(dst, rev, V, E):
    K = _K()
    dst_ptr, dst_perm = K.csr_build(dst.to(DEV), V)
    rev_ptr, rev_perm = K.csr_build(rev.to(DEV), E)
    return dst_ptr, dst_perm, rev_ptr, rev_perm


def _compare(got, ref64, ref32, dtype, what, worst):
    """fp32: within max(1e-6, 4 x err32) of fp64 (err32: the same expression in fp32 torch ops on the
    CPU).  bf16: the fp32 restatement rounded once, so within one bf16 rounding (2^-8 normalised) of it,
    as the element tests of test_gpu_bf16_backward.py."""
    if dtype == BF16:
        assert got.dtype == BF16, what
        assert_parity(got.float(), ref32, ULP, what)
        return
    err32, err = norm_err(ref32, ref64), norm_err(got, ref64)
    worst[0], worst[1] = max(worst[0], err32), max(worst[1], err)
    assert err <= max(1e-6, 4 * err32), f"{what}: {err:.3e} vs err32 {err32:.3e}"


# ------------------------------------------------------------------ 5. message / edge backward / gather rows
@COLLATES
@DTYPES
@pytest.mark.parametrize("h", [13, 16, 36, 64])
def test_message(h, dtype, collate):
    """A = S[src] - act(H[rev]) for the eight activations; ReLU and Identity bit-exact (one
    subtraction per element, one rounding in bf16).
    Measured on an MI355X (fp32, worst over the activations, per h and collate): err32 4.1e-8 .. 5.5e-8,
    kernel the same figure to three digits in every case (the planted |H| = 100 sets the scale)."""
    K = _K()
    src, dst, rev, V, E = _graph(collate)
    H, S = _hidden(E, h, dtype, h), _rand(V, h, dtype, h + 1)
    dev = [t.to(DEV) for t in (H, S, src, rev)]
    worst = [0.0, 0.0]
    for act in R.ACTS:
        got = K.dmpnn_message(*dev, act=_code(act)).cpu()
        ref32 = R.message_ref(H.float(), S.float(), src, rev, R.ACTS[act], dtype=F32)
        _compare(got, R.message_ref(H, S, src, rev, R.ACTS[act]), ref32, dtype, f"message {act} h={h}", worst)
        if act in ("ReLU", "Identity"):
            assert torch.equal(got, ref32.to(dtype)), act
    if dtype == F32:
        print(f"message h={h} {collate}: err32 {worst[0]:.3e} kernel {worst[1]:.3e}")


@COLLATES
@DTYPES
@pytest.mark.parametrize("h", [13, 16, 36, 64])
def test_edge_backward(h, dtype, collate):
    """(G or 0) + act'(H) * (dS[dst] / c - scatter(dA, rev)): eight activations x sum / mean x residual
    on / off (off: G = None); fp32 amax = max|out| exactly.
    Measured on an MI355X (fp32, worst over the 32 combinations, per h and collate): err32 2.1e-7 ..
    4.1e-7, kernel 2.1e-7 .. 4.1e-7 (equal to three digits except h = 13 / nodes: 2.059e-7 against
    2.076e-7)."""
    K = _K()
    src, dst, rev, V, E = _graph(collate)
    H = _hidden(E, h, dtype, h)
    G, dA, dS = _rand(E, h, dtype, h + 1), _rand(E, h, dtype, h + 2), _rand(V, h, dtype, h + 3)
    dst_ptr, _, rev_ptr, rev_perm = _device_csrs(dst, rev, V, E)
    Gd, Hd, dAd, dSd, dstd = (t.to(DEV) for t in (G, H, dA, dS, dst))
    worst = [0.0, 0.0]
    for act in R.ACTS:
        for reduce in ("sum", "mean"):
            for residual in (True, False):
                amax = torch.zeros(1, device=DEV) if dtype == F32 else None
                got = K.dmpnn_edge_backward(Gd if residual else None, Hd, dAd, dSd, dstd, rev_ptr, rev_perm,
                                            dst_ptr if reduce == "mean" else None, residual=residual,
                                            act=_code(act), reduce=reduce, amax=amax)
                what = f"edge backward {act} {reduce} residual={residual} h={h}"
                g = G if residual else None
                ref32 = R.edge_backward_ref(None if g is None else g.float(), H.float(), dA.float(), dS.float(),
                                            dst, rev, R.ACTS[act], reduce, dtype=F32)
                ref64 = R.edge_backward_ref(g, H, dA, dS, dst, rev, R.ACTS[act], reduce)
                _compare(got.cpu(), ref64, ref32, dtype, what, worst)
                if amax is not None:
                    assert amax.item() == got.abs().max().item(), what
    if dtype == F32:
        print(f"edge backward h={h} {collate}: err32 {worst[0]:.3e} kernel {worst[1]:.3e}")


@DTYPES
@pytest.mark.parametrize("h", [13, 16, 36, 64])
def test_gather_rows(h, dtype):
    """out[i] = (base[i] or 0) + X[dst i] / c: base on / off, sum / mean (the mean CSR holds nodes of
    in-degree 0 and 1); the plain gather is exact; fp32 amax = max|out| exactly.
    Measured on an MI355X (fp32): err32 4.7e-8 .. 5.7e-8, kernel the same figures."""
    K = _K()
    src, dst, rev, V, E = _graph("nodes")
    X, base = _rand(V, h, dtype, h), _rand(E, h, dtype, h + 1)
    dst_ptr, _ = K.csr_build(dst.to(DEV), V)
    worst = [0.0, 0.0]
    for mean in (False, True):
        for b in (base, None):
            amax = torch.zeros(1, device=DEV) if dtype == F32 else None
            got = K.gather_rows(X.to(DEV), dst.to(DEV), base=None if b is None else b.to(DEV),
                                seg_ptr=dst_ptr if mean else None, amax=amax)
            what = f"gather rows mean={mean} base={b is not None} h={h}"
            ref32 = R.gather_rows_ref(X.float(), dst, None if b is None else b.float(),
                                      R.counts(dst, V, F32) if mean else None, dtype=F32)
            ref64 = R.gather_rows_ref(X, dst, b, R.counts(dst, V) if mean else None)
            _compare(got.cpu(), ref64, ref32, dtype, what, worst)
            if not mean and b is None:
                assert torch.equal(got.cpu(), X[dst]), what
            if amax is not None:
                assert amax.item() == got.abs().max().item(), what
    if dtype == F32:
        print(f"gather rows h={h}: err32 {worst[0]:.3e} kernel {worst[1]:.3e}")


def test_grid_stride():
    """70 001 rows of 31 pieces: more lanes than the grids hold (256 * 32 blocks of 256).  rev swaps
    neighbours (the odd last row reverses into itself), dst cycles over 1000 nodes.
    Measured on an MI355X: err32 6.05e-8, kernel 6.05e-8 (worst of the two kernels)."""
    K = _K()
    n, h, V = 70_001, 124, 1000
    rev = torch.arange(n) ^ 1
    rev[-1] = n - 1
    dst = torch.arange(n) % V
    H, G, dA, dS = _rand(n, h, F32, 1, 3.0), _rand(n, h, F32, 2), _rand(n, h, F32, 3), _rand(V, h, F32, 4)
    dst_ptr, _, rev_ptr, rev_perm = _device_csrs(dst, rev, V, n)
    worst = [0.0, 0.0]
    got = K.dmpnn_edge_backward(G.to(DEV), H.to(DEV), dA.to(DEV), dS.to(DEV), dst.to(DEV), rev_ptr, rev_perm,
                                dst_ptr, act=_code("ReLU"), reduce="mean").cpu()
    _compare(got, R.edge_backward_ref(G, H, dA, dS, dst, rev, R.ACTS["ReLU"], "mean"),
             R.edge_backward_ref(G, H, dA, dS, dst, rev, R.ACTS["ReLU"], "mean", dtype=F32), F32, "edge backward", worst)
    got = K.gather_rows(dS.to(DEV), dst.to(DEV), base=G.to(DEV), seg_ptr=dst_ptr).cpu()
    _compare(got, R.gather_rows_ref(dS, dst, G, R.counts(dst, V)),
             R.gather_rows_ref(dS, dst, G, R.counts(dst, V, F32), dtype=F32), F32, "gather rows", worst)
    assert torch.equal(K.gather_rows(dS.to(DEV), dst.to(DEV)).cpu(), dS[dst])
    print(f"grid stride: err32 {worst[0]:.3e} kernel {worst[1]:.3e}")


# ------------------------------------------------------------------ 6. the max / min arg kernels
def _ref_arg(Y, idx, nseg, reduce):
    seg_ptr, perm = R.csr(idx, nseg)
    return R.segment_arg_ref(Y, seg_ptr, perm, reduce)


@COLLATES
@DTYPES
@pytest.mark.parametrize("h", [13, 16, 64])
def test_edge_backward_arg(h, dtype, collate):
    """dS[dst e] reaches row e only where arg[dst e] == e; arg from the loop reference (not from
    nt_segment_arg).  Max / min x ReLU / Identity / SiLU x residual on / off; fp32 amax exact.
    Measured on an MI355X (fp32, worst over the 12 combinations, per h and collate): err32 1.7e-7 ..
    4.1e-7, kernel the same figures to three digits."""
    K = _K()
    src, dst, rev, V, E = _graph(collate)
    H = _hidden(E, h, dtype, h)
    G, dA, dS = _rand(E, h, dtype, h + 1), _rand(E, h, dtype, h + 2), _rand(V, h, dtype, h + 3)
    _, _, rev_ptr, rev_perm = _device_csrs(dst, rev, V, E)
    Gd, Hd, dAd, dSd, dstd = (t.to(DEV) for t in (G, H, dA, dS, dst))
    worst = [0.0, 0.0]
    for act in ("ReLU", "Identity", "SiLU"):
        for reduce in ("max", "min"):
            arg = _ref_arg(R.ACTS[act](H.double()), dst, V, reduce)
            assert (arg[V - 2] == -1).all() and (arg[V - 1] == E - 1).all()
            for residual in (True, False):
                amax = torch.zeros(1, device=DEV) if dtype == F32 else None
                got = K.dmpnn_edge_backward_arg(Gd if residual else None, Hd, dAd, dSd, arg.to(DEV), dstd, rev_ptr,
                                                rev_perm, residual=residual, act=_code(act), amax=amax)
                what = f"edge backward arg {act} {reduce} residual={residual} h={h}"
                g = G if residual else None
                ref32 = R.edge_backward_arg_ref(None if g is None else g.float(), H.float(), dA.float(), dS.float(),
                                                arg, dst, rev, R.ACTS[act], dtype=F32)
                ref64 = R.edge_backward_arg_ref(g, H, dA, dS, arg, dst, rev, R.ACTS[act])
                _compare(got.cpu(), ref64, ref32, dtype, what, worst)
                if amax is not None:
                    assert amax.item() == got.abs().max().item(), what
    if dtype == F32:
        print(f"edge backward arg h={h} {collate}: err32 {worst[0]:.3e} kernel {worst[1]:.3e}")


@DTYPES
@pytest.mark.parametrize("h", [13, 16, 64])
def test_gather_rows_arg(h, dtype):
    """out[i] = (base[i] or 0) + (arg[dst i] == i ? X[dst i] : 0).  Without base the gradient is
    conserved: the rows of a segment sum to X[s] exactly (one non-zero term per column), 0 for an
    empty segment.  fp32 amax exact.  (An exact selection and at most one addition: err32 and the
    kernel's error were both 0 without base and equal with it on an MI355X.)"""
    K = _K()
    src, dst, rev, V, E = _graph("nodes")
    X, base, Hsel = _rand(V, h, dtype, h), _rand(E, h, dtype, h + 1), _rand(E, h, F32, h + 2).round()
    worst = [0.0, 0.0]
    for reduce in ("max", "min"):
        arg = _ref_arg(Hsel, dst, V, reduce)  # rounded values: ties, so the first row matters
        for b in (base, None):
            amax = torch.zeros(1, device=DEV) if dtype == F32 else None
            got = K.gather_rows_arg(X.to(DEV), dst.to(DEV), arg.to(DEV), base=None if b is None else b.to(DEV),
                                    amax=amax)
            what = f"gather rows arg {reduce} base={b is not None} h={h}"
            ref32 = R.gather_rows_arg_ref(X.float(), dst, arg, None if b is None else b.float(), dtype=F32)
            _compare(got.cpu(), R.gather_rows_arg_ref(X, dst, arg, b), ref32, dtype, what, worst)
            if amax is not None:
                assert amax.item() == got.abs().max().item(), what
            if b is None:
                assert torch.equal(got.cpu(), ref32.to(dtype)), what
                total = torch.zeros(V, h).index_add_(0, dst, got.cpu().float())
                live = arg[:, 0] >= 0
                assert torch.equal(total[live], X.float()[live]) and (total[~live] == 0).all(), what
                assert not live[V - 2] and live[V - 1]


@pytest.mark.parametrize("reduce", ["max", "min"])
def test_arg_unaligned(reduce):
    """h = 16 with arg one int into its buffer (data_ptr % 16 == 4): the scalar instances, same bits."""
    K = _K()
    h = 16
    src, dst, rev, V, E = _graph("nodes")
    H = _hidden(E, h, F32, 5)
    G, dA, dS = _rand(E, h, F32, 6), _rand(E, h, F32, 7), _rand(V, h, F32, 8)
    _, _, rev_ptr, rev_perm = _device_csrs(dst, rev, V, E)
    arg = _ref_arg(torch.relu(H.double()), dst, V, reduce).to(DEV)
    arg_u = torch.empty(arg.numel() + 4, dtype=torch.int32, device=DEV)[1:1 + arg.numel()].view(V, h).copy_(arg)
    assert arg.data_ptr() % 16 == 0 and arg_u.data_ptr() % 16 == 4
    Gd, Hd, dAd, dSd, dstd = (t.to(DEV) for t in (G, H, dA, dS, dst))
    a = K.dmpnn_edge_backward_arg(Gd, Hd, dAd, dSd, arg, dstd, rev_ptr, rev_perm)
    b = K.dmpnn_edge_backward_arg(Gd, Hd, dAd, dSd, arg_u, dstd, rev_ptr, rev_perm)
    assert torch.equal(a, b)
    a = K.gather_rows_arg(dSd, dstd, arg, base=Gd)
    b = K.gather_rows_arg(dSd, dstd, arg_u, base=Gd)
    assert torch.equal(a, b)


# ------------------------------------------------------------------ 7. wrapper checks
class _NoLibrary:
    def __getattr__(self, name):
        def entry(*args, **kwargs):
            raise AssertionError("reached the library")

        return entry


@pytest.fixture
def no_library(monkeypatch):
    """Every entry point raises: a missing check cannot become a launch with a bad pointer."""
    from notorch_amd import _lib

    monkeypatch.setattr(_lib, "load", lambda: _NoLibrary())


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _strided(t):
    """t's values in a non-contiguous view."""
    buf = torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)
    buf[::2] = t.flatten()
    return buf[::2].view(t.shape) if t.dim() == 1 else torch.stack([t, t], -1)[..., 0]


def _reduce_args():
    return dict(X=torch.zeros(6, 8, device=DEV), seg_ptr=_i32(0, 2, 2, 6), perm=_i32(*range(6)), nseg=3)


def _bad_csr(good):
    return [
        ("seg_ptr", good["seg_ptr"].long(), TypeError),
        ("seg_ptr", _i32(0, 2, 6), ValueError),
        ("seg_ptr", _strided(good["seg_ptr"]), ValueError),
        ("perm", good["perm"].long(), TypeError),
        ("perm", _i32(*range(5)), ValueError),
        ("perm", _strided(good["perm"]), ValueError),
    ]


def _expect(fn, good, name, value, exc):
    kwargs = dict(good)
    kwargs[name] = value
    with pytest.raises(exc):
        fn(**kwargs)


def test_segment_reduce_rejects(no_library):
    K = _K()
    good = dict(_reduce_args(), out=torch.zeros(3, 8, device=DEV))
    with pytest.raises(AssertionError, match="reached the library"):
        K.segment_reduce(**good)
    for name, value, exc in _bad_csr(good) + [("out", torch.zeros(4, 8, device=DEV), ValueError),
                                              ("out", torch.zeros(3, 4, device=DEV), ValueError),
                                              ("out", torch.zeros(3, 8, device=DEV, dtype=BF16), TypeError)]:
        _expect(K.segment_reduce, good, name, value, exc)


def test_segment_arg_rejects(no_library):
    K = _K()
    good = dict(_reduce_args(), reduce="max")
    with pytest.raises(AssertionError, match="reached the library"):
        K.segment_arg(**good)
    for name, value, exc in _bad_csr(good):
        _expect(K.segment_arg, good, name, value, exc)


def test_gather_rows_arg_rejects(no_library):
    K = _K()
    good = dict(X=torch.zeros(3, 8, device=DEV), idx=torch.zeros(6, dtype=torch.int64, device=DEV),
                arg=torch.zeros(3, 8, dtype=torch.int32, device=DEV), base=torch.zeros(6, 8, device=DEV))
    with pytest.raises(AssertionError, match="reached the library"):
        K.gather_rows_arg(**good)
    for name, value, exc in [
        ("idx", good["idx"].int(), TypeError),
        ("idx", _strided(good["idx"]), ValueError),
        ("arg", good["arg"].long(), TypeError),
        ("arg", good["arg"][:, :4].contiguous(), ValueError),
        ("arg", good["arg"][:2].contiguous(), ValueError),
        ("arg", _strided(good["arg"]), ValueError),
        ("base", torch.zeros(5, 8, device=DEV), ValueError),
    ]:
        _expect(K.gather_rows_arg, good, name, value, exc)


def test_edge_backward_arg_rejects(no_library):
    K = _K()
    z = lambda *s: torch.zeros(*s, device=DEV)
    good = dict(G=z(6, 8), H=z(6, 8), dA=z(6, 8), dS=z(3, 8), arg=torch.zeros(3, 8, dtype=torch.int32, device=DEV),
                dst=torch.zeros(6, dtype=torch.int64, device=DEV), rev_ptr=_i32(*range(7)), rev_perm=_i32(*range(6)))
    with pytest.raises(AssertionError, match="reached the library"):
        K.dmpnn_edge_backward_arg(**good)
    for name, value, exc in [
        ("arg", good["arg"].long(), TypeError),
        ("arg", good["arg"][:, :4].contiguous(), ValueError),
        ("arg", torch.zeros(6, 8, dtype=torch.int32, device=DEV), ValueError),
        ("arg", _strided(good["arg"]), ValueError),
        ("dst", good["dst"].int(), TypeError),
        ("dst", good["dst"][:5].contiguous(), ValueError),
        ("dst", _strided(good["dst"]), ValueError),
        ("rev_ptr", good["rev_ptr"].long(), TypeError),
        ("rev_ptr", _i32(*range(6)), ValueError),
        ("rev_ptr", _strided(good["rev_ptr"]), ValueError),
        ("rev_perm", good["rev_perm"].long(), TypeError),
        ("rev_perm", _i32(*range(5)), ValueError),
        ("rev_perm", _strided(good["rev_perm"]), ValueError),
    ]:
        _expect(K.dmpnn_edge_backward_arg, good, name, value, exc)


def test_amax_is_fp32_only(no_library):
    """bf16 kernels write no amax: asking for one is an error, not a silent zero."""
    K = _K()
    z = lambda *s: torch.zeros(*s, device=DEV, dtype=BF16)
    amax = torch.zeros(1, device=DEV)
    seg_ptr = _i32(0, 2, 2, 6)
    with pytest.raises(ValueError, match="amax is fp32 only"):
        K.dmpnn_edge_backward(z(6, 8), z(6, 8), z(6, 8), z(3, 8), torch.zeros(6, dtype=torch.int64, device=DEV),
                              _i32(*range(7)), _i32(*range(6)), None, amax=amax)
    with pytest.raises(ValueError, match="amax is fp32 only"):
        K.gather_rows(z(3, 8), torch.zeros(6, dtype=torch.int64, device=DEV), amax=amax)
    with pytest.raises(ValueError, match="amax is fp32 only"):
        K.segment_reduce_chunked(z(6, 8), seg_ptr, _i32(*range(6)), 3, K.chunk_plan(seg_ptr), amax=amax)
    with pytest.raises(ValueError, match="amax is fp32 only"):
        K.gather_rows_arg(z(3, 8), torch.zeros(6, dtype=torch.int64, device=DEV),
                          torch.zeros(3, 8, dtype=torch.int32, device=DEV), amax=amax)
    with pytest.raises(ValueError, match="amax is fp32 only"):
        K.dmpnn_edge_backward_arg(z(6, 8), z(6, 8), z(6, 8), z(3, 8), torch.zeros(3, 8, dtype=torch.int32, device=DEV),
                                  torch.zeros(6, dtype=torch.int64, device=DEV), _i32(*range(7)), _i32(*range(6)),
                                  amax=amax)
