"""The CPU references of tests/segment_ref.py against torch's own scatter / functional ops, on random
inputs (no ties), so a wrong reference cannot pass a wrong kernel.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import segment_ref as R

COUNTS = [0, 1, 3, 4, 5, 8, 9, 0, 37, 2]


def _case(shuffle, h=7, seed=0):
    idx = R.index_from_counts(COUNTS * 3, shuffle_seed=5 if shuffle else None)
    X = torch.randn(len(idx), h, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    seg_ptr, perm = R.csr(idx, len(COUNTS) * 3)
    return idx, X, seg_ptr, perm


@pytest.mark.parametrize("shuffle", [False, True])
def test_csr_is_stable(shuffle):
    idx, _, seg_ptr, perm = _case(shuffle)
    assert torch.equal(seg_ptr[1:] - seg_ptr[:-1], torch.tensor(COUNTS * 3))
    assert torch.equal(idx[perm], torch.sort(idx).values)
    for s in range(len(seg_ptr) - 1):  # rows of a segment ascend
        rows = perm[seg_ptr[s]:seg_ptr[s + 1]]
        assert torch.equal(rows, torch.sort(rows).values)
    if not shuffle:
        assert torch.equal(perm, torch.arange(len(idx)))


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("reduce,torch_reduce", [("sum", "sum"), ("mean", "mean"), ("max", "amax"), ("min", "amin")])
@pytest.mark.parametrize("act", ["Identity", "ReLU", "SiLU"])
def test_segment_reduce_ref(shuffle, reduce, torch_reduce, act):
    idx, X, seg_ptr, perm = _case(shuffle)
    got = R.segment_reduce_ref(X, seg_ptr, None if not shuffle else perm, reduce, R.ACTS[act])
    nseg = len(seg_ptr) - 1
    want = torch.zeros(nseg, X.shape[1], dtype=torch.float64).scatter_reduce(
        0, idx[:, None].expand_as(X), R.ACTS[act](X), torch_reduce, include_self=False)
    assert torch.allclose(got, want, rtol=1e-13, atol=1e-13)
    empty = torch.tensor(COUNTS * 3) == 0
    assert (got[empty] == 0).all()


def test_segment_reduce_ref_fp32_is_sequential():
    """fp32: the accumulation order is ascending CSR position (a hand loop agrees bit for bit)."""
    idx, X, seg_ptr, perm = _case(True)
    X = X.float()
    got = R.segment_reduce_ref(X, seg_ptr, perm, "sum", dtype=torch.float32)
    for s in (2, 8, 18):
        acc = torch.zeros(X.shape[1])
        for j in range(seg_ptr[s], seg_ptr[s + 1]):
            acc = acc + X[perm[j]]
        assert torch.equal(got[s], acc)


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("reduce", ["max", "min"])
def test_segment_arg_ref(shuffle, reduce):
    idx, X, seg_ptr, perm = _case(shuffle)
    arg = R.segment_arg_ref(X, seg_ptr, None if not shuffle else perm, reduce)
    val = R.segment_reduce_ref(X, seg_ptr, None if not shuffle else perm, reduce)
    for s in range(len(seg_ptr) - 1):
        if seg_ptr[s] == seg_ptr[s + 1]:
            assert (arg[s] == -1).all()
            continue
        assert (idx[arg[s].long()] == s).all()
        assert torch.equal(X.gather(0, arg[s].long()[None])[0], val[s])


def test_segment_arg_ref_first_row_wins_ties():
    Y = torch.tensor([[1.0, 0.0], [1.0, -0.0], [0.0, 0.0], [1.0, 5.0]])
    seg_ptr = torch.tensor([0, 0, 4])
    perm = torch.tensor([2, 1, 0, 3])  # CSR order: rows 2, 1, 0, 3
    assert R.segment_arg_ref(Y, seg_ptr, perm, "max").tolist() == [[-1, -1], [1, 3]]
    assert R.segment_arg_ref(Y, seg_ptr, perm, "min").tolist() == [[-1, -1], [2, 2]]


@pytest.mark.parametrize("act,fn", [
    ("Identity", lambda x: torch.ones_like(x)),
    ("ReLU", lambda x: (x > 0).double()),
    ("LeakyReLU", lambda x: torch.where(x > 0, torch.ones_like(x), torch.full_like(x, 0.1))),
    ("ELU", lambda x: torch.where(x > 0, torch.ones_like(x), 1.3 * torch.exp(x))),
    ("GELU", lambda x: 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * torch.pi) ** 0.5),
    ("SiLU", lambda x: torch.sigmoid(x) * (1 + x * (1 - torch.sigmoid(x)))),
    ("Tanh", lambda x: 1 - torch.tanh(x) ** 2),
    ("Sigmoid", lambda x: torch.sigmoid(x) * (1 - torch.sigmoid(x))),
])
def test_act_grad_ref(act, fn):
    x = torch.randn(50, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 3
    assert torch.allclose(R.act_grad_ref(x, R.ACTS[act]), fn(x), rtol=1e-12, atol=1e-14)


def _edges(seed=0, E=40, V=9, h=5):
    g = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, V, (E,), generator=g), torch.randint(0, V - 1, (E,), generator=g)
    rev = torch.randint(0, E // 2, (E,), generator=g)  # not a permutation: rows get 0, 1, several
    t = lambda n: torch.randn(n, h, generator=g, dtype=torch.float64)
    return src, dst, rev, t(E), t(E), t(E), t(V), t(V)


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("residual", [True, False])
def test_edge_backward_ref_is_the_autograd_of_the_layer(reduce, residual):
    """One layer's message written with index ops, differentiated by autograd: dL/dH of
    L = <G, H> (residual) + <dA, A(H)> with A = S[src] - act(H)[rev], S = scatter(act(H), dst)."""
    src, dst, rev, G, H, dA, _, _ = _edges()
    V = 9
    Hx = H.clone().requires_grad_(True)
    M = F.silu(Hx)
    S = torch.zeros(V, H.shape[1], dtype=torch.float64).index_add_(0, dst, M)
    if reduce == "mean":
        S = S / R.counts(dst, V)[:, None]
    A = S[src] - M[rev]
    ((G * Hx).sum() * (1.0 if residual else 0.0) + (dA * A).sum()).backward()
    dS = torch.zeros(V, H.shape[1], dtype=torch.float64).index_add_(0, src, dA)
    got = R.edge_backward_ref(G if residual else None, H, dA, dS, dst, rev, R.ACTS["SiLU"], reduce)
    assert torch.allclose(got, Hx.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("reduce", ["max", "min"])
def test_edge_backward_arg_ref_is_the_autograd_of_the_layer(reduce):
    src, dst, rev, G, H, dA, _, _ = _edges(1)
    V = 9
    Hx = H.clone().requires_grad_(True)
    M = torch.tanh(Hx)
    S = torch.zeros(V, H.shape[1], dtype=torch.float64).scatter_reduce(
        0, dst[:, None].expand_as(M), M, "amax" if reduce == "max" else "amin", include_self=False)
    ((G * Hx).sum() + (dA * (S[src] - M[rev])).sum()).backward()
    dS = torch.zeros(V, H.shape[1], dtype=torch.float64).index_add_(0, src, dA)
    seg_ptr, perm = R.csr(dst, V)
    arg = R.segment_arg_ref(torch.tanh(H), seg_ptr, perm, reduce)
    got = R.edge_backward_arg_ref(G, H, dA, dS, arg, dst, rev, R.ACTS["Tanh"])
    assert torch.allclose(got, Hx.grad, rtol=1e-12, atol=1e-12)


def test_message_and_gather_refs():
    src, dst, rev, G, H, _, S, X = _edges(2)
    assert torch.equal(R.message_ref(H, S, src, rev, R.ACTS["ReLU"]), S[src] - torch.relu(H[rev]))
    V = 9
    Xx = X.clone().requires_grad_(True)
    node = torch.zeros(V, X.shape[1], dtype=torch.float64).index_add_(0, dst, H) / R.counts(dst, V)[:, None]
    # d<X, mean-scatter(H)>/dH = X[dst] / c
    got = R.gather_rows_ref(X, dst, base=G, mean_idx_counts=R.counts(dst, V))
    Hx = H.clone().requires_grad_(True)
    node = torch.zeros(V, X.shape[1], dtype=torch.float64).index_add_(0, dst, Hx) / R.counts(dst, V)[:, None]
    ((X * node).sum() + (G * Hx).sum()).backward()
    assert torch.allclose(got, Hx.grad, rtol=1e-12, atol=1e-12)
    assert torch.equal(R.gather_rows_ref(X, dst), X[dst])
    # max scatter: autograd routes to the arg
    Hx = H.clone().requires_grad_(True)
    node = torch.zeros(V, X.shape[1], dtype=torch.float64).scatter_reduce(
        0, dst[:, None].expand_as(Hx), Hx, "amax", include_self=False)
    (X * node).sum().backward()
    seg_ptr, perm = R.csr(dst, V)
    arg = R.segment_arg_ref(H, seg_ptr, perm, "max")
    assert torch.allclose(R.gather_rows_arg_ref(X, dst, arg), Hx.grad, rtol=0, atol=0)
    assert torch.equal(R.gather_rows_arg_ref(X, dst, arg, base=G), G + Hx.grad)
