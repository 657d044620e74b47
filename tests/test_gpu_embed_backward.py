"""GPU: the embedding tables train on the kernel path.

* nt_embed_bag_backward (csrc/embed_backward.hip) against fp64 ``index_add_`` on the CPU: the LDS
  instances, the chunked path for tables past the LDS partial, every k, empties, the CSR form (the
  node table's: R[i] = sum of dX over segment i), padded row pitch, bit-equal repeat calls.
  Tolerance: the fp32 contract of tests/test_gpu_backward.py (normalised max error <= GRAD_TOL, or 4 x
  the fp32 CPU evaluation's own distance from fp64 where long sums put the fp32 floor above that);
  bf16 output: one bf16 rounding of the fp32 sum (2^-8 normalised).
* EmbeddedChempropBlock / GraphEmbedding under autograd: gradients of both tables and every layer
  parameter against fp64 autograd of the torch restatement (oracle/dmpnn_ref.py) with the embedding as
  ``T[idx].sum(1)``; forward bits equal to the no-grad fused forward; dW / db bits equal to the unfused
  pair's; no library embedding op and no torch recompute on the way.
"""
import pytest
import torch
import torch.nn as nn

from helpers import assert_parity, norm_err
from oracle import dmpnn_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
GRAD_TOL = 1e-5
BF16 = torch.bfloat16
BF16_ULP = 2.0 ** -8


# ------------------------------------------------------------------------------------ the kernel
def _reference(dX, idx, ntypes, seg_ptr=None, perm=None, dtype=torch.float64):
    """dT by index_add_ on the CPU in ``dtype`` (fp64: the truth; fp32: the floor guard)."""
    X = dX.detach().cpu().to(dtype)
    if seg_ptr is not None:
        sp, pm = seg_ptr.cpu().long(), perm.cpu().long()
        seg = torch.repeat_interleave(torch.arange(sp.numel() - 1), sp[1:] - sp[:-1])
        X = torch.zeros(sp.numel() - 1, X.shape[1], dtype=dtype).index_add_(0, seg, X[pm])
    idx = idx.cpu()
    out = torch.zeros(ntypes, X.shape[1], dtype=dtype)
    for j in range(idx.shape[1]):
        out.index_add_(0, idx[:, j], X)
    return out


def _check_kernel(dX, idx, ntypes, seg_ptr=None, perm=None, out_dtype=None):
    from notorch_amd import kernels as K

    got = K.embed_bag_backward(dX, idx, ntypes, seg_ptr, perm, out_dtype=out_dtype)
    assert got.shape == (ntypes, dX.shape[1]) and got.dtype == (out_dtype or dX.dtype)
    truth = _reference(dX, idx, ntypes, seg_ptr, perm)
    if got.dtype == BF16:
        tol = BF16_ULP
    else:
        tol = max(GRAD_TOL, 4 * norm_err(_reference(dX, idx, ntypes, seg_ptr, perm, torch.float32), truth))
    err = norm_err(got.float(), truth)
    print(f"embed_bag_backward n={idx.shape[0]} k={idx.shape[1]} h={dX.shape[1]} T={ntypes} "
          f"{dX.dtype}->{got.dtype}: normalised max error {err:.3e} (tol {tol:.1e})")
    assert err <= tol
    unused = torch.ones(ntypes, dtype=torch.bool)
    unused[idx.cpu().flatten()] = False
    assert (got[unused.to(DEV)] == 0).all()  # a type no row uses: exact zeros
    return got


GRID = [(1, 1, 2, 1), (65, 2, 13, 13), (257, 7, 300, 42), (1000, 7, 512, 42), (3000, 2, 64, 1000)]


@pytest.mark.parametrize("n,k,h,ntypes", GRID)
def test_kernel_grid_fp32(n, k, h, ntypes):
    g = torch.Generator().manual_seed(n + h)
    dX = torch.randn(n, h, generator=g).to(DEV)
    idx = torch.randint(0, ntypes, (n, k), generator=g).to(DEV)
    _check_kernel(dX, idx, ntypes)


@pytest.mark.parametrize("n,k,h,ntypes", [c for c in GRID if c[2] in (64, 512)])
@pytest.mark.parametrize("out_dtype", [BF16, torch.float32])
def test_kernel_grid_bf16(n, k, h, ntypes, out_dtype):
    g = torch.Generator().manual_seed(n + h)
    dX = torch.randn(n, h, generator=g).to(BF16).to(DEV)
    idx = torch.randint(0, ntypes, (n, k), generator=g).to(DEV)
    _check_kernel(dX, idx, ntypes, out_dtype=out_dtype)


def _contention(n=1000, k=7, h=512, ntypes=42):
    g = torch.Generator().manual_seed(5)
    return torch.randn(n, h, generator=g).to(DEV), torch.full((n, k), 3, dtype=torch.int64, device=DEV)


def test_kernel_contention_and_empties():
    from notorch_amd import kernels as K

    dX, idx = _contention()  # every index the same type: one row takes all n * k adds, 41 stay zero
    got = _check_kernel(dX, idx, 42)
    assert got[3].abs().max() > 0 and got.abs().sum(1).count_nonzero() == 1
    g = torch.Generator().manual_seed(6)
    # one type never used
    idx = torch.randint(0, 12, (300, 7), generator=g)
    idx[idx >= 5] += 1
    _check_kernel(torch.randn(300, 40, generator=g).to(DEV), idx.to(DEV), 13)
    # fewer rows than launched workgroups (3 chunks of a 1000-type table over one row range)
    _check_kernel(torch.randn(2, 64, generator=g).to(DEV), torch.tensor([[0, 999], [500, 500]], device=DEV), 1000)
    # n = 0: zeros
    out = K.embed_bag_backward(torch.empty(0, 24, device=DEV), torch.empty(0, 7, dtype=torch.int64, device=DEV), 9)
    assert out.shape == (9, 24) and (out == 0).all()
    # an index out of range contributes nothing and writes nowhere else
    dX = torch.randn(10, 8, generator=g).to(DEV)
    idx = torch.randint(0, 4, (10, 2), generator=g)
    ok = K.embed_bag_backward(dX, idx.to(DEV), 4)
    bad = torch.cat([idx, torch.tensor([[4, -1]] * 10)], 1)
    assert torch.equal(K.embed_bag_backward(dX, bad.to(DEV), 4), ok)


@pytest.mark.parametrize("dtype,h", [(torch.float32, 300), (torch.float32, 13), (BF16, 64)])
def test_kernel_with_csr(dtype, h):
    """Segments of length 0, 1..4 and one hub of 200 rows, perm a real permutation, dX row-padded."""
    from notorch_amd import kernels as K
    from notorch_amd.nn.gnn import _engine

    g = torch.Generator().manual_seed(7)
    lens = torch.randint(0, 5, (150,), generator=g)
    lens[0], lens[17], lens[149] = 0, 200, 0
    n, n_dx = lens.numel(), int(lens.sum())
    seg_of_row = torch.repeat_interleave(torch.arange(n), lens)[torch.randperm(n_dx, generator=g)]
    seg_ptr, perm = K.csr_build(seg_of_row.to(DEV), n)
    assert not torch.equal(perm.cpu().long(), torch.arange(n_dx))
    idx = torch.randint(0, 42, (n, 7), generator=g).to(DEV)
    X = torch.randn(n_dx, h, generator=g).to(dtype)
    _check_kernel(X.to(DEV), idx, 42, seg_ptr, perm)
    if dtype == torch.float32 and h == 300:
        pitch = _engine.row_pitch(300, torch.float32)
        assert pitch is not None and pitch > h
        Xp = K.padded_rows(n_dx, h, pitch, torch.float32, DEV)
        Xp.copy_(X)
        assert Xp.stride(0) == pitch
        a = K.embed_bag_backward(Xp, idx, 42, seg_ptr, perm)
        assert torch.equal(a, K.embed_bag_backward(X.to(DEV), idx, 42, seg_ptr, perm))
        assert torch.equal(K.embed_bag_backward(Xp, idx, 42, seg_ptr, perm, pitch=pitch), a)
    # all segments empty
    empty_ptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    out = K.embed_bag_backward(torch.empty(0, h, dtype=dtype, device=DEV), idx, 42, empty_ptr,
                               torch.empty(0, dtype=torch.int32, device=DEV))
    assert (out == 0).all()


def test_kernel_is_deterministic():
    from notorch_amd import kernels as K

    dX, idx = _contention()
    assert torch.equal(K.embed_bag_backward(dX, idx, 42), K.embed_bag_backward(dX, idx, 42))
    g = torch.Generator().manual_seed(8)
    dX = torch.randn(1000, 512, generator=g).to(DEV)
    idx = torch.randint(0, 42, (1000, 7), generator=g).to(DEV)
    assert torch.equal(K.embed_bag_backward(dX, idx, 42), K.embed_bag_backward(dX, idx, 42))


def test_kernel_binding_rejects_bad_arguments():
    from notorch_amd import kernels as K

    dX = torch.zeros(4, 8, device=DEV)
    idx = torch.zeros(4, 2, dtype=torch.int64, device=DEV)
    with pytest.raises(TypeError):
        K.embed_bag_backward(dX, idx.int(), 3)
    with pytest.raises(TypeError):
        K.embed_bag_backward(dX.double(), idx, 3)
    with pytest.raises(ValueError):
        K.embed_bag_backward(dX[:3], idx, 3)  # no CSR: one row of dX per row of idx
    with pytest.raises(ValueError):
        K.embed_bag_backward(dX.t(), idx, 3)
    with pytest.raises(ValueError):
        K.embed_bag_backward(dX, idx, 3, seg_ptr=torch.zeros(5, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------------------------ the modules
def _graph(kind="qm9", n=32, seed=0):
    from notorch_amd.data.synth import make_batch

    return make_batch(kind, n, seed=seed).collate("nodes")


def _modules(h, depth, dtype=torch.float32, fuse=True, **opts):
    from notorch_amd.nn import ChempropBlock, EmbeddedChempropBlock, GraphEmbedding

    torch.manual_seed(3)
    emb = GraphEmbedding(42, 13, h)
    blk = ChempropBlock(hidden_dim=h, depth=depth, **opts)
    return emb, blk, EmbeddedChempropBlock(emb, blk, fuse=fuse).to(dtype).to(DEV).train()


def _params(enc):
    layers = enc.block._chemprop_layers()
    return ([enc.embedding.node.weight, enc.embedding.edge.weight] + [l.linear.weight for l in layers]
            + [l.linear.bias for l in layers])


def _names(depth):
    return ["dTv", "dTe"] + [f"dW[{l}]" for l in range(depth)] + [f"db[{l}]" for l in range(depth)]


def _step(enc, Gd):
    """One training step's forward + backward: (node, edge, grads)."""
    from notorch_amd.nn import Sum

    for p in enc.parameters():
        p.grad = None
    out = enc(Gd)
    Sum()(out).float().pow(2).sum().backward()
    return out.node_feats.detach(), out.edge_feats.detach(), [p.grad for p in _params(enc)]


def _truth(G, enc, masks=None):
    """fp64 autograd of the torch restatement on the CPU, the tables as leaves."""
    blk = enc.block
    ps = [p.detach().double().cpu().requires_grad_(True) for p in _params(enc)]
    d = blk.depth
    Tv, Te, Ws, bs = ps[0], ps[1], ps[2:2 + d], ps[2 + d:]
    Xv, Xe = Tv[G.node_feats].sum(1), Te[G.edge_feats].sum(1)
    n, _ = dmpnn_ref.chemprop_block(Xv, Xe, G.edge_index, G.rev_index, Ws, bs, residual=blk.residual,
                                    reduce=blk.reduce, dropout_masks=masks)
    dmpnn_ref.readout(n, G.batch_node_index, len(G), "sum").pow(2).sum().backward()
    return [p.grad for p in ps]


@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("h", [32, 300])
def test_embedded_block_grads(h, reduce, residual):
    G, Gd = _graph("qm9", 32, seed=h), _graph("qm9", 32, seed=h).to(DEV)  # to() moves a batch in place
    emb, blk, enc = _modules(h, 2, reduce=reduce, residual=residual)
    node, edge, got = _step(enc, Gd)
    truth = _truth(G, enc)
    for name, a, t in zip(_names(2), got, truth):
        assert a is not None, name
        print(f"h={h} {reduce} residual={residual} {name}: {norm_err(a, t):.3e}")
        assert_parity(a, t, GRAD_TOL, name)
    # the forward under autograd has the bits of the no-grad fused forward
    with torch.no_grad():
        ref = enc(Gd)
    assert torch.equal(node, ref.node_feats) and torch.equal(edge, ref.edge_feats)
    # dW / db have the bits of the unfused pair's (the same kernels on the same inputs)
    enc.fuse = False
    node_u, edge_u, unfused = _step(enc, Gd)
    assert torch.equal(node_u, node) and torch.equal(edge_u, edge)
    for name, a, b in list(zip(_names(2), got, unfused))[2:]:
        assert torch.equal(a, b), name
    for name, a, t in list(zip(_names(2), unfused, truth))[:2]:
        assert_parity(a, t, GRAD_TOL, name + " (EmbedBagFunction)")


def test_embedded_block_depth0():
    G = _graph("qm9", 32, seed=1)
    emb, blk, enc = _modules(48, 0)
    _, _, got = _step(enc, _graph("qm9", 32, seed=1).to(DEV))
    for name, a, t in zip(_names(0), got, _truth(G, enc)):
        assert_parity(a, t, GRAD_TOL, name)


def test_training_runs_on_the_kernel_path(monkeypatch):
    """Neither the library's embedding_bag nor the torch recompute of the block is touched by a training
    step of the embedded encoder or of a standalone GraphEmbedding."""
    from notorch_amd.nn.gnn import _engine

    def boom(*a, **k):
        raise AssertionError("the embedded encoder must train on the kernel path")

    monkeypatch.setattr(torch.nn.functional, "embedding_bag", boom)
    monkeypatch.setattr(_engine, "_torch_block", boom)
    calls = []
    real = _engine.K.embed_bag_backward
    monkeypatch.setattr(_engine.K, "embed_bag_backward", lambda *a, **k: calls.append(1) or real(*a, **k))
    G, Gd = _graph("qm9", 32, seed=2), _graph("qm9", 32, seed=2).to(DEV)  # to() moves a batch in place
    emb, blk, enc = _modules(64, 2)
    _, _, got = _step(enc, Gd)
    assert len(calls) == 2 and all(g is not None and g.abs().sum() > 0 for g in got)
    del calls[:]
    for p in emb.parameters():
        p.grad = None
    out = emb(Gd)
    (out.node_feats.pow(2).sum() + out.edge_feats.sum()).backward()
    assert len(calls) == 2
    Tv = emb.node.weight.detach().double().cpu().requires_grad_(True)
    Te = emb.edge.weight.detach().double().cpu().requires_grad_(True)
    (Tv[G.node_feats].sum(1).pow(2).sum() + Te[G.edge_feats].sum(1).sum()).backward()
    assert_parity(emb.node.weight.grad, Tv.grad, GRAD_TOL, "standalone dTv")
    assert_parity(emb.edge.weight.grad, Te.grad, GRAD_TOL, "standalone dTe")


@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_embedded_block_dropout(reduce):
    """Active dropout on the fused training path: the unfused path's masks for the same manual_seed."""
    from notorch_amd import kernels as K
    from notorch_amd.nn.gnn import _engine

    G, Gd = _graph("qm9", 32, seed=4), _graph("qm9", 32, seed=4).to(DEV)  # to() moves a batch in place
    h, depth, p = 48, 2, 0.25
    emb, blk, enc = _modules(h, depth, dropout=p, reduce=reduce)
    torch.manual_seed(11)
    node, edge, got = _step(enc, Gd)
    enc.fuse = False
    torch.manual_seed(11)
    node_u, edge_u, unfused = _step(enc, Gd)
    assert torch.equal(node, node_u) and torch.equal(edge, edge_u)
    with torch.no_grad():
        assert not torch.equal(enc.eval()(Gd).edge_feats, edge)  # the masks were applied
    enc.train()
    torch.manual_seed(11)
    seed = _engine.draw_dropout_seed()
    ones = torch.ones(G.num_edges, h, device=DEV)
    masks = [K.dropout_residual(ones, p, seed, _engine.dropout_offset(l, G.num_edges, h)).double().cpu()
             for l in range(depth)]
    truth = _truth(G, enc, masks)
    for name, a, b, t in zip(_names(depth), got, unfused, truth):
        assert_parity(a, t, GRAD_TOL, name)
        assert_parity(b, t, GRAD_TOL, name + " (unfused)")


def test_frozen_node_table(monkeypatch):
    from notorch_amd.nn.gnn import _engine

    calls = []
    real = _engine.K.embed_bag_backward
    monkeypatch.setattr(_engine.K, "embed_bag_backward", lambda *a, **k: calls.append(1) or real(*a, **k))
    G = _graph("qm9", 32, seed=5)
    emb, blk, enc = _modules(32, 2)
    emb.node.weight.requires_grad_(False)
    _, _, got = _step(enc, _graph("qm9", 32, seed=5).to(DEV))
    assert emb.node.weight.grad is None and len(calls) == 1  # nothing launched for the frozen table
    truth = _truth(G, enc)
    for name, a, t in list(zip(_names(2), got, truth))[1:]:
        assert_parity(a, t, GRAD_TOL, name)


def test_nt_bwd_torch_still_trains(monkeypatch):
    G, Gd = _graph("qm9", 32, seed=6), _graph("qm9", 32, seed=6).to(DEV)  # to() moves a batch in place
    emb, blk, enc = _modules(32, 2)
    _, _, kernel = _step(enc, Gd)
    monkeypatch.setenv("NT_BWD", "torch")
    _, _, lib = _step(enc, Gd)
    for name, a, b, t in zip(_names(2), lib, kernel, _truth(G, enc)):
        assert_parity(a, t, GRAD_TOL, name + " (NT_BWD=torch)")
        assert_parity(a, b, GRAD_TOL, name + " (NT_BWD=torch vs kernel)")


def test_embedded_block_grads_bf16(monkeypatch):
    """The README's bf16 contract for the table gradients: no further from fp64 (on the same bf16-valued
    parameters) than 2 x torch's own bf16 evaluation, nn.EmbeddingBag's backward on the device
    (NT_EMBED_BWD=torch: the library path of the same encoder)."""
    G, Gd = _graph("zinc", 64, seed=7), _graph("zinc", 64, seed=7).to(DEV)  # to() moves a batch in place
    emb, blk, enc = _modules(128, 2, BF16)
    truth = _truth(G, enc)
    node, edge, got = _step(enc, Gd)
    with torch.no_grad():
        ref = enc(Gd)
    assert torch.equal(node, ref.node_feats) and torch.equal(edge, ref.edge_feats)
    monkeypatch.setenv("NT_EMBED_BWD", "torch")
    _, _, lib = _step(enc, Gd)
    for name, a, r, t in list(zip(_names(2), got, lib, truth))[:2]:
        assert a.dtype == BF16 and torch.isfinite(a.float()).all(), name
        e, e_lib = norm_err(a.float(), t), norm_err(r.float(), t)
        print(f"bf16 {name}: kernel {e:.3e} | nn.EmbeddingBag bf16 {e_lib:.3e}")
        assert e <= 2 * e_lib, f"{name}: {e:.3e} vs torch bf16 {e_lib:.3e}"
