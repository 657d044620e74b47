"""GPU parity of the bf16 layer kernel above hidden 512 (csrc/bf16.hip, update_bf16_wide_kernel: column
passes of 512 output columns x K chunks of 512 input columns on the 64-edge tile of the narrow kernel).

Criteria are those of tests/test_gpu_bf16.py and tests/test_gpu_bf16_backward.py:
* one launch / dense mode: normalised max error <= 2^-8 against the fp32 CPU product of the bf16-rounded
  operands (one final bf16 rounding, <= 2^-9 of the element, plus the fp32 accumulation order; neither
  grows with K to that level);
* fused launch: H_out bit-identical to the plain launch, S_out within 2^-8 of the segment reduce of it;
* block + readout: no further from fp64 truth than BF16_FACTOR x PyTorch's own bf16 evaluation of the
  restatement on the same device (normalised max and relative L2 error);
* training: every gradient no further from the fp64 oracle than BF16_FACTOR x the torch-op recompute
  (NT_BWD=torch), or than the floor BF16_FLOOR.
"""
import functools

import pytest
import torch
import torch.nn as nn

from helpers import assert_parity, norm_err
from oracle import dmpnn_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
ULP_TOL = 2.0 ** -8
WALK_TOL = 2e-2
BLOCK_TOL = 2e-2
BF16_FACTOR = 2.0
BF16_FLOOR = 2e-2


def _K():
    from notorch_amd import kernels

    return kernels


def _graph(kind="zinc", n=32, seed=0, rev_offset="nodes"):
    from notorch_amd.data.synth import make_batch

    return make_batch(kind, n, seed=seed).collate(rev_offset)


def _rand_bf16(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(BF)


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


_ACTS = {"relu": (nn.ReLU, torch.relu), "identity": (nn.Identity, lambda x: x),
         "silu": (nn.SiLU, torch.nn.functional.silu)}


# ------------------------------------------------------------------ one update launch
@functools.lru_cache(maxsize=None)
def _launch_case(h, n, act="relu"):
    """Inputs of one launch and the fp32 CPU product A W^T, computed once per (h, n, act)."""
    G = _graph("zinc", n, seed=3)  # n = 40: E is not a multiple of the 64-edge tile
    E, V = G.num_edges, G.num_nodes
    H, S = _rand_bf16(E, h, seed=4), _rand_bf16(V, h, seed=5)
    W = (_rand_bf16(h, h, seed=6).float() / h ** 0.5).to(BF)
    b = _rand_bf16(h, seed=7)
    src, rev = G.edge_index[0], G.rev_index
    # the message operand is rounded to bf16 before the MFMA (what a bf16 nn.Linear input holds)
    A = (S.float()[src] - _ACTS[act][1](H.float()[rev])).to(BF).float()
    return G, H, S, W, b, A @ W.float().T


def _check_launch(h, n, residual, bias, act="relu"):
    K = _K()
    G, H, S, W, b, AW = _launch_case(h, n, act)
    src, rev = G.edge_index[0], G.rev_index
    got = K.dmpnn_update(H.to(DEV), S.to(DEV), src.to(DEV), rev.to(DEV), K.pack_weights(W.to(DEV)),
                         b.to(DEV) if bias else None, residual=residual, act=K.act_code(_ACTS[act][0]()))
    assert got.dtype == BF
    ref = AW
    if bias:
        ref = ref + b.float()
    if residual:
        ref = ref + H.float()
    e = norm_err(got.float(), ref)
    print(f"update bf16 h={h} act={act} residual={residual} bias={bias}: normalised max error {e:.3e}")
    assert_parity(got.float(), ref, ULP_TOL, f"update bf16 h={h} {act}")
    assert _K()._lib.load().nt_last_kernel().startswith(b"update_bf16_kernel: wide")


# 520: one 8-wide remainder in the second K chunk and the second column pass; 1024: exactly 2 x 2;
# 1032: three passes and chunks with a sliver; 2400: five passes
@pytest.mark.parametrize("h", [520, 640, 1024, 1032, 2400])
@pytest.mark.parametrize("residual,bias", [(True, True), (False, False)])
def test_update_bf16_wide(h, residual, bias):
    _check_launch(h, 40, residual, bias)


def test_update_bf16_wide_h8192():
    _check_launch(8192, 2, True, True)


@pytest.mark.parametrize("act", ["identity", "silu"])
def test_update_bf16_wide_runtime_activations(act):
    _check_launch(640, 40, True, False, act)


def test_update_bf16_wide_rejects_h_not_multiple_of_8():
    K = _K()
    with pytest.raises(Exception, match="h % 8 == 0"):
        K.pack_weights(torch.zeros(516, 516, device=DEV, dtype=BF))


# ------------------------------------------------------------------ fused update + aggregation
def _plan(G):
    K = _K()
    dst_ptr, perm = K.csr_build(G.edge_index[1].contiguous().to(DEV), G.num_nodes)
    deg = (dst_ptr[1:] - dst_ptr[:-1]).cpu()
    plan = K.tile_plan(dst_ptr, G.num_edges, int(deg.max()))  # 64-row tiles
    return dst_ptr, perm, plan, bool((deg == 0).any())


def _check_fused(G, h, reduce, agg):
    K = _K()
    E, V = G.num_edges, G.num_nodes
    H, S = _rand_bf16(E, h, seed=14).to(DEV), _rand_bf16(V, h, seed=15).to(DEV)
    W = (_rand_bf16(h, h, seed=16).float() / h ** 0.5).to(BF)
    b = _rand_bf16(h, seed=17).to(DEV)
    Wp = K.pack_weights(W.to(DEV))
    src, rev = G.edge_index[0].to(DEV), G.rev_index.to(DEV)
    dst_ptr, perm, plan, zf = _plan(G)
    relu, agg_act = K.act_code(nn.ReLU()), K.act_code(_ACTS[agg][0]())
    Hn, Sn = K.dmpnn_update_fused(H, S, src, rev, Wp, b, residual=True, act=relu, plan=plan, perm=perm,
                                  reduce=reduce, agg_act=agg_act, zero_fill=zf)
    assert _K()._lib.load().nt_last_kernel().startswith(b"update_bf16_kernel: wide")
    plain = K.dmpnn_update(H, S, src, rev, Wp, b, residual=True, act=relu)
    assert torch.equal(Hn, plain), f"fused H_out differs from the plain launch h={h} {reduce} {agg}"
    ref = K.segment_reduce(plain, dst_ptr, perm, V, reduce=reduce, act=agg_act)
    e = norm_err(Sn.float(), ref.float())
    print(f"fused bf16 h={h} {reduce} {agg}: S_out normalised max error {e:.3e}")
    assert_parity(Sn.float(), ref.float(), ULP_TOL, f"S_out h={h} {reduce} {agg}")
    return zf, Sn


@pytest.mark.parametrize("h", [520, 1024])
@pytest.mark.parametrize("reduce,agg", [("sum", "relu"), ("sum", "identity"), ("max", "relu"),
                                        ("mean", "identity")])
def test_update_fused_bf16_wide(h, reduce, agg):
    _check_fused(_graph("zinc", 40, seed=9), h, reduce, agg)


def test_update_fused_bf16_wide_zero_in_degree_nodes():
    from notorch_amd.data.models.graph import BatchedGraph, Graph

    gs = [
        Graph(torch.zeros(3, 7, dtype=torch.long), torch.zeros(4, 2, dtype=torch.long),
              torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), torch.tensor([1, 0, 3, 2])),
        Graph(torch.zeros(1, 7, dtype=torch.long), torch.zeros(0, 2, dtype=torch.long),
              torch.zeros(2, 0, dtype=torch.long), torch.zeros(0, dtype=torch.long)),
        Graph(torch.zeros(2, 7, dtype=torch.long), torch.zeros(2, 2, dtype=torch.long),
              torch.tensor([[0, 1], [1, 0]]), torch.tensor([1, 0])),
    ]
    G = BatchedGraph.from_graphs(gs, rev_offset="edges")
    zf, Sn = _check_fused(G, 520, "sum", "relu")
    assert zf and (Sn[3] == 0).all()


def test_update_fused_bf16_wide_persistent_walk():
    """More tiles than resident workgroups (two per CU) and ntiles % 8 != 0: ragged per-XCD chunks,
    several tiles per workgroup, each walking its column passes and K chunks."""
    K = _K()
    h = 1024
    slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    per_mol = _graph("qm9", 64, seed=11).num_edges / 64
    n0 = int((slots + 4) * 64 / per_mol)
    for n in range(n0, 2 * n0, 7):
        G = _graph("qm9", n, seed=11)
        dst_ptr, perm, plan, zf = _plan(G)
        if plan[1] % 8 != 0 and plan[1] > slots + 3:
            break
    else:
        pytest.fail("no batch size in range gives the wanted tile count")
    E, V = G.num_edges, G.num_nodes
    H, S = _rand_bf16(E, h, seed=n), _rand_bf16(V, h, seed=n + 1)
    W = (_rand_bf16(h, h, seed=2).float() / h ** 0.5).to(BF)
    b = _rand_bf16(h, seed=3)
    relu = K.act_code(nn.ReLU())
    Hn, Sn = K.dmpnn_update_fused(H.to(DEV), S.to(DEV), G.edge_index[0].to(DEV), G.rev_index.to(DEV),
                                  K.pack_weights(W.to(DEV)), b.to(DEV), residual=True, act=relu, plan=plan,
                                  perm=perm, agg_act=relu, zero_fill=zf)
    # CPU layer reference (chemprop.py:36-43, residual.py:27-28, the next layer's chemprop.py:37-39)
    src, dst, rev = G.edge_index[0], G.edge_index[1], G.rev_index
    Hf = H.float()
    rH = Hf + nn.functional.linear(S.float()[src] - torch.relu(Hf)[rev], W.float(), b.float())
    rS = dmpnn_ref.scatter(torch.relu(rH), dst, V, "sum")
    assert_parity(Hn.float(), rH, WALK_TOL, f"walk H ntiles={plan[1]}")
    assert_parity(Sn.float(), rS, WALK_TOL, f"walk S ntiles={plan[1]}")


# ------------------------------------------------------------------ dense mode (the backward's dA)
@pytest.mark.parametrize("h,M", [(640, 700), (1024, 1), (1024, 3000)])
def test_dense_matmul_bf16_wide(h, M):
    K = _K()
    g = torch.Generator().manual_seed(M + h)
    X = torch.randn(M, h, generator=g).to(BF)
    W = (torch.randn(h, h, generator=g) / h ** 0.5).to(BF)
    out = K.dense_matmul(X.to(DEV), K.pack_weights(W.t().contiguous().to(DEV)))
    assert out.dtype == BF
    assert_parity(out.float(), X.float() @ W.float(), ULP_TOL, f"dense bf16 h={h} M={M}")


# ------------------------------------------------------------------ block + readout
def _block_vs_torch_bf16(kind, n, h, depth, seed=0, dropout_seed=None, **opts):
    """Device block + Sum against fp64 truth, no further than BF16_FACTOR x the torch-bf16 restatement
    on the same device.  Returns the engine's record of the last layer launch.
    dropout_seed (with opts["dropout"] > 0): a training-mode forward; the restatements get the block's
    own masks, recovered by running nt_dropout_residual on ones (keep / (1 - p), cast to the
    restatement's dtype: the bf16 one then carries one extra rounding per layer, as the device path does
    by storing the update before the dropout kernel)."""
    from notorch_amd.nn import ChempropBlock, Sum
    from notorch_amd.nn.gnn import _engine

    G = _graph(kind, n, seed=seed)
    torch.manual_seed(seed)
    emb_v = nn.EmbeddingBag(42, h, mode="sum")
    emb_e = nn.EmbeddingBag(13, h, mode="sum")
    with torch.no_grad():
        Xv, Xe = emb_v(G.node_feats).to(BF), emb_e(G.edge_feats).to(BF)
    blk = ChempropBlock(hidden_dim=h, depth=depth, **opts).to(BF)
    blk = blk.eval() if dropout_seed is None else blk.train()
    Ws, bs = dmpnn_ref.block_params(blk)
    act = {nn.ReLU: torch.relu, nn.SiLU: torch.nn.functional.silu}[type(blk._chemprop_layers()[0].act)]
    ei, rev, bni = G.edge_index.to(DEV), G.rev_index.to(DEV), G.batch_node_index.to(DEV)
    Gd = G.update(node_feats=Xv, edge_feats=Xe).to(DEV)
    masks = None
    if dropout_seed is not None:
        p, E = opts["dropout"], G.num_edges
        torch.manual_seed(dropout_seed)
        drawn = _engine.draw_dropout_seed()
        ones = torch.ones(E, h, device=DEV, dtype=BF)
        masks = [(_K().dropout_residual(ones, p, drawn, _engine.dropout_offset(l, E, h)) != 0).double() / (1 - p)
                 for l in range(depth)]
        assert all(0.6 < (m != 0).double().mean().item() < 0.9 for m in masks)

    def restated(dtype):
        with torch.inference_mode():
            kw = {} if masks is None else dict(dropout_masks=[m.to(dtype) for m in masks])
            nd, e = dmpnn_ref.chemprop_block(
                Xv.to(DEV, dtype), Xe.to(DEV, dtype), ei, rev, [W.to(DEV, dtype) for W in Ws],
                [None if b is None else b.to(DEV, dtype) for b in bs], act=act,
                residual=opts.get("residual", True), reduce=opts.get("reduce", "sum"), **kw)
            return e, nd, dmpnn_ref.readout(nd, bni, len(G), "sum")

    truth = restated(torch.float64)
    torch_bf16 = restated(BF)
    _engine.LAST_UPDATE_INFO.clear()
    if dropout_seed is not None:
        torch.manual_seed(dropout_seed)  # the block draws the same seed
    with torch.no_grad():
        out_G = blk.to(DEV)(Gd)
        dev = (out_G.edge_feats, out_G.node_feats, Sum()(out_G))
    info = dict(_engine.LAST_UPDATE_INFO)
    for what, d, t, ref in zip(("edge", "node", "readout"), dev, torch_bf16, truth):
        assert d.dtype == BF, what
        e_dev, e_t = norm_err(d, ref), norm_err(t, ref)
        l_dev, l_t = _rel_l2(d, ref), _rel_l2(t, ref)
        print(f"{kind} h={h} {opts} {what}: device vs fp64 max {e_dev:.3e} L2 {l_dev:.3e}; torch bf16 vs fp64 "
              f"max {e_t:.3e} L2 {l_t:.3e}")
        assert e_dev <= BF16_FACTOR * e_t, f"{what}: max err {e_dev:.3e} > {BF16_FACTOR} x torch bf16 {e_t:.3e}"
        assert l_dev <= BF16_FACTOR * l_t, f"{what}: L2 err {l_dev:.3e} > {BF16_FACTOR} x torch bf16 {l_t:.3e}"
        # and the absolute bf16 block criterion of tests/test_gpu_bf16.py: on hub graphs
        # torch's bf16 scatter loses whole digits, and the relative yardstick alone would ask little
        assert e_dev <= BLOCK_TOL, f"{what}: max err {e_dev:.3e} > {BLOCK_TOL}"
    return info


@pytest.mark.parametrize("h", [640, 1024])
@pytest.mark.parametrize("opts", [dict(), dict(reduce="mean"), dict(residual=False), dict(shared=True),
                                  dict(act=nn.SiLU)])
def test_block_bf16_wide(h, opts):
    info = _block_vs_torch_bf16("zinc", 64, h, 3, seed=4, **opts)
    assert info["fused"] and info["kernel_short"] == "update_bf16", info
    assert "wide" in info["kernel"], info


def test_block_bf16_wide_polymer_hubs():
    """A hub graph has no tile plan: the plain launch per layer and the chunked segment reduce."""
    info = _block_vs_torch_bf16("polymer", 2, 640, 3, seed=5, reduce="mean")
    assert info["fused"] is False and info["kernel_short"] == "update_bf16", info


def test_embedded_block_bf16_wide():
    from notorch_amd.nn import ChempropBlock, EmbeddedChempropBlock, GraphEmbedding

    G = _graph("zinc", 64, seed=5)
    torch.manual_seed(3)
    emb = GraphEmbedding(42, 13, 640)
    blk = ChempropBlock(hidden_dim=640, depth=3)
    fused = EmbeddedChempropBlock(emb, blk).eval().to(BF).to(DEV)
    Gd = G.to(DEV)
    with torch.no_grad():
        out = fused(Gd)
        unfused = blk(emb(Gd))
    assert out.edge_feats.dtype == BF
    assert torch.equal(out.node_feats, unfused.node_feats)
    assert torch.equal(out.edge_feats, unfused.edge_feats)


# ------------------------------------------------------------------ training
def test_block_grads_bf16_wide(monkeypatch):
    """h = 640: dA runs on the layer kernel's dense mode (K.dense_matmul), the weight gradient on the
    message kernel + library GEMM (the bf16 weight-gradient kernel stops at h = 512)."""
    from notorch_amd import kernels as K
    from notorch_amd.nn import ChempropBlock, Sum

    h, depth = 640, 2
    G = _graph("zinc", 16, seed=3)
    torch.manual_seed(0)
    Xv = nn.EmbeddingBag(42, h, mode="sum")(G.node_feats).detach().to(BF)
    Xe = nn.EmbeddingBag(13, h, mode="sum")(G.edge_feats).detach().to(BF)
    torch.manual_seed(1)
    blk = ChempropBlock(h, depth=depth, act=nn.SiLU).to(DEV, BF).train()

    Ws, bs = dmpnn_ref.block_params(blk)
    Ws = [W.detach().double().requires_grad_(True) for W in Ws]
    bs = [b.detach().double().requires_grad_(True) for b in bs]
    Xv_r, Xe_r = Xv.double().requires_grad_(True), Xe.double().requires_grad_(True)
    nd, e = dmpnn_ref.chemprop_block(Xv_r, Xe_r, G.edge_index, G.rev_index, Ws, bs,
                                     act=torch.nn.functional.silu, residual=True, reduce="sum")
    r = dmpnn_ref.readout(nd, G.batch_node_index, len(G), "sum")
    (r.pow(2).sum() + (e * torch.linspace(-1, 1, h, dtype=torch.float64)).sum()).backward()
    truth = [Xv_r.grad, Xe_r.grad] + [W.grad for W in Ws] + [b.grad for b in bs]

    dense_calls = []
    real = K.dense_matmul
    monkeypatch.setattr(K, "dense_matmul", lambda *a, **k: dense_calls.append(a[0].shape) or real(*a, **k))

    def device(mode):
        monkeypatch.setenv("NT_BWD", mode)
        for p in blk.parameters():
            p.grad = None
        Xv_d, Xe_d = Xv.to(DEV).requires_grad_(True), Xe.to(DEV).requires_grad_(True)
        out = blk(G.update(node_feats=Xv_d, edge_feats=Xe_d).to(DEV))
        ef = out.edge_feats.float()
        (Sum()(out).float().pow(2).sum() + (ef * torch.linspace(-1, 1, h, device=DEV)).sum()).backward()
        layers = blk._chemprop_layers()
        return ([Xv_d.grad, Xe_d.grad] + [l.linear.weight.grad for l in layers]
                + [l.linear.bias.grad for l in layers])

    got = device("kernel")
    assert len(dense_calls) == depth and all(s == (G.num_edges, h) for s in dense_calls), dense_calls
    ref = device("torch")
    names = ["dXv", "dXe"] + [f"dW[{l}]" for l in range(depth)] + [f"db[{l}]" for l in range(depth)]
    for name, a, rf, t in zip(names, got, ref, truth):
        assert a.dtype == BF and torch.isfinite(a.float()).all(), name
        e_max, r_max = norm_err(a.float(), t), norm_err(rf.float(), t)
        e_l2, r_l2 = _rel_l2(a, t), _rel_l2(rf, t)
        print(f"{name}: kernel max {e_max:.2e} l2 {e_l2:.2e} | torch bf16 max {r_max:.2e} l2 {r_l2:.2e}")
        assert e_max <= max(BF16_FLOOR, BF16_FACTOR * r_max), f"{name}: max {e_max:.3e} vs torch bf16 {r_max:.3e}"
        assert e_l2 <= max(BF16_FLOOR, BF16_FACTOR * r_l2), f"{name}: L2 {e_l2:.3e} vs torch bf16 {r_l2:.3e}"
