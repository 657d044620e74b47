"""nt_dmpnn_update above hidden 512: the unfused entry point that a standalone ChempropLayer forward
(chemprop.py:36-43) and a training forward with dropout (chemprop.py:26 inside `update`) go through.
fp32 with h % 4 == 0 runs update_fk_kernel's plain mode (column chunks, h <= 8192); bf16 with
h % 8 == 0 the bf16 kernel's column-pass variant.

Criteria: tests/test_gpu_dropout.py's (fp32 contract, masks recovered by running the dropout kernel on
ones) and tests/test_gpu_bf16.py's block criterion (no further from fp64 than BF16_FACTOR x torch bf16)."""
import pytest
import torch
import torch.nn as nn

from helpers import FP32_NORM_TOL, assert_parity
from oracle import dmpnn_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-5
H_WIDE = 640


def _graph(n, seed):
    from notorch_amd.data.synth import make_batch

    return make_batch("qm9", n, seed=seed).collate("nodes")


def test_standalone_layer_fp32_h640():
    from notorch_amd.nn import ChempropLayer

    G = _graph(8, 6)
    h = H_WIDE
    torch.manual_seed(0)
    H = torch.randn(G.num_edges, h)
    layer = ChempropLayer(h).to(DEV).eval()
    ei, rev = G.edge_index.clone(), G.rev_index.clone()
    with torch.no_grad():
        got = layer(H.to(DEV), torch.zeros(G.num_nodes, h, device=DEV), ei.to(DEV), rev.to(DEV))
    W = layer.linear.weight.detach().double().cpu()
    b = layer.linear.bias.detach().double().cpu()
    ref = dmpnn_ref.chemprop_layer(H.double(), torch.zeros(G.num_nodes, h, dtype=torch.float64), ei, rev, W, b)
    assert_parity(got, ref, FP32_NORM_TOL, "standalone layer h=640")


def test_block_dropout_forward_and_grads_fp32_h640():
    from notorch_amd import kernels as K
    from notorch_amd.nn import ChempropBlock
    from notorch_amd.nn.gnn import _engine

    G = _graph(24, 4)
    h, depth, p = H_WIDE, 2, 0.25
    E = G.num_edges
    torch.manual_seed(0)
    Xv = nn.EmbeddingBag(42, h, mode="sum")(G.node_feats).detach()
    Xe = nn.EmbeddingBag(13, h, mode="sum")(G.edge_feats).detach()
    torch.manual_seed(1)
    blk = ChempropBlock(h, depth=depth, dropout=p).to(DEV).train()

    torch.manual_seed(99)
    seed = _engine.draw_dropout_seed()
    ones = torch.ones(E, h, device=DEV)
    masks = [K.dropout_residual(ones, p, seed, _engine.dropout_offset(l, E, h)).double().cpu()
             for l in range(depth)]
    assert all(0.6 < (m != 0).double().mean().item() < 0.9 for m in masks)

    torch.manual_seed(99)  # the block draws the same seed
    Xv_d, Xe_d = Xv.to(DEV).requires_grad_(True), Xe.to(DEV).requires_grad_(True)
    out = blk(G.update(node_feats=Xv_d, edge_feats=Xe_d).to(DEV))
    wts = torch.linspace(-1, 1, h, device=DEV)
    (out.node_feats.pow(2).sum() + (out.edge_feats * wts).sum()).backward()

    Ws, bs = dmpnn_ref.block_params(blk)
    Ws = [W.double().requires_grad_(True) for W in Ws]
    bs = [b.double().requires_grad_(True) for b in bs]
    Xv_r, Xe_r = Xv.double().requires_grad_(True), Xe.double().requires_grad_(True)
    n_r, e_r = dmpnn_ref.chemprop_block(Xv_r, Xe_r, G.edge_index, G.rev_index, Ws, bs, dropout_masks=masks)
    (n_r.pow(2).sum() + (e_r * wts.double().cpu()).sum()).backward()

    assert_parity(out.node_feats, n_r, TOL, "node")
    assert_parity(out.edge_feats, e_r, TOL, "edge")
    assert_parity(Xv_d.grad, Xv_r.grad, TOL, "dXv")
    assert_parity(Xe_d.grad, Xe_r.grad, TOL, "dXe")
    for l, layer in enumerate(blk._chemprop_layers()):
        assert_parity(layer.linear.weight.grad, Ws[l].grad, TOL, f"dW[{l}]")
        assert_parity(layer.linear.bias.grad, bs[l].grad, TOL, f"db[{l}]")


def test_block_dropout_forward_bf16_h640():
    """The same block in bf16: dropout takes the unfused bf16 update (the column-pass kernel)."""
    from test_gpu_bf16_wide import _block_vs_torch_bf16

    info = _block_vs_torch_bf16("qm9", 24, H_WIDE, 2, seed=4, dropout_seed=99, dropout=0.25)
    assert info["fused"] is False and info["kernel_short"] == "update_bf16" and "wide" in info["kernel"], info
