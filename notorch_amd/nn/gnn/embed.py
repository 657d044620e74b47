"""``GraphEmbedding`` (reference ``notorch/nn/gnn/embed.py:11-36``): sum-mode EmbeddingBag of the
integer atom / bond type columns into ``node_feats`` V x h and ``edge_feats`` E x h, and
``EmbeddedChempropBlock``, the same embedding fused into the D-MPNN initial gather
(SURVEY §8(f) row 2).

``GraphEmbedding`` keeps the reference's module tree (``node`` / ``edge`` ``nn.EmbeddingBag``, so the
``state_dict`` keys match).  On a ROCm device its forward is the ``nt_embed_bag`` kernel; under
autograd it goes through ``_engine.EmbedBagFunction``, whose backward is ``nt_embed_bag_backward`` (a
deterministic LDS reduction of the output gradient into the table), so the tables train on the
kernels.  Bags with non-default options and tables that are neither fp32 nor bf16 run
``nn.EmbeddingBag`` itself (device ops).  On the CPU it is the reference module unchanged (it is the
featurisation step ahead of the hot path, not the hot path).

``EmbeddedChempropBlock(embedding, block)`` computes ``block(embedding(G))`` — a drop-in for that
pair of modules in a ``TensorDictSequential`` — and, on the device, runs ``nt_dmpnn_init_embed``:
``H0 = Xv[src] + Xe`` straight from the type indices and the two tables, so the V x h / E x h embedded
matrices are never written nor read back.  Bit-identical to the unfused pair.  When gradients are
needed it runs ``_engine.EmbeddedBlockFunction``: the same forward with the layer states kept (active
dropout included, with the unfused path's masks), and a backward that ends in two
``nt_embed_bag_backward`` launches over ``G = dL/dH0`` (the node table through the src CSR, so dXv is
never written either).  ``fuse=False`` is the embedding kernels, then the block; in training
``EmbedBagFunction`` followed by ``ChempropBlockFunction``.  Mixed or generic activations go through
``block(embedding(G))``.  ``NT_EMBED_BWD=torch`` selects the library path for training instead
(``nn.EmbeddingBag`` under autograd, then the block; an A/B reference).

Mixed precision.  Under ``torch.autocast(device_type="cuda", dtype=torch.bfloat16)``
``EmbeddedChempropBlock`` behaves as one lower-precision op like ``ChempropBlock`` (see
``nn/gnn/chemprop.py``): fp32 tables enter through ``nt_dmpnn_init_embed_mixed`` (both bags summed in
fp32, added in fp32, one rounding to bf16), the bf16 kernels run, the outputs are bf16, and an fp32
table receives the fp32 output of ``nt_embed_bag_backward``.  ``fuse=True`` and ``fuse=False`` return the
same bits.  ``GraphEmbedding`` on its own does not take part in autocast: it returns the dtype of its
tables (fp32 for fp32 tables, as torch's ``embedding_bag`` under autocast), and the readouts follow
the dtype of their input.
"""
from __future__ import annotations

import os
import weakref

import torch
import torch.nn as nn

from notorch_amd import kernels as K
from notorch_amd._lib import NT_ACT_IDENTITY
from notorch_amd.data.models.graph import types_in_range
from notorch_amd.data.synth import DEFAULT_NUM_ATOM_TYPES, DEFAULT_NUM_BOND_TYPES
from notorch_amd.nn.gnn import _engine
from notorch_amd.nn.gnn.chemprop import ChempropBlock, _dropout, autocast_bf16_applies
from notorch_amd.nn.residual import Residual

DEFAULT_HIDDEN_DIM = 256  # notorch/conf.py


def _plain_bag(bag: nn.EmbeddingBag) -> bool:
    """The kernel covers the default EmbeddingBag configuration GraphEmbedding builds."""
    return (bag.mode == "sum" and bag.max_norm is None and bag.padding_idx is None
            and not bag.scale_grad_by_freq and not bag.include_last_offset)


def _embed_bwd_kernel() -> bool:
    """NT_EMBED_BWD=torch: train the tables through nn.EmbeddingBag (library ops) instead of the kernels."""
    return os.environ.get("NT_EMBED_BWD", "kernel") != "torch"


class GraphEmbedding(nn.Module):
    def __init__(
        self,
        num_node_types: int = DEFAULT_NUM_ATOM_TYPES,
        num_edge_types: int = DEFAULT_NUM_BOND_TYPES,
        hidden_dim: int = DEFAULT_HIDDEN_DIM,
    ):
        super().__init__()
        self.node = nn.EmbeddingBag(num_node_types, hidden_dim, mode="sum")
        self.edge = nn.EmbeddingBag(num_edge_types, hidden_dim, mode="sum")

    def _kernel_ok(self, G) -> bool:
        w = self.node.weight
        return (w.device.type == "cuda" and G.node_feats.dim() == 2 and G.edge_feats.dim() == 2
                and _plain_bag(self.node) and _plain_bag(self.edge))

    def _needs_grad(self) -> bool:
        return torch.is_grad_enabled() and (self.node.weight.requires_grad or self.edge.weight.requires_grad)

    def _use_kernel(self, G) -> bool:
        """The inference kernel applies (no gradient needed)."""
        return self._kernel_ok(G) and not self._needs_grad()

    def _train_kernel(self, G) -> bool:
        """The kernel pair under autograd applies (EmbedBagFunction)."""
        return (self._kernel_ok(G) and self._needs_grad() and _embed_bwd_kernel()
                and all(b.weight.dtype in (torch.float32, torch.bfloat16) for b in (self.node, self.edge)))

    def forward(self, G):
        train = self._train_kernel(G)
        if train or self._use_kernel(G):
            nt_, et_ = G.node_feats.contiguous(), G.edge_feats.contiguous()
            ok = types_in_range(getattr(G, "_nt_layout", None), nt_, et_, self.num_node_types,
                                self.num_edge_types)
            if ok is False:
                raise IndexError("type index out of range for the embedding tables")
            if train:
                Xv = _engine.EmbedBagFunction.apply(self.node.weight, nt_, ok is None)
                Xe = _engine.EmbedBagFunction.apply(self.edge.weight, et_, ok is None)
            else:
                Xv = K.embed_bag(self.node.weight.detach(), nt_, validate=ok is None)
                Xe = K.embed_bag(self.edge.weight.detach(), et_, validate=ok is None)
            return G.update(node_feats=Xv, edge_feats=Xe)
        return G.update(node_feats=self.node(G.node_feats), edge_feats=self.edge(G.edge_feats))

    @property
    def num_node_types(self) -> int:
        return self.node.num_embeddings

    @property
    def num_edge_types(self) -> int:
        return self.edge.num_embeddings


class EmbeddedChempropBlock(nn.Module):
    """``block(embedding(G))`` with the embedding fused into the block's initial gather."""

    def __init__(self, embedding: GraphEmbedding, block: ChempropBlock, fuse: bool = True):
        super().__init__()
        self.embedding = embedding
        self.block = block
        self.fuse = fuse  # False: GraphEmbedding kernel, then the block (same bytes out)

    def forward(self, G):
        emb, blk = self.embedding, self.block
        needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        dropout = any(l.training and l.update[1].p > 0 for l in blk._chemprop_layers())
        fusable = (
            self.fuse
            and G.node_feats.device.type == "cuda"
            and emb._kernel_ok(G)
            and emb.node.weight.dtype == emb.edge.weight.dtype
            # training: the kernel backward (EmbeddedBlockFunction); inference: no dropout to apply
            and ((_embed_bwd_kernel() and emb.node.weight.dtype in (torch.float32, torch.bfloat16))
                 if needs_grad else not dropout)
        )
        layers = blk._chemprop_layers()
        codes = [_engine.layer_act(l.act) for l in layers]
        dps = {float(l.update[1].p) if l.training and l.update[1].p > 0 else None for l in layers}
        if not fusable or any(c is None for c in codes) or len(set(codes)) > 1 or len(dps) > 1:
            return blk(emb(G))  # the block takes generic / mixed activations (and dropouts) layer by layer
        # under bf16 autocast the pair is one lower-precision op: fp32 and bf16 tensors may meet
        bf16_compute = autocast_bf16_applies(
            emb.node.weight.device, emb.node.weight.shape[1],
            [emb.node.weight, emb.edge.weight] + [p for l in layers for p in (l.linear.weight, l.linear.bias)])
        if not bf16_compute and any(l.linear.weight.dtype != emb.node.weight.dtype for l in layers):
            raise RuntimeError("embedding tables and layer weights must share one dtype")
        act = codes[0] if codes else (NT_ACT_IDENTITY, 0.0)
        residual = bool(layers) and isinstance(blk.layers[0], Residual)
        # the layout needs V: give dst_layout a graph whose node_feats has V rows (the type matrix)
        lay = _engine.dst_layout(G)
        node_types, edge_types = G.node_feats.contiguous(), G.edge_feats.contiguous()
        # not through _layout._cached: the entry holds the type tensors weakly (a pinned object would keep
        # a batch's features alive with its layout) and is written only after a forward that passed
        seen = lay.embed_checked
        # the check is against these table sizes: a smaller table must re-validate the indices
        key = (node_types._version, edge_types._version, emb.node.num_embeddings, emb.edge.num_embeddings)
        validate = not (
            seen is not None and seen[0]() is node_types and seen[1]() is edge_types and seen[2] == key
        )
        if validate:  # the collate's host statistics answer without a device -> host sync
            ok = types_in_range(lay, node_types, edge_types, emb.node.num_embeddings, emb.edge.num_embeddings)
            if ok is False:
                raise IndexError("type index out of range for the embedding tables")
            validate = ok is None
        if needs_grad:
            node, H = _engine.EmbeddedBlockFunction.apply(
                emb.node.weight, emb.edge.weight, node_types, edge_types, G.edge_index, G.rev_index.contiguous(),
                lay, layers[0].act if layers else nn.Identity(), act, blk.reduce, residual, len(layers),
                _dropout(layers), validate, bf16_compute,
                *[l.linear.weight for l in layers], *[l.linear.bias for l in layers],
            )
        else:
            node, H, _ = _engine.block_forward_embedded(
                emb.node.weight.detach(), node_types, emb.edge.weight.detach(), edge_types,
                G.edge_index[0].contiguous(), G.rev_index.contiguous(), lay,
                [l.linear.weight for l in layers], [l.linear.bias for l in layers], act, blk.reduce,
                residual, validate=validate, bf16_compute=bf16_compute,
            )
        # type indices validated for these tensors: no host sync on the next call
        lay.embed_checked = (weakref.ref(node_types), weakref.ref(edge_types), key)
        return G.update(node_feats=node, edge_feats=H)
