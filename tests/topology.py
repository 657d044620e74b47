"""Graph generators for the topology tests (tests/test_topology.py, tests/test_gpu_topology.py): what the
three synthetic molecule generators never produce.  In-degrees 5..65 on bond graphs, directed graphs
whose in-degree differs from their out-degree, and "ladders" that put a run of in-edges at a chosen
row of the layer kernel's tiles.  The engine takes any edge_index / rev_index (the reference's Graph,
graph.py:14-39, does), so every graph here is a legal input.

Every generator returns a :class:`Topology`: the per-graph ``Graph`` objects for
``BatchedGraph.from_graphs(..., rev_offset=...)`` and the batch's raw tensors for the oracle.  Features
are type indices in the synthetic vocabularies (notorch_amd.data.synth), so the same graphs feed the
embedded block; :func:`embed` turns them into float features.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn

from helpers import norm_err
from oracle import dmpnn_ref

GRAD_TOL = 1e-5  # tests/test_gpu_backward.py
# the fp32 oracle's own error against fp64 on every gradient case stays below this, so the rule
# tol = max(GRAD_TOL, 4 x floor) never widens GRAD_TOL (tests/test_topology.py checks it on the CPU)
GRAD_FLOOR_MAX = 2.5e-6


@dataclass
class Topology:
    graphs: list  # notorch_amd Graph objects (type-index features)
    V: int
    edge_index: torch.Tensor  # 2 x E, batch-global node ids
    rev_local: list  # per graph: rev_index in the graph's own edge ids
    batch: torch.Tensor  # V: graph of every node

    @property
    def E(self) -> int:
        return self.edge_index.shape[1]

    def rev_index(self, rev_offset: str = "nodes") -> torch.Tensor:
        """The batch's rev_index as the collate builds it: each graph's offset by the running node
        count ("nodes", the reference) or edge count ("edges")."""
        out, off = [], 0
        for G, r in zip(self.graphs, self.rev_local):
            out.append(r + off)
            off += G.num_nodes if rev_offset == "nodes" else G.num_edges
        return torch.cat(out)

    def raw(self, rev_offset: str = "nodes"):
        """(V, edge_index, rev_index, batch) for the oracle."""
        return self.V, self.edge_index, self.rev_index(rev_offset), self.batch

    def collate(self, rev_offset: str = "nodes"):
        from notorch_amd.data.models.graph import BatchedGraph

        return BatchedGraph.from_graphs(self.graphs, rev_offset=rev_offset)

    def in_degree(self) -> torch.Tensor:
        return torch.bincount(self.edge_index[1], minlength=self.V)

    def out_degree(self) -> torch.Tensor:
        return torch.bincount(self.edge_index[0], minlength=self.V)


def _topology(parts, rng) -> Topology:
    """parts: per graph (n nodes, edge_index 2 x e int64 numpy (local ids), rev e, per-edge type rows)."""
    from notorch_amd.data.models.graph import Graph
    from notorch_amd.data.synth import _types

    graphs, eis, revs, batch = [], [], [], []
    off = 0
    for i, (n, ei, rev, bond_of_edge) in enumerate(parts):
        nb = int(bond_of_edge.max()) + 1 if len(bond_of_edge) else 0
        atom_types, bond_types = _types(rng, n, nb)
        ei_t, rev_t = torch.from_numpy(ei.astype(np.int64)), torch.from_numpy(rev.astype(np.int64))
        graphs.append(Graph(torch.from_numpy(atom_types), torch.from_numpy(bond_types[bond_of_edge]), ei_t, rev_t))
        eis.append(ei_t + off)
        revs.append(rev_t)
        batch.append(torch.full((n,), i, dtype=torch.int64))
        off += n
    return Topology(graphs, off, torch.cat(eis, dim=1), revs, torch.cat(batch))


def capped_bonds(mols, seed: int = 0) -> Topology:
    """Symmetric bond graphs in MolToGraph layout (bond b -> edges 2b = (u->v), 2b+1 = (v->u),
    rev = e ^ 1), one per entry of ``mols``, a list of per-atom degree caps.  Greedy: for u in order,
    bond u to a random v while both are under their caps and the pair is new.  In-degree = out-degree =
    the atom's bond count <= its cap; with enough partners the first atoms reach their caps exactly."""
    rng = np.random.default_rng(seed)
    parts = []
    for caps in mols:
        caps = np.asarray(caps, dtype=np.int64)
        n = len(caps)
        deg = np.zeros(n, dtype=np.int64)
        adj = np.zeros((n, n), dtype=bool)
        bonds = []
        for u in range(n):
            while deg[u] < caps[u]:
                ok = (deg < caps) & ~adj[u]
                ok[u] = False
                cand = np.flatnonzero(ok)
                if len(cand) == 0:
                    break
                v = int(cand[rng.integers(len(cand))])
                adj[u, v] = adj[v, u] = True
                deg[u] += 1
                deg[v] += 1
                bonds.append((u, v))
        b = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
        ei = np.empty((2, 2 * len(b)), dtype=np.int64)
        ei[0, 0::2], ei[1, 0::2] = b[:, 0], b[:, 1]
        ei[0, 1::2], ei[1, 1::2] = b[:, 1], b[:, 0]
        parts.append((n, ei, np.arange(2 * len(b)) ^ 1, np.repeat(np.arange(len(b)), 2)))
    return _topology(parts, rng)


def hub_caps(hubs, n_rest: int, seed: int = 0) -> list:
    """Degree caps of one molecule: the given hub degrees first, then n_rest atoms with caps 1..4
    (mixed degrees: a regular molecule's mean-reduce weight gradient is identically zero)."""
    rng = np.random.default_rng(seed)
    return list(hubs) + rng.integers(1, 5, size=n_rest).tolist()


def directed(indeg, seed: int = 0) -> Topology:
    """One directed graph with the prescribed in-degree sequence: edge order shuffled, sources drawn
    from the first half of the nodes only (so a first-half node of in-degree 0 still has out-edges, and
    a second-half node of in-degree > 0 has none), rev_index an arbitrary in-range gather."""
    rng = np.random.default_rng(seed)
    indeg = np.asarray(indeg, dtype=np.int64)
    n = len(indeg)
    dst = np.repeat(np.arange(n), indeg)
    rng.shuffle(dst)
    e = len(dst)
    src = rng.integers(0, n // 2, size=e)
    rev = rng.integers(0, e, size=e)
    return _topology([(n, np.stack([src, dst]), rev, np.arange(e))], rng)


def ladder(degs, seed: int = 0) -> Topology:
    """One directed graph whose dst-sorted edge order is exactly the in-degree sequence ``degs`` (node
    v's in-edges are positions [sum(degs[:v]), sum(degs[:v + 1])) of the dst CSR), so a run of in-edges
    sits at a chosen row of a tile.  Edge ids are shuffled; src and rev_index are random gathers."""
    rng = np.random.default_rng(seed)
    degs = np.asarray(degs, dtype=np.int64)
    n = len(degs)
    e = int(degs.sum())
    dst = np.empty(e, dtype=np.int64)
    dst[rng.permutation(e)] = np.repeat(np.arange(n), degs)
    src = rng.integers(0, n, size=e)
    rev = rng.integers(0, e, size=e)
    return _topology([(n, np.stack([src, dst]), rev, np.arange(e))], rng)


# ------------------------------------------------------------------------------------ ladders
def tile_stride(maxdeg: int, rows: int) -> int:
    """Stride of the largest-tile plan (nt_dmpnn_tile_stride with ncu = 0)."""
    return rows + 1 - max(int(maxdeg), 1)


def ladder_pieces(D: int, rows: int) -> list:
    """The runs the layer kernel's segmented scan must get right at max in-degree D, each list placed
    at the start of a tile by ladder_degs.  With D = 32: [1, 32] (a run entering a 16-row row tile
    through the carry and covering all of it: 16 rounds), [32, 32] (a 64-row tile filled exactly),
    [15, 17] and [16, 16] (runs ending / starting on a row-tile edge), [1, 31, 32], and a mix with
    in-degree-0 nodes between runs."""
    c = lambda d: max(1, min(d, D))  # noqa: E731
    pre = lambda k: [k] if k <= D else [1] * k  # noqa: E731  (k rows ahead of a run)
    pieces = [
        [1, D],
        [D] * (rows // D) if rows % D == 0 else [D, D],
        pre(15) + [c(17)],
        pre(16) + [c(16)],
        [1] + pre(31) + [D],
        pre(15) + [D],  # D <= 17: the run's last row needs min(D - 1, 16) rounds
        [c(7), 0, c(9), D, 0, 0, c(3), D],
        [d for d in (0, 1, 4, 0, 5, 9, 0, 0, 10, 16, 0, 17, 1, 0) if d <= D],
    ]
    return pieces


def ladder_degs(D: int, rows: int) -> list:
    """In-degree sequence holding every piece of ladder_pieces(D, rows) at the start of a tile of the
    largest-tile plan: single-edge nodes pad the position to the next multiple of the stride."""
    stride = tile_stride(D, rows)
    degs, pos = [], 0
    for piece in ladder_pieces(D, rows):
        pad = -pos % stride
        degs += [1] * pad + piece
        pos += pad + sum(piece)
    return degs + [0, 2, 0]


def ladder_rows(degs, D: int, rows: int):
    """(tile sizes, per node (row of its first in-edge in its tile, in-degree)) of the largest-tile plan
    (tile k starts at the first node boundary >= k * stride), and the scan rounds the worst row needs:
    a row is final after its distance from its run's first row, or, when the run entered its 16-row row
    tile through the carry, after its row in that row tile + 1."""
    stride = tile_stride(D, rows)
    ptr = np.concatenate([[0], np.cumsum(degs)])
    E = int(ptr[-1])
    ntiles = (E + stride - 1) // stride
    starts = [int(ptr[np.searchsorted(ptr, k * stride, side="left")]) for k in range(ntiles)] + [E]
    starts = np.asarray(starts)
    sizes = np.diff(starts)
    runs, rounds = [], 0
    for v, d in enumerate(degs):
        if d == 0:
            continue
        t = int(np.searchsorted(starts, ptr[v], side="right")) - 1
        s = int(ptr[v] - starts[t])
        runs.append((s, int(d)))
        for r in range(s, s + d):
            rounds = max(rounds, r - s if s >= 16 * (r // 16) else r % 16 + 1)
    return sizes, runs, rounds


# ------------------------------------------------------------------------------------ features, gradients
def embed(n_node_types, n_edge_types, h: int, seed: int = 0, scale: float = 1.0):
    """Float features from type indices, as the tests of the molecule graphs draw them."""
    torch.manual_seed(seed)
    nt = nn.EmbeddingBag(42, h, mode="sum")
    et = nn.EmbeddingBag(13, h, mode="sum")
    with torch.no_grad():
        return nt(n_node_types) * scale, et(n_edge_types) * scale


ACTS = {"ReLU": (nn.ReLU, torch.relu), "SiLU": (nn.SiLU, torch.nn.functional.silu)}


def make_block(h, depth, act="ReLU", reduce="sum", seed=1, w_var=1.0, **opts):
    """A ChempropBlock with W ~ N(0, w_var / h) (biases as nn.Linear draws them)."""
    from notorch_amd.nn import ChempropBlock

    torch.manual_seed(seed)
    blk = ChempropBlock(h, act=ACTS[act][0], depth=depth, reduce=reduce, **opts)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for layer in {id(l): l for l in blk._chemprop_layers()}.values():
            layer.linear.weight.copy_(torch.randn(h, h, generator=g) * (w_var / h) ** 0.5)
    return blk


def readout_of(reduce: str) -> str:
    """The readout a gradient case pairs with its aggregation."""
    return "mean" if reduce == "mean" else "sum"


def oracle_grads(raw, n_graphs, Xv, Xe, blk, act, reduce, dtype, residual=True):
    """tests/test_gpu_backward.py's recipe on raw tensors: loss = sum(readout^2) + sum(edge * ramp),
    gradients by the oracle's autograd in ``dtype``."""
    V, edge_index, rev, batch = raw
    Ws, bs = dmpnn_ref.block_params(blk)
    Ws = [W.detach().to(dtype, copy=True).requires_grad_(True) for W in Ws]
    bs = [None if b is None else b.detach().to(dtype, copy=True).requires_grad_(True) for b in bs]
    Xv_r = Xv.detach().to(dtype, copy=True).requires_grad_(True)
    Xe_r = Xe.detach().to(dtype, copy=True).requires_grad_(True)
    n, e = dmpnn_ref.chemprop_block(Xv_r, Xe_r, edge_index, rev, Ws, bs, act=ACTS[act][1], residual=residual,
                                    reduce=reduce)
    r = dmpnn_ref.readout(n, batch, n_graphs, readout_of(reduce))
    loss = r.pow(2).sum() + (e * torch.linspace(-1, 1, e.shape[1], dtype=dtype)).sum()
    loss.backward()
    return [loss.detach(), Xv_r.grad, Xe_r.grad] + [W.grad for W in Ws] + [b.grad for b in bs if b is not None]


def grad_names(depth):
    return ["loss", "dXv", "dXe"] + [f"dW[{l}]" for l in range(depth)] + [f"db[{l}]" for l in range(depth)]


def oracle_floor(raw, n_graphs, Xv, Xe, blk, act, reduce):
    """(fp64 gradients, the fp32 oracle's largest normalised error against them)."""
    truth = oracle_grads(raw, n_graphs, Xv, Xe, blk, act, reduce, torch.float64)
    o32 = oracle_grads(raw, n_graphs, Xv, Xe, blk, act, reduce, torch.float32)
    return truth, max(norm_err(a, b) for a, b in zip(o32[1:], truth[1:]))


# ------------------------------------------------------------------------------------ the test graphs
def block_graph(name: str) -> Topology:
    """The graphs of the block tests, by name.  b<D>: bond graphs with max in-degree D (others <= 4);
    b33mix: max 33 with atoms at 9, 10 and 32; dir: one directed graph."""
    if name == "dir":
        rng = np.random.default_rng(5)
        indeg = rng.integers(0, 7, size=120)
        indeg[:8] = [0, 0, 3, 0, 12, 0, 1, 0]  # first half: in-degree 0 with out-edges
        indeg[-6:] = [32, 0, 17, 9, 0, 5]  # second half: in-degree > 0, no out-edge
        return directed(indeg, seed=6)
    hubs = {"b9": [9], "b10": [10], "b32": [32], "b33": [33], "b33mix": [33, 32, 10, 9], "b64": [64], "b65": [65]}[name]
    seed = sum(hubs)
    mols = [hub_caps(hubs, max(hubs) + 24, seed), hub_caps([3], 9, seed + 1), hub_caps([4], 40, seed + 2)]
    return capped_bonds(mols, seed)


BLOCK_GRAPHS = ("b9", "b10", "b32", "b33", "b33mix", "b64", "b65", "dir")
BOND_GRAPHS = BLOCK_GRAPHS[:-1]
MAX_IN_DEGREE = {"b9": 9, "b10": 10, "b32": 32, "b33": 33, "b33mix": 33, "b64": 64, "b65": 65, "dir": 32}


def full_tile_graph() -> Topology:
    """About 24.7k edges at max in-degree 32: the engine's balanced plans (256 slots) then cut tiles of
    the kernels' full capacity (stride 97 of the 128-row plan needs E just below 256 * 97 = 24 832; the
    64-row plan runs three rounds of stride 33)."""
    mols, seed = [], 0
    while len(mols) < 123:
        mols.append(hub_caps([32, 17 + seed % 9, 5 + seed % 7], 56, 100 + seed))
        seed += 1
    return capped_bonds(mols, 77)


# gradient cases of tests/test_gpu_topology.py (e): (graph, h, act, reduce); the CPU floor test runs them all
GRAD_CASES = [
    ("b32", 32, "SiLU", "sum"), ("b32", 300, "ReLU", "sum"), ("b32", 32, "ReLU", "mean"), ("b32", 32, "SiLU", "max"),
    ("b33", 32, "SiLU", "sum"), ("b33", 300, "SiLU", "mean"), ("b33", 32, "ReLU", "max"),
    ("dir", 32, "SiLU", "sum"), ("dir", 300, "ReLU", "mean"), ("dir", 32, "ReLU", "max"), ("dir", 300, "SiLU", "sum"),
    ("b10", 32, "ReLU", "sum"), ("b65", 32, "SiLU", "mean"),
]
GRAD_DEPTH = 2


def grad_case(name, h, act, reduce, rev_offset="nodes"):
    """(topology, collated graph, raw, Xv, Xe, block) of one gradient case: W ~ N(0, 1 / (16 h))."""
    T = block_graph(name)
    G = T.collate(rev_offset)
    Xv, Xe = embed(G.node_feats, G.edge_feats, h)
    blk = make_block(h, GRAD_DEPTH, act, reduce, w_var=1 / 16)
    return T, G, T.raw(rev_offset), Xv, Xe, blk
