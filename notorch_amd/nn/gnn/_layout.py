"""What the engine derives from a graph's indices and keeps on its DeviceLayout: the dst / molecule
CSRs, degree statistics, tile and chunk plans, row tables and the backward's CSRs.  Every lazily built
entry goes through _cached, and every attribute set here is a declared DeviceLayout field."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from notorch_amd import kernels as K
from notorch_amd.data.models.graph import DeviceLayout


def _cached(lay: DeviceLayout, name: str, key: tuple, build, pin=None):
    """The value stored under lay.<name> if it was built for an equal key (a tuple) and the same pinned
    object (`is`: a tensor whose identity, not only its storage, the value depends on), else build() is
    stored and returned.  Entries are (pin, value, *key)."""
    hit = getattr(lay, name, None)
    if hit is None or hit[0] is not pin or hit[2:] != key:
        hit = (pin, build(), *key)
        setattr(lay, name, hit)
    return hit[1]


def _validate_indices(edge_index: Tensor, rev_index: Tensor, V: int) -> None:
    E = edge_index.shape[-1]
    if rev_index.numel() != E:
        raise RuntimeError(f"rev_index has {rev_index.numel()} entries for {E} edges")
    if E == 0:
        return
    mm = torch.stack(
        [edge_index.min(), edge_index.max(), rev_index.min(), rev_index.max()]
    ).cpu()  # one sync per new graph (the collate path validates on the host instead)
    if mm[0] < 0 or mm[1] >= V:
        raise IndexError(f"edge_index out of range for {V} nodes")
    if mm[2] < 0 or mm[3] >= E:
        raise IndexError(f"rev_index out of range for {E} edges")


def dst_layout(G) -> DeviceLayout:
    """The in-edge CSR of ``G`` on its device: cached from the collate, else built with nt_csr_build."""
    ei = G.edge_index
    lay: Optional[DeviceLayout] = getattr(G, "_nt_layout", None)
    if (
        lay is not None
        and lay.dst_ptr is not None
        and lay.validated
        and lay.edge_index is ei
        and lay.dst_ptr.device == ei.device
    ):
        return lay
    V = G.node_feats.shape[0]
    _validate_indices(ei, G.rev_index, V)
    dst = ei[1].contiguous()
    dst_ptr, dst_perm = K.csr_build(dst, V, check_bounds=False)
    new = DeviceLayout(dst_ptr, dst_perm, edge_index=ei, validated=True)
    if lay is not None and lay.mol_ptr is not None and lay.mol_ptr.device == ei.device:
        new.mol_ptr, new.mol_perm, new.batch_node_index = lay.mol_ptr, lay.mol_perm, lay.batch_node_index
    try:
        G._nt_layout = new
    except AttributeError:  # a foreign graph object that refuses new attributes: no caching
        pass
    return new


def mol_layout(G) -> tuple[Tensor, Optional[Tensor]]:
    """(mol_ptr, mol_perm) of a BatchedGraph: nodes of every molecule, for the readouts."""
    bni = G.batch_node_index
    B = len(G)
    lay: Optional[DeviceLayout] = getattr(G, "_nt_layout", None)
    if (
        lay is not None
        and lay.mol_ptr is not None
        and lay.batch_node_index is bni
        and lay.mol_ptr.device == bni.device
        and lay.mol_ptr.numel() == B + 1
    ):
        return lay.mol_ptr, lay.mol_perm
    mol_ptr, mol_perm = K.csr_build(bni.contiguous(), B, check_bounds=True)
    if lay is None:
        lay = DeviceLayout()
    lay.mol_ptr, lay.mol_perm, lay.batch_node_index = mol_ptr, mol_perm, bni
    try:
        G._nt_layout = lay
    except AttributeError:
        pass
    return mol_ptr, mol_perm


LONG_SEGMENT = 64  # segments longer than this switch the aggregation to the chunked reduce


def _degree_range(lay: DeviceLayout) -> tuple[int, int]:
    """(max, min) in-degree of the layout's dst CSR; one host sync per layout, cached."""
    mm = getattr(lay, "deg_range", None)
    if mm is None:
        deg = lay.dst_ptr[1:] - lay.dst_ptr[:-1]
        if deg.numel() == 0:
            mm = (0, 0)
        else:
            t = torch.stack([deg.max(), deg.min()]).cpu()
            mm = (int(t[0]), int(t[1]))
        lay.deg_range = mm
    return mm


MAX_FUSED_IN_DEGREE = 32  # larger in-degrees do not fit node-aligned tiles: the graph has hubs
# the hub-graph init (nt_dmpnn_init with skip_degree = MAX_FUSED_IN_DEGREE, then the chunked init over
# the skipped nodes' chunks) needs every multi-chunk segment to be a skipped node (notorch_amd.h)
assert K.CHUNK_ROWS >= MAX_FUSED_IN_DEGREE, "chunk rows must cover the wave init's in-degree cut"
HUB_DEGREE = 9  # in a hub graph, nodes with more in-edges are cut at the stride and reduced separately


def hub_info(lay: DeviceLayout):
    """(hub ids int32, count, largest non-hub in-degree) of the dst CSR when some node has more than
    MAX_FUSED_IN_DEGREE in-edges (hubs: every node with more than HUB_DEGREE), else None.  Cached on
    the layout (the host collate ships it); one sync otherwise."""
    if lay.hubs is None:
        hubs = False
        if lay.dst_ptr.numel() > 1 and _degree_range(lay)[0] > MAX_FUSED_IN_DEGREE:
            deg = lay.dst_ptr[1:] - lay.dst_ptr[:-1]
            is_hub = deg > HUB_DEGREE
            ids = torch.nonzero(is_hub).view(-1).to(torch.int32)
            rest = int(torch.where(is_hub, torch.zeros_like(deg), deg).max())
            hubs = (ids, ids.numel(), rest)
        lay.hubs = hubs
    return lay.hubs or None


def zero_rows_needed(lay: DeviceLayout, src: Tensor, V: int) -> tuple[bool, bool, bool]:
    """Which node-row outputs need a zero fill because no row of a plan writes them: (out, mid, bwd) =
    some node has in-degree 0 (the final node output: torch_scatter's empty segment is 0), some node
    has in-degree 0 and out-degree > 0 (an intermediate S row that a later S[src] gather reads), some
    node has out-degree 0 and in-degree > 0 (a dS row that the edge backward's dS[dst] reads).  Bond
    graphs have in-degree = out-degree, so only `out` can hold (isolated atoms).  Cached; the first
    call syncs once unless the in-degrees alone decide it."""
    def build():
        zf_out = V > 0 and _degree_range(lay)[1] == 0
        mid = bwd = False
        if zf_out or (V > 0 and src.numel() > 0):
            indeg = (lay.dst_ptr[1:] - lay.dst_ptr[:-1])
            outdeg = torch.bincount(src, minlength=V)[:V]
            t = torch.stack([((indeg == 0) & (outdeg > 0)).any(), ((outdeg == 0) & (indeg > 0)).any()]).cpu()
            mid, bwd = bool(t[0]), bool(t[1])
        return zf_out, mid, bwd

    return _cached(lay, "zero_rows", (src.data_ptr(), src.numel(), V), build)


def fused_plan(lay: DeviceLayout, V: int, E: int, rows: int = 64, dtype: torch.dtype = torch.float32):
    """Tile plan of the fused update for this layout with tiles of at most ``rows`` (64 or 128) rows,
    balanced to whole rounds over PLAN_NCU CUs, as (tile_ptr, ntiles, dst_sorted, zero_fill), cached on
    it.  Hub nodes (more than HUB_DEGREE in-edges, polymer graphs) are cut at the stride; the fp32
    layer leaves their aggregation to nt_dmpnn_hub_aggregate (None for bf16: those graphs take the
    unfused path).  One sync per layout."""
    hubs = hub_info(lay) if E > 0 and V > 0 else None
    if hubs is not None and dtype != torch.float32:
        return None
    hub, maxdeg = (HUB_DEGREE, hubs[2]) if hubs is not None else (0, None)
    if lay.plan is None:
        plan = False
        if E > 0 and V > 0:
            mx, mindeg = _degree_range(lay)
            tile_ptr, ntiles, dsts = K.tile_plan(lay.dst_ptr, E, mx if maxdeg is None else maxdeg, rows=64,
                                                 ncu=K.PLAN_SLOTS64, hub_degree=hub)
            plan = (tile_ptr, ntiles, dsts, mindeg == 0)
        lay.plan = plan
    if not lay.plan:
        return None
    if rows <= 64:
        return lay.plan
    if lay.plan_wide is None:  # node-aligned tiles of <= 128 rows, balanced over the CUs
        mx = _degree_range(lay)[0] if maxdeg is None else maxdeg
        tile_ptr, ntiles, _ = K.tile_plan(lay.dst_ptr, E, mx, rows=128, ncu=K.PLAN_NCU, hub_degree=hub)
        lay.plan_wide = (tile_ptr, ntiles)
    return lay.plan_wide[0], lay.plan_wide[1], lay.plan[2], lay.plan[3]


def fused_max_in_degree(lay: DeviceLayout) -> int:
    """The in-degree the fused kernel's segmented scan must cover: the largest non-hub in-degree."""
    hubs = hub_info(lay)
    return _degree_range(lay)[0] if hubs is None else hubs[2]


def dst_chunks(lay: DeviceLayout):
    """Chunk plan of the dst CSR when some node's in-degree exceeds LONG_SEGMENT (hubs), else None."""
    ch = getattr(lay, "dst_chunks", None)
    if ch is None:
        ch = False
        if lay.dst_ptr.numel() > 1 and _degree_range(lay)[0] > LONG_SEGMENT:
            ch = K.chunk_plan(lay.dst_ptr)
        lay.dst_chunks = ch
    return ch or None


def hub_chunk_ids(lay: DeviceLayout, chunks) -> Tensor:
    """The chunks of the dst chunk plan that belong to segments longer than MAX_FUSED_IN_DEGREE (the
    hubs' part of a hub graph's init), int32, cached on the layout with the plan; one sync."""
    def build():
        chunk_ptr = chunks[2].long()
        nch = chunk_ptr[1:] - chunk_ptr[:-1]
        deg = (lay.dst_ptr[1:] - lay.dst_ptr[:-1]).long()
        seg_of = torch.repeat_interleave(torch.arange(deg.numel(), device=deg.device), nch, output_size=chunks[1])
        return torch.nonzero(deg[seg_of] > MAX_FUSED_IN_DEGREE).flatten().to(torch.int32)

    return _cached(lay, "hub_chunk_ids", (), build, pin=chunks[0])


def row_table(lay: DeviceLayout, dsts: Tensor, src: Tensor, rev: Tensor, V: int) -> Tensor:
    """The fp32 layer kernel's row table of this graph (nt_dmpnn_row_table), cached on the layout
    (keyed on the src storage and the rev_index tensor, like backward_layout)."""
    return _cached(lay, "row_table", (src.data_ptr(), src.numel(), rev.data_ptr(), rev.numel(), V),
                   lambda: K.dmpnn_row_table(lay.dst_perm, dsts, src, rev, V), pin=rev)


def embed_records(lay: DeviceLayout, node_types: Tensor, nv: int, edge_types: Tensor, ne: int, src: Tensor) -> Tensor:
    """The graph's type records for the wave-per-node embedding init (kernels.embed_edge_records),
    cached on the layout, keyed on the type tensors (identity and version) and src."""
    key = (node_types.data_ptr(), node_types._version, edge_types.data_ptr(), edge_types._version,
           src.data_ptr(), src.numel(), nv, ne)
    return _cached(lay, "embed_records", key,
                   lambda: K.embed_edge_records(node_types, nv, edge_types, ne, src, lay.dst_perm))


def hub_run_table(lay: DeviceLayout, rt: Tensor, tile_ptr: Tensor, dsts: Tensor, run_rows: int) -> tuple:
    """The row table with hub sub-runs (kernels.hub_runs) for this plan's tiles, cached on the layout
    (keyed on the base table and the plan): (table, nslots, hubs, slot_ptr)."""
    return _cached(lay, "hub_runs", (rt.data_ptr(), tile_ptr.data_ptr(), tile_ptr.numel(), run_rows),
                   lambda: K.hub_runs(rt, lay.dst_ptr, dsts, tile_ptr, HUB_DEGREE, run_rows))


def dA_plan(lay: DeviceLayout, src: Tensor, V: int, E: int, src_ptr: Tensor, src_perm: Tensor):
    """The backward's fused dA + dS launch plan (fp32): node-aligned 64-row tiles over the src-sorted
    edge order (the transpose of the forward's dst plan) and its row table {edge, e, -1, src node}:
    A[e] = G[e] (the "src" row of the gather is the edge itself, nothing subtracted), so the layer
    kernel's fused mode computes dA = G W and dS[v] = sum_{e: src[e] = v} dA[e] in ascending edge order
    (the bits of segment_reduce(dA, src CSR)).  None when some node has more than
    MAX_FUSED_IN_DEGREE out-edges (then dense_matmul + segment_reduce).  Cached on the layout."""
    def build():
        if E <= 0 or V <= 0:
            return None
        outdeg = src_ptr[1:] - src_ptr[:-1]
        dmax, dmin = int(outdeg.max()), int(outdeg.min())
        if dmax > MAX_FUSED_IN_DEGREE:
            return None
        tile_ptr, ntiles, dsts = K.tile_plan(src_ptr, E, dmax, rows=64, ncu=K.PLAN_SLOTS64)
        ident = torch.arange(E, dtype=torch.int64, device=src.device)
        none = torch.full((E,), -1, dtype=torch.int64, device=src.device)
        # the gathered operand is G (E rows): the row table's bound on the "src" index is E
        rt = K.dmpnn_row_table(src_perm, dsts, ident, none, E)
        # dS rows no tile writes (out-degree 0) need zeros only if an edge's dS[dst] reads them
        zf = dmin == 0 and zero_rows_needed(lay, src, V)[2]
        return (tile_ptr, ntiles, dsts), dmax, zf, ident, none, rt

    return _cached(lay, "da_plan", (src.data_ptr(), src.numel(), V), build)


def backward_layout(lay: DeviceLayout, src: Tensor, rev: Tensor, V: int, E: int) -> tuple:
    """(src_ptr, src_perm, rev_ptr, rev_perm): the CSRs of the two gathers' transposes (scatter by
    src into nodes, scatter by rev_index into edges), built once per graph and cached on its layout."""
    # keyed on the storage (src is a fresh view of edge_index[0] on every call) and the rev tensor
    return _cached(lay, "bwd", (src.data_ptr(), src.numel(), rev.data_ptr(), rev.numel(), V),
                   lambda: (*K.csr_build(src, V, check_bounds=False), *K.csr_build(rev, E, check_bounds=False)),
                   pin=rev)


def mol_chunks(G, mol_ptr: Tensor):
    """Chunk plan of the molecule CSR when some molecule has more than LONG_SEGMENT atoms (polymers,
    config 5), else None; cached on the layout with the molecule CSR it belongs to."""
    def build():
        n = mol_ptr[1:] - mol_ptr[:-1]
        return K.chunk_plan(mol_ptr) if n.numel() and int(n.max()) > LONG_SEGMENT else False

    lay = getattr(G, "_nt_layout", None)
    ch = build() if lay is None else _cached(lay, "mol_chunks", (), build, pin=mol_ptr)
    return ch or None
