"""CPU checks of the topology generators (tests/topology.py): they deliver what the GPU tests of
tests/test_gpu_topology.py rely on.  Degree histograms, the three zero-row conditions of a directed
graph, rev_index in range, the collate in both rev modes equal to the reference restatement
(oracle/collate_ref.py) with the host plans shipped, the ladders' runs at the rows they are meant
for, and the gradient cases' fp32 floor (the oracle's own fp32 error against fp64)."""
import numpy as np
import pytest
import torch

import topology as T
from oracle import collate_ref


@pytest.mark.parametrize("name", T.BOND_GRAPHS)
def test_capped_bonds_degrees(name):
    top = T.block_graph(name)
    indeg, outdeg = top.in_degree(), top.out_degree()
    assert torch.equal(indeg, outdeg)  # bond graphs
    D = T.MAX_IN_DEGREE[name]
    assert int(indeg.max()) == D
    big = sorted(d for d in indeg.tolist() if d > 4)
    assert big == ([9, 10, 32, 33] if name == "b33mix" else [D])
    off = 0
    for G, rev in zip(top.graphs, top.rev_local):
        e = G.num_edges
        assert torch.equal(rev, torch.arange(e) ^ 1) and torch.equal(G.rev_index, rev)
        src, dst = G.edge_index
        assert torch.equal(src[0::2], dst[1::2]) and torch.equal(dst[0::2], src[1::2])  # edges 2b, 2b+1
        assert torch.equal(G.edge_feats[0::2], G.edge_feats[1::2])
        pairs = set(zip(src[0::2].tolist(), dst[0::2].tolist()))
        assert len(pairs) == e // 2 and all((v, u) not in pairs and u != v for u, v in pairs)
        deg = indeg[off:off + G.num_nodes]
        assert len(set(deg.tolist())) > 2, "degrees must be mixed inside a molecule"
        off += G.num_nodes


def test_directed_graph_conditions():
    from notorch_amd.nn.gnn import _engine

    rng = np.random.default_rng(0)
    want = rng.integers(0, 6, size=40)
    want[:3] = 0
    want[-3:] = [7, 0, 2]
    top = T.directed(want, seed=1)
    assert top.in_degree().tolist() == want.tolist()
    for top in (top, T.block_graph("dir")):
        indeg, outdeg = top.in_degree(), top.out_degree()
        half = top.V // 2
        assert int(top.edge_index[0].max()) < half
        assert ((indeg[:half] == 0) & (outdeg[:half] > 0)).any()
        assert ((indeg[half:] > 0) & (outdeg[half:] == 0)).any() and (indeg == 0).any()
        rev = top.rev_local[0]
        assert 0 <= int(rev.min()) and int(rev.max()) < top.E
        assert not torch.equal(rev, torch.arange(top.E) ^ 1)
        G = top.collate("edges")
        assert _engine.zero_rows_needed(G._nt_layout, G.edge_index[0].contiguous(), top.V) == (True, True, True)
    assert int(T.block_graph("dir").in_degree().max()) == T.MAX_IN_DEGREE["dir"]
    assert int(T.block_graph("dir").out_degree().max()) <= 32  # the backward's fused dA + dS plan applies


@pytest.mark.parametrize("name", T.BLOCK_GRAPHS + ("full",))
@pytest.mark.parametrize("rev_offset", ["nodes", "edges"])
def test_collate_matches_reference_and_ships_plans(name, rev_offset):
    from notorch_amd.data.models import graph as gm

    top = T.full_tile_graph() if name == "full" else T.block_graph(name)
    G = top.collate(rev_offset)
    ref = collate_ref.from_graphs(top.graphs, rev_offset)
    for key in ("node_feats", "edge_feats", "edge_index", "rev_index", "batch_node_index", "batch_edge_index"):
        assert torch.equal(getattr(G, key), ref[key]), key
    assert len(G) == ref["size"] == len(top.graphs)
    V, ei, rev, batch = top.raw(rev_offset)
    assert V == G.num_nodes and torch.equal(ei, G.edge_index) and torch.equal(rev, G.rev_index)
    assert torch.equal(batch, G.batch_node_index)
    assert 0 <= int(rev.min()) and int(rev.max()) < top.E

    lay = G._nt_layout
    indeg = top.in_degree()
    D = int(indeg.max())
    assert lay.validated and lay.deg_range == (D, int(indeg.min()))
    dst_ptr = lay.dst_ptr.numpy()
    assert np.array_equal(np.diff(dst_ptr), indeg.numpy())
    assert torch.equal(ei[1][lay.dst_perm.long()], torch.repeat_interleave(torch.arange(V), indeg))
    if D > gm.MAX_FUSED_IN_DEGREE:
        ids, nhub, rest = lay.hubs
        assert ids.tolist() == torch.nonzero(indeg > gm.HUB_CUT_DEGREE).flatten().tolist() and nhub == len(ids)
        assert rest == int(indeg[indeg <= gm.HUB_CUT_DEGREE].max())
        plan_deg, hub = rest, gm.HUB_CUT_DEGREE
    else:
        assert lay.hubs is False
        plan_deg, hub = D, 0
    assert (lay.dst_chunks is not False) == (D > gm.LONG_SEGMENT)
    for rows, (tile_ptr, ntiles) in ((64, lay.plan[:2]), (128, lay.plan_wide)):
        want, n, _ = gm.host_tile_plan(dst_ptr, top.E, plan_deg, rows=rows, ncu=gm.PLAN_NCU, hub_degree=hub)
        sizes = np.diff(tile_ptr.numpy())
        assert n == ntiles and torch.equal(tile_ptr, want) and sizes.min() >= 0 and sizes.max() <= rows
    assert torch.equal(lay.plan[2].long(), torch.repeat_interleave(torch.arange(V), indeg))
    assert lay.plan[3] == bool((indeg == 0).any())


def test_full_tile_graph_fills_the_engine_tiles():
    """The 64-row and 128-row plans the collate ships for the large batch hold tiles close to the
    kernels' capacity (small graphs never do: the plans balance over 256 slots)."""
    top = T.full_tile_graph()
    assert int(top.in_degree().max()) == 32 and 24_000 <= top.E <= 256 * 97
    lay = top.collate("nodes")._nt_layout
    assert np.diff(lay.plan[0].numpy()).max() > 48
    assert np.diff(lay.plan_wide[0].numpy()).max() > 96


@pytest.mark.parametrize("rows", [64, 128])
@pytest.mark.parametrize("D", [4, 5, 9, 10, 17, 32])
def test_ladder_places_the_runs(D, rows):
    from notorch_amd.data.models import graph as gm

    degs = T.ladder_degs(D, rows)
    top = T.ladder(degs, seed=D)
    assert top.in_degree().tolist() == degs and max(degs) == D and degs.count(0) >= 4
    assert top.E < 3000
    G = top.collate("edges")
    lay = G._nt_layout
    assert np.array_equal(np.diff(lay.dst_ptr.numpy()), degs)
    assert not torch.equal(lay.dst_perm.long(), torch.arange(top.E))  # edge ids are shuffled
    sizes, runs, rounds = T.ladder_rows(degs, D, rows)
    tile_ptr, ntiles, _ = gm.host_tile_plan(lay.dst_ptr.numpy(), top.E, D, rows=rows, ncu=0)
    assert np.array_equal(np.diff(tile_ptr.numpy()), sizes) and sizes.max() <= rows
    # the worst case of the scan instance that serves D: min(D - 1, 16) rounds, not one fewer
    assert rounds == min(D - 1, 16)
    assert (1, D) in runs and (0, D) in runs
    if D == 32:
        assert sizes.max() == rows  # [32, 32] (or four of them) fill a tile exactly
        pairs = set(zip(runs, runs[1:]))
        for a, b in (((0, 15), (15, 17)), ((0, 16), (16, 16)), ((1, 31), (32, 32)), ((0, 15), (15, 32))):
            assert (a, b) in pairs
    if D >= 17:
        mixed = {d for _, d in runs}
        assert {1, 4, 5, 9, 10, 16, 17} <= mixed


@pytest.mark.parametrize("case", T.GRAD_CASES, ids=lambda c: "-".join(map(str, c)))
def test_gradient_cases_fp32_floor(case):
    """Every gradient case of the GPU tests: the fp32 oracle's own error against fp64 stays below
    GRAD_FLOOR_MAX, so 4 x floor never widens GRAD_TOL; and no true gradient is degenerate (a regular
    graph's mean-reduce dW is identically zero, and a normalised error against it means nothing)."""
    name, h, act, reduce = case
    top, G, raw, Xv, Xe, blk = T.grad_case(name, h, act, reduce)
    truth, floor = T.oracle_floor(raw, len(top.graphs), Xv, Xe, blk, act, reduce)
    print(f"{case}: fp32 oracle vs fp64 {floor:.2e}")
    assert floor <= T.GRAD_FLOOR_MAX and 4 * floor <= T.GRAD_TOL
    for nm, g in zip(T.grad_names(T.GRAD_DEPTH), truth):
        assert torch.isfinite(g).all() and g.abs().max() > 1e-6 * max(1.0, truth[0].abs().item() ** 0.5), nm
