"""GPU: the layer kernels on in-degrees 5..65 and on directed graphs (graphs of tests/topology.py; the
molecule generators stop at in-degree 4 plus hubs cut into sub-runs of <= 9 rows, always with in-degree
= out-degree).

(a) the fp32 layer kernel, one launch on largest-tile plans: every scan instance (3 / 8 / 16 rounds) on
    the run that needs all of its rounds, runs that end / start on a row-tile edge, tiles filled exactly,
    every walk (two-workgroup 64-row, 128-row, narrow 64-row variants, column chunks).  H' against the
    fp64 layer at FP32_NORM_TOL; S' bit-identical to the CPU scatter of the kernel's own H'.
(b) the bf16 fused layer on the same ladders: S' = the CPU reduce of the stored H', rounded once.
(c) nt_dmpnn_init (wave and thread forms) on in-degrees 6..33, with and without skip_degree.
(d) ChempropBlock through the engine across the dispatch thresholds (in-degree 9/10, 32/33, 64/65, hub
    graphs with nodes at 9 / 10 / 32), on a directed graph, and on one batch large enough for full tiles.
(e) the kernel backward against fp64 oracle autograd: out-degree 32 / 33 (the fused dA + dS plan and
    its fallback), the directed graph (the dS zero fill).
(f) the collate's host plans equal the device planners'.

Every test prints its achieved error as a line ``TOPOERR <class> <value> <case>``."""
import functools

import pytest
import torch
import torch.nn as nn

import topology as T
from helpers import FP32_NORM_TOL, assert_parity, norm_err
from oracle import dmpnn_ref
from test_gpu_fk import _ref_layer

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
DEGREES = (4, 5, 9, 10, 17, 32)


def _K():
    from notorch_amd import kernels

    return kernels


def _report(cls, err, case):
    print(f"TOPOERR {cls} {err:.3e} {case}")


def _last_kernel():
    from notorch_amd import _lib

    return _lib.load().nt_last_kernel().decode()


@functools.lru_cache(maxsize=None)
def _ladder(D, rows):
    degs = T.ladder_degs(D, rows)
    top = T.ladder(degs, seed=D)
    return degs, top, top.collate("edges")


_ACT = {"relu": (nn.ReLU(), torch.relu), "identity": (nn.Identity(), lambda x: x),
        "silu": (nn.SiLU(), torch.nn.functional.silu)}
_WALK = {"nw4": (64, "two 4-wave workgroups per CU, 64-row tiles"),
         "wide": (128, "one 8-wave workgroup per CU, 128-row tiles"),
         "narrow": (64, "one 8-wave workgroup per CU, 64-row tiles")}


def _layer_cases():
    cases = []
    for D in DEGREES:  # relu / sum layers: the two-workgroup 64-row walk and the 128-row walk
        for walk in ("nw4", "wide"):
            cases += [(walk, 300, D, "relu", "sum", "relu"), (walk, 36, D, "relu", "sum", "identity")]
    cases += [("nw4", 64, 32, "relu", "sum", "relu"), ("wide", 64, 32, "relu", "sum", "identity")]
    for D in (5, 32):  # the narrow 64-row variants (always the 16-round scan)
        for h in (36, 300):
            cases += [("narrow", h, D, "silu", "sum", "relu"), ("narrow", h, D, "silu", "sum", "identity"),
                      ("narrow", h, D, "relu", "mean", "relu"), ("narrow", h, D, "relu", "max", "relu"),
                      ("narrow", h, D, "relu", "min", "identity")]
    # h = 640: the column-chunked path
    cases += [("narrow", 640, 32, "relu", "sum", "relu"), ("narrow", 640, 17, "relu", "mean", "relu"),
              ("narrow", 640, 10, "relu", "sum", "identity")]
    return cases


@pytest.mark.parametrize("walk,h,D,act,reduce,agg", _layer_cases())
def test_layer_kernel_on_ladders(walk, h, D, act, reduce, agg):
    """One launch of nt_dmpnn_update_fused over the ladder of max in-degree D, passed exactly as
    max_in_degree (so D = 4 / 5..9 / 10.. select the 3 / 8 / 16-round scan of the relu / sum walks)."""
    K = _K()
    rows, kernel = _WALK[walk]
    degs, top, G = _ladder(D, rows)
    E, V = top.E, top.V
    dst = G.edge_index[1]
    dst_ptr, perm = K.csr_build(dst.to(DEV), V)
    plan = K.tile_plan(dst_ptr, E, D, rows=rows, ncu=0)
    sizes = T.ladder_rows(degs, D, rows)[0]
    assert (plan[0][1:] - plan[0][:-1]).cpu().tolist() == sizes.tolist()
    g = torch.Generator().manual_seed(1000 * D + h)
    H, S = torch.randn(E, h, generator=g), torch.randn(V, h, generator=g)
    W = torch.randn(h, h, generator=g) / h ** 0.5
    residual = reduce != "mean"
    b = torch.randn(h, generator=g) if residual else None
    act_mod, act_fn = _ACT[act]
    agg_mod, agg_fn = _ACT[agg]
    assert K.fused_tile_rows(h, torch.float32, K.act_code(act_mod), reduce, K.act_code(agg_mod)) >= rows
    amax_out = torch.zeros(2, device=DEV)
    Hn, Sn = K.dmpnn_update_fused(
        H.to(DEV), S.to(DEV), G.edge_index[0].to(DEV), G.rev_index.to(DEV), K.pack_weights(W.to(DEV)),
        None if b is None else b.to(DEV), residual=residual, act=K.act_code(act_mod), plan=plan, tile_rows=rows,
        max_in_degree=D, perm=perm, reduce=reduce, agg_act=K.act_code(agg_mod), zero_fill=True, amax_out=amax_out,
    )
    assert kernel in _last_kernel(), _last_kernel()
    rH, rS = _ref_layer(G, H, S, W, b, residual, act_fn, agg_fn, reduce)
    case = f"{walk} h={h} D={D} {act} {reduce} {agg}"
    _report("layer_fp32_H", norm_err(Hn, rH), case)
    _report("layer_fp32_S", norm_err(Sn, rS), case)
    assert_parity(Hn, rH, FP32_NORM_TOL, f"H {case}")
    assert_parity(Sn, rS, FP32_NORM_TOL, f"S {case}")
    # the bit-exact contract: S' is the CPU scatter (ascending edge id) of the kernel's own H'
    exact = dmpnn_ref.scatter(agg_fn(Hn.cpu()), dst, V, reduce)
    bad = torch.nonzero((Sn.cpu() != exact).any(1)).flatten().tolist()
    assert not bad, f"{case}: S' rows differ from the scatter of H' at nodes {bad[:8]} (in-degrees " \
                    f"{[degs[v] for v in bad[:8]]})"
    assert amax_out[0].item() == Hn.abs().max().item()
    assert amax_out[1].item() == Sn.abs().max().item()


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("h", [64, 200])
@pytest.mark.parametrize("D", DEGREES)
def test_bf16_fused_layer_on_ladders(D, h, reduce):
    """The bf16 fused layer on the ladders: H' within one bf16 ulp of the fp32 evaluation (the message
    rounded to bf16 as the kernel's MFMA operand), S' = the CPU reduce of the stored H', rounded once."""
    K = _K()
    degs, top, G = _ladder(D, 64)
    E, V = top.E, top.V
    src, dst, rev = G.edge_index[0], G.edge_index[1], G.rev_index
    dst_ptr, perm = K.csr_build(dst.to(DEV), V)
    plan = K.tile_plan(dst_ptr, E, D, rows=64, ncu=0)
    g = torch.Generator().manual_seed(77 * D + h)
    H, S = torch.randn(E, h, generator=g).to(BF), torch.randn(V, h, generator=g).to(BF)
    W = (torch.randn(h, h, generator=g) / h ** 0.5).to(BF)
    b = torch.randn(h, generator=g).to(BF)
    relu = K.act_code(nn.ReLU())
    Hn, Sn = K.dmpnn_update_fused(H.to(DEV), S.to(DEV), src.to(DEV), rev.to(DEV), K.pack_weights(W.to(DEV)),
                                  b.to(DEV), residual=True, act=relu, plan=plan, tile_rows=64, max_in_degree=D,
                                  perm=perm, reduce=reduce, agg_act=relu, zero_fill=True)
    assert Hn.dtype == BF and Sn.dtype == BF
    A = (S.float()[src] - torch.relu(H.float()[rev])).to(BF).float()
    ref = H.float() + A @ W.float().T + b.float()
    _report("layer_bf16_H", norm_err(Hn.float(), ref), f"h={h} D={D} {reduce}")
    assert_parity(Hn.float(), ref, 2.0 ** -8, f"bf16 H h={h} D={D}")
    exact = dmpnn_ref.scatter(torch.relu(Hn.float().cpu()), dst, V, reduce).to(BF)
    bad = torch.nonzero((Sn.cpu() != exact).any(1)).flatten().tolist()
    assert not bad, f"bf16 {reduce} h={h} D={D}: S' rows differ at nodes {bad[:8]} (in-degrees " \
                    f"{[degs[v] for v in bad[:8]]})"


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("h,skip", [(300, 0), (300, 32), (128, 32), (600, 0), (64, 0), (36, 0)])
def test_init_on_degrees_6_to_33(h, skip, reduce):
    """nt_dmpnn_init with the aggregation on in-degrees 6..33 (and 0): the wave-per-node form (h >= 128,
    one or two column passes) and the thread form (h < 128).  H0 and S bit-identical to the CPU
    evaluation in the same order.  skip_degree = 32 (the hub graphs' init) leaves the in-degree-33 nodes
    to the chunked init over their chunks, which completes H0 and S."""
    from notorch_amd.data.models.graph import DeviceLayout
    from notorch_amd.nn.gnn import _engine

    K = _K()
    degs = []
    for d in range(6, 34):
        degs += [d, 0] if d % 5 == 0 else [d]
    degs = [0, 33] + degs + [33, 0, 0]
    top = T.ladder(degs, seed=h + skip)
    E, V = top.E, top.V
    src, dst = top.edge_index
    g = torch.Generator().manual_seed(h + len(reduce))
    Xv, Xe = torch.randn(V, h, generator=g), torch.randn(E, h, generator=g)
    dst_ptr, perm = K.csr_build(dst.to(DEV), V)
    relu = K.act_code(nn.ReLU())
    am = torch.zeros(2, device=DEV)
    H0, S = K.dmpnn_init(Xv.to(DEV), Xe.to(DEV), src.to(DEV), dst_ptr, perm, act=relu, reduce=reduce, amax=am,
                         skip_degree=skip)
    rH = Xv[src] + Xe
    rS = dmpnn_ref.scatter(torch.relu(rH), dst, V, reduce)
    indeg = torch.tensor(degs)
    if skip:
        kept = indeg <= skip
        assert torch.equal(H0.cpu()[kept[dst]], rH[kept[dst]])
        assert torch.equal(S.cpu()[kept], rS[kept])
        lay = DeviceLayout(dst_ptr, perm)
        chunks = K.chunk_plan(dst_ptr)
        ids = _engine.hub_chunk_ids(lay, chunks)
        assert ids.numel() == 2 * int((~kept).sum())  # 33 in-edges: a chunk of 32 and a chunk of 1
        K.dmpnn_init_chunked(Xv.to(DEV), Xe.to(DEV), src.to(DEV), dst_ptr, perm, chunks, act=relu, reduce=reduce,
                             amax=am, H0=H0, S=S, chunk_ids=ids)
        assert_parity(S, rS.double(), FP32_NORM_TOL, "S after the chunked init")
        assert torch.equal(S.cpu()[kept], rS[kept])
    else:
        assert torch.equal(S.cpu(), rS)
    assert torch.equal(H0.cpu(), rH)
    assert am[0].item() == rH.abs().max().item()
    assert am[1].item() == S.abs().max().item()


# ------------------------------------------------------------------------------------ (d) blocks
@functools.lru_cache(maxsize=None)
def _block_graph(name, rev_offset):
    top = T.full_tile_graph() if name == "full" else T.block_graph(name)
    return top, top.collate(rev_offset)


def _forward_truth(top, G, rev_offset, Xv, Xe, blk, act, reduce, dtype=torch.float64, masks=None, residual=True):
    V, ei, rev, batch = top.raw(rev_offset)
    Ws, bs = dmpnn_ref.block_params(blk)
    with torch.no_grad():
        return dmpnn_ref.chemprop_block(Xv.to(dtype), Xe.to(dtype), ei, rev, [W.to(dtype) for W in Ws],
                                        [None if b is None else b.to(dtype) for b in bs], act=T.ACTS[act][1],
                                        residual=residual, reduce=reduce, dropout_masks=masks)


def _block_fp32(name, rev_offset, h, act, reduce, monkeypatch, walk128=False):
    from notorch_amd.nn.gnn import _engine

    top, G = _block_graph(name, rev_offset)
    Xv, Xe = T.embed(G.node_feats, G.edge_feats, h)
    blk = T.make_block(h, 3, act, reduce).eval()
    ref_n, ref_e = _forward_truth(top, G, rev_offset, Xv, Xe, blk, act, reduce)
    if walk128:
        monkeypatch.setattr(_engine, "NW4_MAX_EDGES", 0)
    blk = blk.to(DEV)
    Gd = G.update(node_feats=Xv, edge_feats=Xe).to(DEV)
    with torch.no_grad():
        out = blk(Gd)
        info = dict(_engine.LAST_UPDATE_INFO)
        again = blk(Gd)
        plan = _engine.fused_plan(Gd._nt_layout, top.V, top.E, 64, torch.float32)
        monkeypatch.setenv("NT_FUSED", "0")
        unfused = blk(Gd)
        info0 = dict(_engine.LAST_UPDATE_INFO)
    case = f"{name} {rev_offset} h={h} {act} {reduce}"
    assert plan is not None, "every graph here has a fused fp32 plan (hubs are cut into sub-runs)"
    assert info["fused"] and not info0["fused"], (info, info0)
    assert torch.equal(out.edge_feats, again.edge_feats) and torch.equal(out.node_feats, again.node_feats)
    for what, o in (("fused", out), ("unfused", unfused)):
        _report("block_fp32_edge", norm_err(o.edge_feats, ref_e), f"{what} {case}")
        _report("block_fp32_node", norm_err(o.node_feats, ref_n), f"{what} {case}")
        assert_parity(o.edge_feats, ref_e, FP32_NORM_TOL, f"edge {what} {case}")
        assert_parity(o.node_feats, ref_n, FP32_NORM_TOL, f"node {what} {case}")
    return info, Gd


_FP32_SETTINGS = [(64, "ReLU", "sum"), (300, "ReLU", "sum"), (300, "SiLU", "mean"), (64, "ReLU", "max"),
                  (300, "ReLU", "mean"), (64, "SiLU", "sum")]


@pytest.mark.parametrize("h,act,reduce", _FP32_SETTINGS)
@pytest.mark.parametrize("rev_offset", ["nodes", "edges"])
@pytest.mark.parametrize("name", T.BOND_GRAPHS)
def test_block_fp32_across_thresholds(name, rev_offset, h, act, reduce, monkeypatch):
    """Depth-3 blocks on bond graphs of max in-degree 9 / 10 (scan instances), 32 / 33 (node-aligned
    tiles against the hub plan, the wave init's skip_degree), 33 with nodes at 9 / 10 / 32 (HUB_DEGREE
    inside a hub graph) and 64 / 65 (the chunked reduce of the unfused path): fused and NT_FUSED=0
    against the fp64 oracle, the fused path taken, two forwards bit-identical."""
    _block_fp32(name, rev_offset, h, act, reduce, monkeypatch)


@pytest.mark.parametrize("h,act,reduce", _FP32_SETTINGS)
def test_block_fp32_directed(h, act, reduce, monkeypatch):
    """The directed graph: intermediate S rows of in-degree-0 source nodes are read by later layers from
    buffers reused across layers (the `mid` zero fill of zero_rows_needed)."""
    from notorch_amd.nn.gnn import _engine

    _, Gd = _block_fp32("dir", "edges", h, act, reduce, monkeypatch)
    assert _engine.zero_rows_needed(Gd._nt_layout, Gd.edge_index[0].contiguous(), Gd.num_nodes) == (True, True, True)


@pytest.mark.parametrize("walk128,h,act,reduce", [(False, 64, "ReLU", "sum"), (True, 64, "ReLU", "sum"),
                                                  (False, 64, "ReLU", "mean")])
def test_block_fp32_full_tiles(walk128, h, act, reduce, monkeypatch):
    """One batch of ~24.6k edges at max in-degree 32: the engine's balanced plans reach the kernels'
    tile capacity (64-row walk, 128-row walk, narrow variant)."""
    from notorch_amd.nn.gnn import _engine

    info, Gd = _block_fp32("full", "nodes", h, act, reduce, monkeypatch, walk128)
    lay = Gd._nt_layout
    t64 = _engine.fused_plan(lay, Gd.num_nodes, Gd.num_edges, 64)[0]
    t128 = _engine.fused_plan(lay, Gd.num_nodes, Gd.num_edges, 128)[0]
    assert int((t64[1:] - t64[:-1]).max()) > 48 and int((t128[1:] - t128[:-1]).max()) > 96
    assert info["rows"] == (128 if walk128 else 64)


@pytest.mark.parametrize("reduce,act", [("sum", "ReLU"), ("mean", "SiLU"), ("max", "ReLU")])
@pytest.mark.parametrize("name", T.BLOCK_GRAPHS + ("full",))
def test_block_bf16(name, reduce, act, monkeypatch):
    """bf16 storage at h = 64, depth 3: the block criterion of tests/test_gpu_bf16.py (normalised max
    error <= 2e-2 against the fp32 oracle on the bf16-valued inputs); the fused path wherever the graph
    has a plan (bf16 hub graphs take the unfused path), bit-identical to NT_FUSED=0 there; two forwards
    bit-identical."""
    from notorch_amd.nn.gnn import _engine

    h = 64
    rev_offset = "edges" if name in ("dir", "b10", "b33") else "nodes"
    top, G = _block_graph(name, rev_offset)
    Xv, Xe = (x.to(BF) for x in T.embed(G.node_feats, G.edge_feats, h))
    blk = T.make_block(h, 3, act, reduce).eval().to(BF)
    ref_n, ref_e = _forward_truth(top, G, rev_offset, Xv, Xe, blk, act, reduce, torch.float32)
    blk = blk.to(DEV)
    Gd = G.update(node_feats=Xv, edge_feats=Xe).to(DEV)
    with torch.no_grad():
        out = blk(Gd)
        fused = _engine.LAST_UPDATE_INFO["fused"]
        again = blk(Gd)
        plan = _engine.fused_plan(Gd._nt_layout, top.V, top.E, 64, BF)
        monkeypatch.setenv("NT_FUSED", "0")
        unfused = blk(Gd)
    assert (plan is not None) == (T.MAX_IN_DEGREE.get(name, 32) <= 32) and fused == (plan is not None)
    assert torch.equal(out.edge_feats, again.edge_feats) and torch.equal(out.node_feats, again.node_feats)
    if fused:
        assert torch.equal(out.edge_feats, unfused.edge_feats) and torch.equal(out.node_feats, unfused.node_feats)
    for what, o in (("fused" if fused else "plain", out), ("unfused", unfused)):
        assert o.edge_feats.dtype == BF
        _report("block_bf16", max(norm_err(o.edge_feats.float(), ref_e), norm_err(o.node_feats.float(), ref_n)),
                f"{what} {name} {act} {reduce}")
        assert_parity(o.edge_feats.float(), ref_e, 2e-2, f"bf16 edge {what} {name}")
        assert_parity(o.node_feats.float(), ref_n, 2e-2, f"bf16 node {what} {name}")


def test_block_dropout_on_in_degree_32():
    """Training-mode dropout (the unfused update + nt_dropout_residual) on the max-in-degree-32 graph:
    forward and gradients against the fp64 oracle with the same masks (tests/test_gpu_dropout.py)."""
    from notorch_amd.nn.gnn import _engine

    K = _K()
    h, depth, p = 48, 3, 0.25
    top, G = _block_graph("b32", "nodes")
    Xv, Xe = T.embed(G.node_feats, G.edge_feats, h)
    blk = T.make_block(h, depth, "ReLU", "sum", w_var=1 / 16, dropout=p).to(DEV).train()
    torch.manual_seed(99)
    seed = _engine.draw_dropout_seed()
    ones = torch.ones(top.E, h, device=DEV)
    masks = [K.dropout_residual(ones, p, seed, _engine.dropout_offset(l, top.E, h)).double().cpu()
             for l in range(depth)]
    torch.manual_seed(99)  # the block draws the same seed
    Xv_d, Xe_d = Xv.to(DEV).requires_grad_(True), Xe.to(DEV).requires_grad_(True)
    out = blk(G.update(node_feats=Xv_d, edge_feats=Xe_d).to(DEV))
    wts = torch.linspace(-1, 1, h, device=DEV)
    (out.node_feats.pow(2).sum() + (out.edge_feats * wts).sum()).backward()
    V, ei, rev, _ = top.raw("nodes")
    Ws, bs = dmpnn_ref.block_params(blk)
    Ws = [W.double().requires_grad_(True) for W in Ws]
    bs = [b.double().requires_grad_(True) for b in bs]
    Xv_r, Xe_r = Xv.double().requires_grad_(True), Xe.double().requires_grad_(True)
    n_r, e_r = dmpnn_ref.chemprop_block(Xv_r, Xe_r, ei, rev, Ws, bs, dropout_masks=masks)
    (n_r.pow(2).sum() + (e_r * wts.double().cpu()).sum()).backward()
    pairs = [("node", out.node_feats, n_r), ("edge", out.edge_feats, e_r), ("dXv", Xv_d.grad, Xv_r.grad),
             ("dXe", Xe_d.grad, Xe_r.grad)]
    for l, layer in enumerate(blk._chemprop_layers()):
        pairs += [(f"dW[{l}]", layer.linear.weight.grad, Ws[l].grad), (f"db[{l}]", layer.linear.bias.grad, bs[l].grad)]
    for what, a, b in pairs:
        _report("dropout", norm_err(a, b), what)
        assert_parity(a, b, 1e-5, what)


def test_embedded_block_on_in_degree_32():
    """EmbeddedChempropBlock (GraphEmbedding fused into the initial gather) on the max-in-degree-32
    graph: bit-identical to the embedding kernel followed by the block, and against the oracle."""
    from notorch_amd.nn import ChempropBlock, EmbeddedChempropBlock, GraphEmbedding

    h = 300
    top, G = _block_graph("b32", "nodes")
    torch.manual_seed(3)
    emb = GraphEmbedding(42, 13, h)
    blk = ChempropBlock(hidden_dim=h, depth=3)
    fused = EmbeddedChempropBlock(emb, blk).eval()
    with torch.no_grad():
        e = emb(G)
        Xv, Xe = e.node_feats, e.edge_feats  # CPU reference embedding
    ref_n, ref_e = _forward_truth(top, G, "nodes", Xv, Xe, blk, "ReLU", "sum")
    fused = fused.to(DEV)
    Gd = G.update().to(DEV)  # a copy: the cached host graph stays on the host
    with torch.no_grad():
        out = fused(Gd)
        unfused = blk(emb(Gd))
    assert torch.equal(out.node_feats, unfused.node_feats) and torch.equal(out.edge_feats, unfused.edge_feats)
    _report("block_fp32_edge", norm_err(out.edge_feats, ref_e), "embedded b32")
    _report("block_fp32_node", norm_err(out.node_feats, ref_n), "embedded b32")
    assert_parity(out.node_feats, ref_n, FP32_NORM_TOL, "node")
    assert_parity(out.edge_feats, ref_e, FP32_NORM_TOL, "edge")


# ------------------------------------------------------------------------------------ (e) backward
def _device_grads(G, Xv, Xe, blk, reduce):
    from notorch_amd.nn import Mean, Sum

    for p in blk.parameters():
        p.grad = None
    Xv_d = Xv.to(DEV).requires_grad_(True)
    Xe_d = Xe.to(DEV).requires_grad_(True)
    out = blk(G.update(node_feats=Xv_d, edge_feats=Xe_d).to(DEV))
    ro = {"sum": Sum, "mean": Mean}[T.readout_of(reduce)]()(out)
    e = out.edge_feats.float()
    loss = ro.float().pow(2).sum() + (e * torch.linspace(-1, 1, e.shape[1], device=DEV)).sum()
    loss.backward()
    layers = blk._chemprop_layers()
    return ([loss.detach(), Xv_d.grad, Xe_d.grad] + [l.linear.weight.grad.clone() for l in layers]
            + [l.linear.bias.grad.clone() for l in layers])


def _da_plan(Gd):
    from notorch_amd.nn.gnn import _engine

    lay = _engine.dst_layout(Gd)
    src, rev = Gd.edge_index[0].contiguous(), Gd.rev_index.contiguous()
    V, E = Gd.num_nodes, Gd.num_edges
    src_ptr, src_perm = _engine.backward_layout(lay, src, rev, V, E)[:2]
    return _engine.dA_plan(lay, src, V, E, src_ptr, src_perm)


@pytest.mark.parametrize("case", T.GRAD_CASES, ids=lambda c: "-".join(map(str, c)))
def test_block_gradients(case, monkeypatch):
    """Kernel forward + kernel backward against fp64 oracle autograd (tests/test_gpu_backward.py's
    recipe, tol = max(GRAD_TOL, 4 x the fp32 oracle's own error), which tests/test_topology.py shows
    never widens GRAD_TOL here).  Out-degree <= 32 (b10, b32, dir): the fused dA + dS launch, never
    dense_matmul; out-degree 33 / 65: no plan.  dir: the dS zero fill (nodes with in-edges and no
    out-edge).  Two backward passes are bit-identical."""
    from notorch_amd.nn.gnn import _engine

    K = _K()
    name, h, act, reduce = case
    top, G, raw, Xv, Xe, blk = T.grad_case(name, h, act, reduce)
    truth, floor = T.oracle_floor(raw, len(top.graphs), Xv, Xe, blk, act, reduce)
    tol = max(T.GRAD_TOL, 4 * floor)
    assert tol == T.GRAD_TOL
    blk = blk.to(DEV).train()
    plan = _da_plan(G.update().to(DEV))
    if int(top.out_degree().max()) <= 32:
        assert plan is not None

        def boom(*a, **k):
            raise AssertionError("out-degree <= 32: dA and dS come from the fused launch")

        monkeypatch.setattr(K, "dense_matmul", boom)
        if name == "dir":
            assert plan[2], "dS rows of nodes without out-edges are read: the plan must zero-fill"
    else:
        assert plan is None
    got = _device_grads(G, Xv, Xe, blk, reduce)
    again = _device_grads(G, Xv, Xe, blk, reduce)
    for nm, a, b, t in zip(T.grad_names(T.GRAD_DEPTH), got, again, truth):
        assert torch.equal(a, b), f"{nm}: two backward passes differ"
        _report("grad_fp32", norm_err(a, t), f"{nm} {case} floor={floor:.2e}")
    for nm, a, t in zip(T.grad_names(T.GRAD_DEPTH), got, truth):
        assert_parity(a, t, tol, f"{nm} {case}")


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("name,act", [("b32", "SiLU"), ("dir", "ReLU")])
def test_block_gradients_bf16(name, act, monkeypatch):
    """bf16 kernel backward on in-degree 32 / the directed graph under the criterion of
    tests/test_gpu_bf16_backward.py: no further from the fp64 oracle than 2 x the torch-op bf16
    recompute (NT_BWD=torch) or the 2e-2 floor, on the normalised max and the relative L2 error."""
    h, reduce = 64, "sum"
    top, G, raw, Xv, Xe, blk = T.grad_case(name, h, act, reduce)
    Xv, Xe = Xv.to(BF), Xe.to(BF)
    blk = blk.to(DEV, BF).train()
    truth = T.oracle_grads(raw, len(top.graphs), Xv, Xe, blk, act, reduce, torch.float64)
    monkeypatch.setenv("NT_BWD", "kernel")
    got = _device_grads(G, Xv, Xe, blk, reduce)
    monkeypatch.setenv("NT_BWD", "torch")
    ref = _device_grads(G, Xv, Xe, blk, reduce)
    for nm, a, r, t in list(zip(T.grad_names(T.GRAD_DEPTH), got, ref, truth))[1:]:
        assert a.dtype == BF and torch.isfinite(a.float()).all(), nm
        e_max, r_max = norm_err(a.float(), t), norm_err(r.float(), t)
        e_l2, r_l2 = _rel_l2(a, t), _rel_l2(r, t)
        _report("grad_bf16", e_max, f"{nm} {name} {act} (torch bf16 {r_max:.2e}; L2 {e_l2:.2e} vs {r_l2:.2e})")
        assert e_max <= max(2e-2, 2.0 * r_max), f"{nm}: max {e_max:.3e} vs torch bf16 {r_max:.3e}"
        assert e_l2 <= max(2e-2, 2.0 * r_l2), f"{nm}: L2 {e_l2:.3e} vs torch bf16 {r_l2:.3e}"


# ------------------------------------------------------------------------------------ (f) plans
@pytest.mark.parametrize("name", T.BLOCK_GRAPHS + ("full",))
def test_device_planners_match_the_collate(name):
    """The layout the collate ships (degree range, hubs, tile plans, chunk plan) equals what the device
    planners build from the dst CSR alone; integers, bit for bit."""
    from notorch_amd.data.models.graph import DeviceLayout
    from notorch_amd.nn.gnn import _engine

    K = _K()
    top, G = _block_graph(name, "nodes")
    lay = G._nt_layout
    V, E = top.V, top.E
    dst_ptr, perm = K.csr_build(G.edge_index[1].to(DEV), V)
    assert torch.equal(dst_ptr.cpu(), lay.dst_ptr) and torch.equal(perm.cpu(), lay.dst_perm)
    d = DeviceLayout(dst_ptr, perm)
    assert _engine._degree_range(d) == lay.deg_range
    hubs = _engine.hub_info(d)
    if lay.hubs:
        assert torch.equal(hubs[0].cpu(), lay.hubs[0]) and hubs[1:] == lay.hubs[1:]
        assert hubs[2] <= _engine.HUB_DEGREE
    else:
        assert hubs is None and lay.deg_range[0] <= _engine.MAX_FUSED_IN_DEGREE
    for rows, shipped in ((64, lay.plan[:2]), (128, lay.plan_wide)):
        tp, n, dsts, zf = _engine.fused_plan(d, V, E, rows)
        assert n == shipped[1] and torch.equal(tp.cpu(), shipped[0])
        assert torch.equal(dsts.cpu(), lay.plan[2]) and zf == lay.plan[3]
    assert _engine.fused_max_in_degree(d) == (lay.hubs[2] if lay.hubs else lay.deg_range[0])
    chunks = _engine.dst_chunks(d)
    if lay.dst_chunks:
        assert lay.deg_range[0] > _engine.LONG_SEGMENT and chunks[1] == lay.dst_chunks[1]
        for a, b in zip(chunks, lay.dst_chunks):
            if isinstance(a, torch.Tensor):
                assert torch.equal(a.cpu(), b)
    else:
        assert chunks is None and lay.deg_range[0] <= _engine.LONG_SEGMENT
