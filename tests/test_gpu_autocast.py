"""ChempropBlock / EmbeddedChempropBlock with fp32 parameters under torch.autocast(dtype=bfloat16): the
block is one lower-precision autocast op on the bf16 kernels.

The yardstick for bf16 behaviour is code that exists without the feature: a copy.deepcopy of the
block moved .to(bfloat16), fed the inputs .to(bfloat16).  With bf16-representable fp32 values the two
must agree bit for bit (outputs, and gradients after rounding to bf16); with general fp32 values the
autocast gradients are held to the project's bf16 contract (BF16_FACTOR, BF16_FLOOR of
tests/test_gpu_bf16_backward.py) against the fp64 oracle on the unrounded values.
"""
import copy

import pytest
import torch
import torch.nn as nn

import topology
from helpers import norm_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
BF16_FACTOR = 2.0  # tests/test_gpu_bf16_backward.py
BF16_FLOOR = 2e-2


def _autocast(**kw):
    return torch.autocast(device_type="cuda", dtype=BF16, **kw)


def _rep(x):
    """The nearest bf16-representable fp32 values."""
    return x.to(BF16).float()


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


# name -> (graph kind, molecules, h, depth, act, reduce, block options, train mode)
CASES = {
    "relu-sum": ("qm9", 64, 64, 3, "ReLU", "sum", {}, False),
    "silu-mean-36": ("qm9", 32, 36, 2, "SiLU", "mean", {}, False),  # scalar rows, unfused update
    "max": ("qm9", 64, 64, 3, "ReLU", "max", {}, False),
    "depth0": ("qm9", 16, 64, 0, "ReLU", "sum", {}, False),
    "shared": ("qm9", 32, 64, 3, "ReLU", "sum", dict(shared=True), False),
    "nobias": ("qm9", 32, 64, 2, "ReLU", "sum", dict(bias=False), False),
    "noresidual": ("qm9", 32, 64, 2, "ReLU", "sum", dict(residual=False), False),
    "dropout": ("qm9", 32, 64, 2, "ReLU", "sum", dict(dropout=0.25), True),
    "wide-528": ("zinc", 64, 528, 2, "ReLU", "sum", {}, False),  # wide layer and wide weight-gradient kernels
    "hub-33": ("b33", 0, 64, 2, "ReLU", "sum", {}, False),  # a node of in-degree 33 (topology.hub_caps)
    "hub-65": ("b65", 0, 64, 2, "ReLU", "mean", {}, False),  # in-degree 65: the chunked aggregation
}


def _case(name, representable):
    """(collated CPU graph with type features, raw, n_graphs, Xv, Xe, fp32 block on the CPU)."""
    kind, n, h, depth, act, reduce, opts, train = CASES[name]
    if kind in ("qm9", "zinc"):
        from notorch_amd.data.synth import make_batch

        G = make_batch(kind, n, seed=3).collate("nodes")
        raw = (G.num_nodes, G.edge_index, G.rev_index, G.batch_node_index)
    else:
        T = topology.block_graph(kind)
        assert T.in_degree().max() > 32
        G = T.collate()
        raw = T.raw()
    Xv, Xe = topology.embed(G.node_feats, G.edge_feats, h)
    blk = topology.make_block(h, depth, act, reduce, w_var=1 / 16, **opts)
    if representable:
        Xv, Xe = _rep(Xv), _rep(Xe)
        with torch.no_grad():
            for p in blk.parameters():
                p.copy_(_rep(p))
    blk.train(train)
    return G, raw, len(G), Xv, Xe, blk, reduce, depth


def _run(blk, G, Xv, Xe, reduce, autocast, grads, seed=7):
    """One forward (+ backward) on the device; the readout and the loss run outside the autocast region
    in the dtype of the block's outputs, the same ops for the autocast block and the yardstick.
    Returns (node, edge, [dXv, dXe, dW.., db..])."""
    from notorch_amd.nn import Mean, Sum

    for p in blk.parameters():
        p.grad = None
    Xv_d = Xv.to(DEV).requires_grad_(grads)
    Xe_d = Xe.to(DEV).requires_grad_(grads)
    Gd = G.to(DEV).update(node_feats=Xv_d, edge_feats=Xe_d)
    torch.manual_seed(seed)  # the dropout seed is drawn from torch's CPU generator
    with torch.set_grad_enabled(grads):
        if autocast:
            with _autocast():
                out = blk(Gd)
        else:
            out = blk(Gd)
        if not grads:
            return out.node_feats, out.edge_feats, None
        ro = (Mean if reduce == "mean" else Sum)()(out)
        e = out.edge_feats.float()
        loss = ro.float().pow(2).sum() + (e * torch.linspace(-1, 1, e.shape[1], device=DEV)).sum()
    loss.backward()
    layers = list({id(l): l for l in blk._chemprop_layers()}.values())
    gs = [Xv_d.grad, Xe_d.grad] + [l.linear.weight.grad for l in layers]
    gs += [l.linear.bias.grad for l in layers if l.linear.bias is not None]
    return out.node_feats, out.edge_feats, gs


def _names(blk):
    layers = list({id(l): l for l in blk._chemprop_layers()}.values())
    nb = sum(l.linear.bias is not None for l in layers)
    return ["dXv", "dXe"] + [f"dW[{i}]" for i in range(len(layers))] + [f"db[{i}]" for i in range(nb)]


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", list(CASES))
def test_forward_equals_bf16_storage(name):
    G, _, _, Xv, Xe, blk, reduce, _ = _case(name, representable=True)
    yard = copy.deepcopy(blk).to(DEV, BF16)
    blk = blk.to(DEV)
    node, edge, _ = _run(blk, G, Xv, Xe, reduce, True, False)
    assert node.dtype == BF16 and edge.dtype == BF16
    assert all(p.dtype == torch.float32 for p in blk.parameters())
    n_ref, e_ref, _ = _run(yard, G, Xv.to(BF16), Xe.to(BF16), reduce, False, False)
    assert torch.equal(edge, e_ref), "edge_feats"
    assert torch.equal(node, n_ref), "node_feats"
    # one fp32 and one bf16 feature tensor, and bf16 features with fp32 parameters: the same bits
    n2, e2, _ = _run(blk, G, Xv, Xe.to(BF16), reduce, True, False)
    assert torch.equal(e2, e_ref) and torch.equal(n2, n_ref)
    n3, e3, _ = _run(blk, G, Xv.to(BF16), Xe.to(BF16), reduce, True, False)
    assert torch.equal(e3, e_ref) and torch.equal(n3, n_ref)


def _embedded(h, depth, fuse, seed=2, **opts):
    from notorch_amd.nn import EmbeddedChempropBlock, GraphEmbedding

    torch.manual_seed(seed)
    emb = GraphEmbedding(hidden_dim=h)
    blk = topology.make_block(h, depth, w_var=1 / 16, **opts)
    return EmbeddedChempropBlock(emb, blk, fuse=fuse)


@pytest.mark.parametrize("h,reduce", [(64, "sum"), (36, "mean")])
def test_embedded_fused_equals_unfused(h, reduce):
    from notorch_amd.data.synth import make_batch

    G = make_batch("qm9", 32, seed=5).collate("nodes").to(DEV)
    fused = _embedded(h, 2, True, reduce=reduce).to(DEV).eval()
    unfused = _embedded(h, 2, False, reduce=reduce).to(DEV).eval()
    unfused.load_state_dict(fused.state_dict())
    with torch.no_grad(), _autocast():
        a, b = fused(G), unfused(G)
        emb_out = fused.embedding(G)
    assert a.node_feats.dtype == BF16 and a.edge_feats.dtype == BF16
    assert torch.equal(a.edge_feats, b.edge_feats) and torch.equal(a.node_feats, b.node_feats)
    assert emb_out.node_feats.dtype == torch.float32  # GraphEmbedding alone: fp32 out, as torch's embedding_bag
    # the single rounding: H0 of the fused init equals bf16 of the fp32 embedded sum (depth 0)
    d0 = _embedded(h, 0, True, reduce=reduce).to(DEV).eval()
    d0.embedding.load_state_dict(fused.embedding.state_dict())
    with torch.no_grad(), _autocast():
        H0 = d0(G).edge_feats
    want = (emb_out.node_feats[G.edge_index[0]] + emb_out.edge_feats).to(BF16)
    assert torch.equal(H0, want)


def test_fp32_features_enter_through_the_mixed_init(monkeypatch):
    """General (not bf16-representable) fp32 features: the block's H0 is bf16 of the fp32 sum Xv[src] + Xe,
    one rounding, which a torch cast of the features followed by the bf16 init does not give; the fused
    init kernel is what runs (one nt_dmpnn_init_mixed call per forward, in inference and in training)."""
    from notorch_amd import kernels as K

    G, _, _, Xv, Xe, blk, reduce, _ = _case("depth0", representable=False)
    src = G.edge_index[0].clone()
    want = (Xv[src] + Xe).to(BF16)
    assert not torch.equal(want, Xv.to(BF16)[src] + Xe.to(BF16))  # the inputs tell the two apart
    calls = []
    real = K.dmpnn_init_mixed
    monkeypatch.setattr(K, "dmpnn_init_mixed", lambda *a, **k: calls.append(1) or real(*a, **k))
    _, edge, _ = _run(blk.to(DEV), G, Xv, Xe, reduce, True, False)
    assert calls == [1]
    assert torch.equal(edge.cpu(), want)
    G3, _, _, Xv3, Xe3, blk3, reduce3, _ = _case("relu-sum", representable=False)
    _run(blk3.to(DEV), G3, Xv3, Xe3, reduce3, True, False)
    _run(blk3, G3, Xv3, Xe3, reduce3, True, True)
    assert calls == [1, 1, 1]


def test_embedded_fused_equals_unfused_on_a_hub_graph():
    """A node of in-degree 65 (the chunked aggregation): the fused embedded init routes as the plain one,
    so fuse=True and fuse=False still return the same bits."""
    G = topology.block_graph("b65").collate().to(DEV)
    fused = _embedded(64, 2, True, reduce="mean").to(DEV).eval()
    unfused = _embedded(64, 2, False, reduce="mean").to(DEV).eval()
    unfused.load_state_dict(fused.state_dict())
    with torch.no_grad(), _autocast():
        a, b = fused(G), unfused(G)
    assert a.node_feats.dtype == BF16
    assert torch.equal(a.edge_feats, b.edge_feats) and torch.equal(a.node_feats, b.node_feats)


def test_embedded_tables_of_two_dtypes_under_autocast():
    """One fp32 and one bf16 embedding table: the pair is not fused (embed.py requires one table dtype),
    GraphEmbedding returns one fp32 and one bf16 feature tensor and the block casts the fp32 one: the bits
    of the unfused module with the same tables."""
    from notorch_amd.data.synth import make_batch

    G = make_batch("qm9", 16, seed=5).collate("nodes").to(DEV)
    mods = []
    for fuse in (True, False):
        m = _embedded(64, 2, fuse).to(DEV).eval()
        m.embedding.edge.to(BF16)
        mods.append(m)
    mods[1].load_state_dict(mods[0].state_dict())
    with torch.no_grad(), _autocast():
        a, b = mods[0](G), mods[1](G)
    assert a.node_feats.dtype == BF16 and a.edge_feats.dtype == BF16
    assert torch.equal(a.edge_feats, b.edge_feats) and torch.equal(a.node_feats, b.node_feats)
    with torch.no_grad(), pytest.raises(RuntimeError, match="must share"):
        mods[0](G)  # outside autocast the pair is rejected as before


def test_library_weight_grad_keeps_fp32_partials():
    """The dW route without the weight-gradient kernel (h % 8 != 0, h > 2048, NT_WGRAD=library) at
    E >= 4096, where the GEMM is split over the edges: the partial products of an fp32 master weight's dW
    stay fp32 (exact bf16 products, fp32 accumulation: the fp32 contract against the fp64 product; partials
    rounded to bf16 would sit near 2^-9)."""
    from helpers import FP32_NORM_TOL
    from notorch_amd.nn.gnn import _engine

    g = torch.Generator().manual_seed(0)
    for E in (5000, 4096 * 2 + 3):  # two equal slices; four slices and a tail of 3 rows
        Gr, A = torch.randn(E, 36, generator=g).to(BF16), torch.randn(E, 36, generator=g).to(BF16)
        dW = _engine._weight_grad(Gr.to(DEV), A.to(DEV), torch.float32)
        assert dW.dtype == torch.float32
        assert norm_err(dW, Gr.double().t() @ A.double()) <= FP32_NORM_TOL
        assert _engine._weight_grad(Gr.to(DEV), A.to(DEV)).dtype == BF16  # the bf16-storage route is as it was


# ------------------------------------------------------------------ gradients
GRAD_CASES = [n for n in CASES if n != "hub-65"]


@pytest.mark.parametrize("name", GRAD_CASES)
def test_grads_equal_bf16_storage_after_rounding(name, monkeypatch):
    """Representable inputs: every fp32 leaf gets an fp32, finite gradient whose rounding to bf16 is the
    yardstick's gradient bit for bit; dW / db keep the weight-gradient kernel's fp32 result (they are not
    a widened bf16 value); a second backward returns the same bits.

    shared=True is held to this per layer, not at the leaf: the shared weight's .grad is autograd's sum
    of the d per-layer gradients, which the autocast block adds in fp32 (each dW_l unrounded, as
    specified) and the yardstick adds in bf16, rounding after every addition, so bf16(sum of fp32) and
    the bf16 running sum differ by construction (on an MI355X the leaf-level comparison of this case
    fails on dW[0] while every other case passes it).  Every layer's own dW_l / db_l, taken
    where block_backward returns them, still equals the yardstick's bit for bit after rounding, and the
    leaf is the fp32 sum of those (to fp32 rounding of a d-term sum, 1e-6 normalised)."""
    from notorch_amd.nn.gnn import _engine

    G, _, _, Xv, Xe, blk, reduce, depth = _case(name, representable=True)
    shared = bool(CASES[name][6].get("shared"))
    yard = copy.deepcopy(blk).to(DEV, BF16)
    blk = blk.to(DEV)
    per_layer = []
    real = _engine.block_backward

    def spy(*a, **k):
        out = real(*a, **k)
        per_layer.append((list(out[2]), list(out[3])))
        return out

    monkeypatch.setattr(_engine, "block_backward", spy)
    node, edge, got = _run(blk, G, Xv, Xe, reduce, True, True)
    n_ref, e_ref, ref = _run(yard, G, Xv.to(BF16), Xe.to(BF16), reduce, False, True)
    assert torch.equal(edge, e_ref) and torch.equal(node, n_ref)
    (dWs, dbs), (dWs_ref, dbs_ref) = per_layer
    assert len(dWs) == len(dWs_ref) == depth
    for l in range(depth):  # every layer's own gradients, shared or not
        assert dWs[l].dtype == torch.float32 and dbs[l].dtype == torch.float32 and dWs_ref[l].dtype == BF16
        assert torch.equal(dWs[l].to(BF16), dWs_ref[l]), f"layer {l}: dW differs after rounding"
        assert torch.equal(dbs[l].to(BF16), dbs_ref[l]), f"layer {l}: db differs after rounding"
    names = _names(blk)
    assert len(got) == len(ref) == len(names)
    kept = {"dW": 0, "db": 0}
    for nm, g, r in zip(names, got, ref):
        assert g is not None and g.dtype == torch.float32, nm
        assert torch.isfinite(g).all(), nm
        assert r.dtype == BF16
        if shared and nm[:2] in kept:
            parts = dWs if nm[:2] == "dW" else dbs
            assert norm_err(g, sum(p.double() for p in parts)) <= 1e-6, f"{nm}: not the fp32 sum of its layers"
        else:
            assert torch.equal(g.to(BF16), r), f"{nm}: differs from the bf16-storage gradient after rounding"
        if nm[:2] in kept and bool((g != g.bfloat16().float()).any()):
            kept[nm[:2]] += 1
    if depth:
        assert kept["dW"] >= 1, "every dW equals its own bf16 rounding: the fp32 result was not kept"
        if any(nm.startswith("db") for nm in names):
            assert kept["db"] >= 1, "every db equals its own bf16 rounding: the fp32 result was not kept"
    _, _, again = _run(blk, G, Xv, Xe, reduce, True, True)
    for nm, g, a in zip(names, got, again):
        assert torch.equal(g, a), f"{nm}: not deterministic"


def _dropout_masks(p, E, h, depth, seed=7):
    """The keep / (1 - p) masks the block draws in _run (its seed is the first draw from torch's CPU
    generator after torch.manual_seed(seed)), regenerated by the hash kernel as the backward does."""
    from notorch_amd import kernels as K
    from notorch_amd.nn.gnn import _engine

    torch.manual_seed(seed)
    s = _engine.draw_dropout_seed()
    ones = torch.ones(E, h, device=DEV)
    return [(K.dropout_residual(ones, p, s, _engine.dropout_offset(l, E, h)) > 0).double().cpu() / (1 - p)
            for l in range(depth)]


def _truth(raw, n_graphs, Xv, Xe, blk, act, reduce, residual, masks):
    """topology.oracle_grads in fp64 with the block's residual flag and dropout masks; a shared layer's
    per-copy gradients summed into its one leaf; [dXv, dXe, dW.., db..]."""
    from oracle import dmpnn_ref

    V, edge_index, rev, batch = raw
    dt = torch.float64
    Ws, bs = dmpnn_ref.block_params(blk)
    shared = len({id(l) for l in blk._chemprop_layers()}) < len(Ws)
    Ws = [W.detach().to(dt, copy=True).requires_grad_(True) for W in Ws]
    bs = [None if b is None else b.detach().to(dt, copy=True).requires_grad_(True) for b in bs]
    Xv_r = Xv.detach().to(dt, copy=True).requires_grad_(True)
    Xe_r = Xe.detach().to(dt, copy=True).requires_grad_(True)
    n, e = dmpnn_ref.chemprop_block(Xv_r, Xe_r, edge_index, rev, Ws, bs, act=topology.ACTS[act][1],
                                    residual=residual, reduce=reduce, dropout_masks=masks)
    r = dmpnn_ref.readout(n, batch, n_graphs, topology.readout_of(reduce))
    loss = r.pow(2).sum() + (e * torch.linspace(-1, 1, e.shape[1], dtype=dt)).sum()
    loss.backward()
    dW, db = [W.grad for W in Ws], [b.grad for b in bs if b is not None]
    if shared:
        dW, db = [sum(dW)], ([sum(db)] if db else [])
    return [Xv_r.grad, Xe_r.grad] + dW + db


@pytest.mark.parametrize("name", GRAD_CASES)
def test_grads_against_fp64_oracle(name):
    """General fp32 inputs and weights, every gradient case (depth 0, bias=False, residual=False and
    train-mode dropout included: the truth of the dropout case applies the block's own masks,
    regenerated by the hash kernel): against the fp64 oracle on the unrounded values the autocast
    gradients are no further than max(BF16_FLOOR, BF16_FACTOR x the yardstick's error against the same
    truth), on the normalised max error and on the relative L2 error."""
    kind, n, h, depth, act, reduce, opts, _ = CASES[name]
    G, raw, ngraphs, Xv, Xe, blk, reduce, depth = _case(name, representable=False)
    masks = _dropout_masks(opts["dropout"], Xe.shape[0], h, depth) if opts.get("dropout") else None
    truth = _truth(raw, ngraphs, Xv, Xe, blk, act, reduce, opts.get("residual", True), masks)
    yard = copy.deepcopy(blk).to(DEV, BF16)
    blk = blk.to(DEV)
    _, _, got = _run(blk, G, Xv, Xe, reduce, True, True)
    _, _, ref = _run(yard, G, Xv.to(BF16), Xe.to(BF16), reduce, False, True)
    names = _names(blk)
    assert len(got) == len(ref) == len(truth) == len(names)
    for nm, g, r, t in zip(names, got, ref, truth):
        assert g.dtype == torch.float32 and torch.isfinite(g).all(), nm
        e_max, r_max = norm_err(g, t), norm_err(r.float(), t)
        e_l2, r_l2 = _rel_l2(g, t), _rel_l2(r, t)
        print(f"{name} {nm}: autocast max {e_max:.2e} l2 {e_l2:.2e} | bf16 storage max {r_max:.2e} l2 {r_l2:.2e}")
        assert e_max <= max(BF16_FLOOR, BF16_FACTOR * r_max), f"{nm}: max {e_max:.3e} vs bf16 storage {r_max:.3e}"
        assert e_l2 <= max(BF16_FLOOR, BF16_FACTOR * r_l2), f"{nm}: L2 {e_l2:.3e} vs bf16 storage {r_l2:.3e}"


def _embedded_run(mod, G, autocast):
    from notorch_amd.nn import Sum

    for p in mod.parameters():
        p.grad = None
    if autocast:
        with _autocast():
            out = mod(G)
    else:
        out = mod(G)
    e = out.edge_feats.float()
    loss = Sum()(out).float().pow(2).sum() + (e * torch.linspace(-1, 1, e.shape[1], device=DEV)).sum()
    loss.backward()
    layers = mod.block._chemprop_layers()
    return ([mod.embedding.node.weight.grad, mod.embedding.edge.weight.grad]
            + [l.linear.weight.grad for l in layers] + [l.linear.bias.grad for l in layers])


@pytest.mark.parametrize("fuse", [True, False])
def test_embedding_table_grads(fuse):
    """fp32 tables under autocast: fp32, finite, deterministic table gradients within the bf16 contract
    of the fp64 oracle (the yardstick: the same module moved .to(bfloat16))."""
    from notorch_amd.data.synth import make_batch

    h, depth = 64, 2
    Gc = make_batch("qm9", 32, seed=6).collate("nodes")
    mod = _embedded(h, depth, fuse).train()
    Tv, Te = mod.embedding.node.weight.detach().double(), mod.embedding.edge.weight.detach().double()
    Xv = Tv[Gc.node_feats].sum(1)
    Xe = Te[Gc.edge_feats].sum(1)
    raw = (Gc.num_nodes, Gc.edge_index, Gc.rev_index, Gc.batch_node_index)
    t = topology.oracle_grads(raw, len(Gc), Xv, Xe, mod.block, "ReLU", "sum", torch.float64)[1:]
    dTv = torch.zeros_like(Tv).index_add_(0, Gc.node_feats.reshape(-1),
                                           t[0].repeat_interleave(Gc.node_feats.shape[1], 0))
    dTe = torch.zeros_like(Te).index_add_(0, Gc.edge_feats.reshape(-1),
                                           t[1].repeat_interleave(Gc.edge_feats.shape[1], 0))
    truth = [dTv, dTe] + t[2:]
    yard = copy.deepcopy(mod).to(DEV, BF16)
    mod = mod.to(DEV)
    G = Gc.to(DEV)
    got = _embedded_run(mod, G, True)
    ref = _embedded_run(yard, G, False)
    names = ["dTv", "dTe"] + [f"dW[{i}]" for i in range(depth)] + [f"db[{i}]" for i in range(depth)]
    for nm, g, r, tr in zip(names, got, ref, truth):
        assert g.dtype == torch.float32 and torch.isfinite(g).all(), nm
        assert r.dtype == BF16
        e_max, r_max = norm_err(g, tr), norm_err(r.float(), tr)
        e_l2, r_l2 = _rel_l2(g, tr), _rel_l2(r, tr)
        print(f"fuse={fuse} {nm}: autocast max {e_max:.2e} l2 {e_l2:.2e} | bf16 storage max {r_max:.2e} l2 {r_l2:.2e}")
        assert e_max <= max(BF16_FLOOR, BF16_FACTOR * r_max), nm
        assert e_l2 <= max(BF16_FLOOR, BF16_FACTOR * r_l2), nm
    again = _embedded_run(mod, G, True)
    for nm, g, a in zip(names, got, again):
        assert torch.equal(g, a), f"{nm}: not deterministic"


def test_torch_recompute_backward_under_autocast(monkeypatch):
    """NT_BWD=torch (the A/B reference) under autocast: the recompute runs on the rounded copies and
    returns every gradient in its leaf's dtype; the kernel backward is held to the bf16 contract
    against it (no further from the fp64 oracle than BF16_FACTOR x the recompute, or the floor)."""
    G, raw, ngraphs, Xv, Xe, blk, reduce, _ = _case("relu-sum", representable=False)
    truth = topology.oracle_grads(raw, ngraphs, Xv, Xe, blk, "ReLU", reduce, torch.float64)[1:]
    blk = blk.to(DEV)
    _, _, kern = _run(blk, G, Xv, Xe, reduce, True, True)
    monkeypatch.setenv("NT_BWD", "torch")
    node, _, ref = _run(blk, G, Xv, Xe, reduce, True, True)
    assert node.dtype == BF16
    for nm, g, r, t in zip(_names(blk), kern, ref, truth):
        assert r.dtype == torch.float32 and torch.isfinite(r).all(), nm
        assert norm_err(g, t) <= max(BF16_FLOOR, BF16_FACTOR * norm_err(r, t)), nm


# ------------------------------------------------------------------ cache
def test_fp32_and_bf16_images_live_side_by_side():
    G, _, _, Xv, Xe, blk, reduce, _ = _case("relu-sum", representable=False)
    blk = blk.to(DEV)
    n0, e0, _ = _run(blk, G, Xv, Xe, reduce, False, False)
    assert n0.dtype == torch.float32
    na, _, _ = _run(blk, G, Xv, Xe, reduce, True, False)
    assert na.dtype == BF16
    n1, e1, _ = _run(blk, G, Xv, Xe, reduce, False, False)
    assert torch.equal(n0, n1) and torch.equal(e0, e1)
    nb, _, _ = _run(blk, G, Xv, Xe, reduce, True, False)
    assert torch.equal(na, nb)


def test_inference_forwards_pack_once(monkeypatch):
    from notorch_amd import kernels as K

    G, _, _, Xv, Xe, blk, reduce, depth = _case("relu-sum", representable=False)
    blk = blk.to(DEV)
    calls = []
    real = K.pack_weights_mixed
    monkeypatch.setattr(K, "pack_weights_mixed", lambda *a, **k: calls.append(len(a[0])) or real(*a, **k))
    a, _, _ = _run(blk, G, Xv, Xe, reduce, True, False)
    b, _, _ = _run(blk, G, Xv, Xe, reduce, True, False)
    assert calls == [depth], f"one launch for all {depth} layers, once: {calls}"
    assert torch.equal(a, b)


def test_more_than_sixteen_layers_and_a_shared_layer(monkeypatch):
    from notorch_amd import kernels as K

    calls = []
    real = K.pack_weights_mixed
    monkeypatch.setattr(K, "pack_weights_mixed", lambda *a, **k: calls.append(len(a[0])) or real(*a, **k))
    from notorch_amd.data.synth import make_batch

    G = make_batch("qm9", 8, seed=3).collate("nodes")
    Xv, Xe = topology.embed(G.node_feats, G.edge_feats, 16)
    for depth, opts, want in ((18, {}, [16, 2]), (5, dict(shared=True), [1])):
        del calls[:]
        blk = topology.make_block(16, depth, w_var=1 / 64, **opts)
        with torch.no_grad():
            for p in blk.parameters():
                p.copy_(_rep(p))
        yard = copy.deepcopy(blk).to(DEV, BF16)
        node, edge, _ = _run(blk.to(DEV), G, _rep(Xv), _rep(Xe), "sum", True, False)
        assert calls == want, (depth, calls)
        n_ref, e_ref, _ = _run(yard, G, Xv.to(BF16), Xe.to(BF16), "sum", False, False)
        assert torch.equal(node, n_ref) and torch.equal(edge, e_ref)


def test_optimizer_step_invalidates_both_images():
    G, _, _, Xv, Xe, blk, reduce, _ = _case("relu-sum", representable=False)
    blk = blk.to(DEV).train()
    opt = torch.optim.Adam(blk.parameters(), lr=1e-2)
    _run(blk, G, Xv, Xe, reduce, False, False)  # the fp32 image is cached too
    _run(blk, G, Xv, Xe, reduce, True, True)
    opt.step()
    node, edge, _ = _run(blk, G, Xv, Xe, reduce, True, False)
    fresh = topology.make_block(CASES["relu-sum"][2], CASES["relu-sum"][3], w_var=1 / 16, seed=99).to(DEV)
    fresh.load_state_dict(blk.state_dict())
    n_ref, e_ref, _ = _run(fresh, G, Xv, Xe, reduce, True, False)
    assert torch.equal(node, n_ref) and torch.equal(edge, e_ref)
    n32, _, _ = _run(blk, G, Xv, Xe, reduce, False, False)
    f32, _, _ = _run(fresh, G, Xv, Xe, reduce, False, False)
    assert torch.equal(n32, f32)


# ------------------------------------------------------------------ outside autocast
def test_outside_bf16_autocast_nothing_changes():
    G, _, _, Xv, Xe, blk, reduce, _ = _case("relu-sum", representable=False)
    blk = blk.to(DEV)
    Gd = G.to(DEV).update(node_feats=Xv.to(DEV), edge_feats=Xe.to(DEV))
    with torch.no_grad():
        plain = blk(Gd)
        assert plain.node_feats.dtype == torch.float32
        with pytest.raises(RuntimeError, match="must share"):
            blk(Gd.update(node_feats=Xv.to(DEV, BF16), edge_feats=Xe.to(DEV, BF16)))
        with torch.autocast(device_type="cuda", dtype=torch.float16):
            half = blk(Gd)
        with _autocast(), torch.autocast(device_type="cuda", enabled=False):
            nested = blk(Gd)
        with _autocast(enabled=False):
            off = blk(Gd)
    for out in (half, nested, off):
        assert out.node_feats.dtype == torch.float32 and out.edge_feats.dtype == torch.float32
        assert torch.equal(out.node_feats, plain.node_feats) and torch.equal(out.edge_feats, plain.edge_feats)


def test_unsupported_h_and_layerwise_blocks_stay_fp32_under_autocast():
    """h = 516 is outside the bf16 rule, and a block with an activation that has no kernel code takes the
    layer-by-layer path: the block leaves both alone (fp32 out, the bits of a plain call).  The generic
    activation here is one torch's autocast does not lower itself (nn.Hardtanh; nn.PReLU is on autocast's
    own bf16 list, so its module call returns bf16 whatever the block does)."""
    from notorch_amd.data.synth import make_batch
    from notorch_amd.nn import ChempropBlock

    for h, act in ((516, nn.ReLU), (32, nn.Hardtanh)):
        G = make_batch("qm9", 8, seed=3).collate("nodes")
        Xv, Xe = topology.embed(G.node_feats, G.edge_feats, h)
        torch.manual_seed(0)
        blk = ChempropBlock(h, act=act, depth=2).to(DEV).eval()
        Gd = G.to(DEV).update(node_feats=Xv.to(DEV), edge_feats=Xe.to(DEV))
        with torch.no_grad():
            plain = blk(Gd)
            with _autocast():
                auto = blk(Gd)
        assert auto.node_feats.dtype == torch.float32
        assert torch.equal(auto.node_feats, plain.node_feats) and torch.equal(auto.edge_feats, plain.edge_feats)
