"""GPU: training-mode dropout inside the fused layer launch (nt_dmpnn_update_fused_dropout):

    U[e]       = W (S[src e] - act(H[rev e])) + b
    H_out[e,j] = (residual ? H[e,j] : 0) + keep(seed, offset + e h + j) U[e,j] / (1 - p)
    S_out[v]   = reduce_{dst e = v} agg_act(H_out[e])

(a) one launch per kernel instance (fp32: the two-workgroup 64-row walk, the 128-row walk, the generic
    64-row instances, h = 400, the column chunks of h = 640, max, hub sub-run partials, in-degree-0
    nodes, padded rows; bf16: h = 64 and the h = 640 column-pass kernel):
    * mask exactness against M = nt_dropout_residual(ones, p, seed, offset), offset != 0: where M == 0,
      H_out is H bit for bit (0 without the residual); p = 1 gives H everywhere;
    * values against the fp64 composition H + M (W A + b): fp32 at tests/test_gpu_dropout.py's
      normalised 1e-5, bf16 at tests/test_gpu_bf16.py's absolute block criterion 2e-2;
    * S_out by tests/test_gpu_topology.py's criterion for the plain fused launch: the bits of the CPU
      scatter (ascending edge id) of the kernel's own stored H_out (bf16: rounded once), and
      nt_segment_reduce of it;
    * amax_out = max|H_out|, max|S_out| of the dropped outputs.
(b) modules: the path taken (LAST_UPDATE_INFO), forward and every gradient against the fp64 oracle with
    the same masks (tests/test_gpu_dropout.py's tolerance), bf16 storage and bf16 autocast by
    tests/test_gpu_bf16_wide.py's yardstick, agreement with the NT_FUSED_DROPOUT=0 path,
    reproducibility, EmbeddedChempropBlock and the standalone ChempropLayer.
p = 0.25 throughout: masks keep 60-90 % of the elements (asserted)."""
import functools

import pytest
import torch
import torch.nn as nn

import topology as T
from helpers import assert_parity, norm_err
from oracle import dmpnn_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
TOL = 1e-5          # tests/test_gpu_dropout.py
BLOCK_TOL = 2e-2    # tests/test_gpu_bf16.py
BF16_FACTOR = 2.0   # tests/test_gpu_bf16_wide.py
P, SEED, OFFSET = 0.25, 0x5EED5EED5EED, 3 * 977 * 48 + 5  # a layer-3-like, odd counter offset

_ACT = {"relu": (nn.ReLU(), torch.relu), "identity": (nn.Identity(), lambda x: x),
        "silu": (nn.SiLU(), torch.nn.functional.silu)}
_WALK = {"nw4": "two 4-wave workgroups per CU, 64-row tiles, dropout in the epilogue",
         "wide": "one 8-wave workgroup per CU, 128-row tiles, dropout in the epilogue",
         "narrow": "one 8-wave workgroup per CU, 64-row tiles, dropout in the epilogue",
         "bf16": "update_bf16_kernel: two 4-wave workgroups per CU, 64-edge tiles, dropout in the epilogue",
         "bf16wide": "update_bf16_kernel: wide (h > 512)"}


def _K():
    from notorch_amd import kernels

    return kernels


def _last_kernel():
    from notorch_amd import _lib

    return _lib.load().nt_last_kernel().decode()


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(collated graph on the CPU, V, E, max in-degree); qm9-<n> or a graph of tests/topology.py."""
    if name.startswith("qm9-"):
        from notorch_amd.data.synth import make_batch

        G = make_batch("qm9", int(name[4:]), seed=4).collate("nodes")
    else:
        G = T.block_graph(name).collate("nodes")
    deg = torch.bincount(G.edge_index[1], minlength=G.num_nodes)
    return G, G.num_nodes, G.num_edges, int(deg.max())


@functools.lru_cache(maxsize=None)
def _operands(name, h, dtype):
    """H, S, W, b on the CPU in the storage dtype, drawn once per (graph, h, dtype)."""
    _, V, E, _ = _graph(name)
    g = torch.Generator().manual_seed(1000 + h)
    H, S = torch.randn(E, h, generator=g), torch.randn(V, h, generator=g)
    W, b = torch.randn(h, h, generator=g) / h ** 0.5, torch.randn(h, generator=g)
    return tuple(t.to(dtype) for t in (H, S, W, b))


@functools.lru_cache(maxsize=None)
def _mask(E, h, p=P, seed=SEED, offset=OFFSET):
    """keep / (1 - p) in fp64 on the CPU from nt_dropout_residual on ones, and the keep decisions."""
    M = _K().dropout_residual(torch.ones(E, h, device=DEV), p, seed, offset).cpu()
    kept = M != 0
    return kept.double() / (1 - p) if p < 1 else kept.double(), kept


def _ref(name, h, dtype, act, residual, p=P):
    """The fp64 composition (residual ? H : 0) + M (W A + b) on the stored operands."""
    G, V, E, _ = _graph(name)
    H, S, W, b = (t.double() for t in _operands(name, h, dtype))
    A = S[G.edge_index[0]] - _ACT[act][1](H)[G.rev_index]
    U = A @ W.T + b
    Mk, kept = _mask(E, h, p)
    return (H if residual else 0) + Mk * U, kept


def _launch(name, h, dtype, rows, act="relu", reduce="sum", agg="relu", residual=True, p=P, pitch=None):
    """One launch over the largest-tile plan of `rows` rows; (H_out, S_out, amax_out) on the device."""
    K = _K()
    G, V, E, D = _graph(name)
    H, S, W, b = (t.to(DEV) for t in _operands(name, h, dtype))
    if pitch is not None:
        Hp, Sp = K.padded_rows(E, h, pitch, dtype, DEV), K.padded_rows(V, h, pitch, dtype, DEV)
        Hp.copy_(H)
        Sp.copy_(S)
        H, S = Hp, Sp
    dst_ptr, perm = K.csr_build(G.edge_index[1].to(DEV), V)
    plan = K.tile_plan(dst_ptr, E, D, rows=rows, ncu=0)
    amax_out = torch.zeros(2, device=DEV) if dtype == torch.float32 else None
    a, g = K.act_code(_ACT[act][0]), K.act_code(_ACT[agg][0])
    if dtype == torch.float32:
        assert K.fused_tile_rows(h, dtype, a, reduce, g) >= rows
    Hn, Sn = K.dmpnn_update_fused(H, S, G.edge_index[0].to(DEV), G.rev_index.to(DEV), K.pack_weights(W), b,
                                  residual=residual, act=a, plan=plan, tile_rows=rows, max_in_degree=D, perm=perm,
                                  reduce=reduce, agg_act=g, zero_fill=True, amax_out=amax_out, pitch_out=pitch,
                                  dropout=(p, SEED, OFFSET))
    return Hn, Sn, amax_out, (dst_ptr, perm)


def _check_launch(name, h, dtype, rows, walk, act="relu", reduce="sum", agg="relu", residual=True):
    K = _K()
    G, V, E, D = _graph(name)
    Hn, Sn, amax_out, (dst_ptr, perm) = _launch(name, h, dtype, rows, act, reduce, agg, residual)
    assert _WALK[walk] in _last_kernel(), _last_kernel()
    assert Hn.dtype == dtype and Sn.dtype == dtype
    ref, kept = _ref(name, h, dtype, act, residual)
    case = f"{name} h={h} {dtype} {walk} {act} {reduce} {agg} residual={residual}"
    assert 0.6 < kept.double().mean().item() < 0.9, case
    # mask exactness: a dropped element is the residual term bit for bit
    H = _operands(name, h, dtype)[0]
    base = H if residual else torch.zeros_like(H)
    got = Hn.cpu()
    assert torch.equal(got[~kept], base[~kept]), f"{case}: dropped elements differ from the residual term"
    assert not torch.equal(got[kept], base[kept]), f"{case}: no element took its update"
    # values
    e = norm_err(got, ref)
    print(f"FUSEDDROP H {e:.3e} {case}")
    assert_parity(got, ref, TOL if dtype == torch.float32 else BLOCK_TOL, f"H {case}")
    # aggregation: of the stored, dropped H_out
    agg_fn = _ACT[agg][1]
    exact = dmpnn_ref.scatter(agg_fn(got.float()), G.edge_index[1], V, reduce).to(dtype)
    if agg in ("relu", "identity"):  # (a transcendental agg_act differs between the CPU and the device)
        bad = torch.nonzero((Sn.cpu() != exact).any(1)).flatten().tolist()
        assert not bad, f"{case}: S_out rows differ from the scatter of the stored H_out at nodes {bad[:8]}"
    else:
        assert_parity(Sn.float(), exact.float(), TOL if dtype == torch.float32 else 2.0 ** -8, f"S {case}")
    seg = K.segment_reduce(Hn.contiguous(), dst_ptr, perm, V, reduce=reduce, act=K.act_code(_ACT[agg][0]))
    assert_parity(Sn.float(), seg.float(), TOL if dtype == torch.float32 else 2.0 ** -8, f"S vs segment_reduce {case}")
    if amax_out is not None:
        assert amax_out[0].item() == Hn.abs().max().item(), case
        assert amax_out[1].item() == Sn.abs().max().item(), case


# (graph, h, rows, walk, act, reduce, agg): every instance the engine dispatches
FP32_CASES = [
    ("qm9-24", 48, 64, "nw4", "relu", "sum", "relu"),       # 3-round scan, the bias in LDS
    ("qm9-24", 48, 64, "nw4", "relu", "sum", "identity"),   # the last layer's node scatter
    ("qm9-24", 48, 128, "wide", "relu", "sum", "relu"),
    ("b32", 48, 64, "nw4", "relu", "sum", "relu"),          # in-degree 32: the 16-round scan
    ("b32", 48, 128, "wide", "relu", "sum", "identity"),
    ("b10", 48, 128, "wide", "relu", "sum", "relu"),        # the 8-round scan
    ("qm9-24", 300, 64, "narrow", "silu", "mean", "silu"),  # generic instance, h % 16 != 0
    ("qm9-24", 300, 64, "nw4", "relu", "sum", "relu"),      # 19 column tiles on 4 waves x 5
    ("qm9-8", 400, 64, "narrow", "relu", "sum", "relu"),    # 25 column tiles: 4 per wave, one chunk
    ("qm9-8", 640, 64, "narrow", "relu", "sum", "relu"),    # two column chunks
    ("qm9-8", 640, 64, "narrow", "silu", "sum", "identity"),
    ("qm9-24", 48, 64, "narrow", "relu", "max", "relu"),
    ("dir", 48, 64, "nw4", "relu", "sum", "relu"),          # in-degree-0 nodes: zero fill
    ("dir", 48, 64, "narrow", "relu", "mean", "relu"),
]


@pytest.mark.parametrize("name,h,rows,walk,act,reduce,agg", FP32_CASES)
def test_fused_dropout_launch_fp32(name, h, rows, walk, act, reduce, agg):
    _check_launch(name, h, torch.float32, rows, walk, act, reduce, agg)


@pytest.mark.parametrize("name,h,walk,act,reduce,agg", [
    ("qm9-24", 64, "bf16", "relu", "sum", "relu"), ("qm9-24", 64, "bf16", "relu", "mean", "identity"),
    ("b32", 64, "bf16", "silu", "max", "silu"), ("dir", 64, "bf16", "relu", "sum", "relu"),
    ("qm9-8", 640, "bf16wide", "relu", "sum", "relu"), ("qm9-8", 640, "bf16wide", "silu", "sum", "identity")])
def test_fused_dropout_launch_bf16(name, h, walk, act, reduce, agg):
    _check_launch(name, h, BF, 64, walk, act, reduce, agg)
    assert "dropout in the epilogue" in _last_kernel()


@pytest.mark.parametrize("name,h,dtype,rows,walk", [
    ("qm9-24", 48, torch.float32, 64, "nw4"), ("qm9-24", 48, torch.float32, 128, "wide"),
    ("qm9-8", 640, torch.float32, 64, "narrow"), ("qm9-24", 64, BF, 64, "bf16"), ("qm9-8", 640, BF, 64, "bf16wide")])
def test_fused_dropout_launch_without_residual(name, h, dtype, rows, walk):
    """residual = False: a dropped element is exactly 0."""
    _check_launch(name, h, dtype, rows, walk, residual=False)


@pytest.mark.parametrize("name,h,dtype,rows", [
    ("qm9-24", 48, torch.float32, 64), ("qm9-24", 48, torch.float32, 128), ("qm9-8", 400, torch.float32, 64),
    ("qm9-24", 64, BF, 64), ("qm9-8", 640, BF, 64)])
def test_fused_dropout_p_one_and_zero(name, h, dtype, rows):
    """p = 1 drops everything (H_out = H, S_out its aggregation); p = 0 keeps everything: the bits of
    the plain fused launch on fp32 values up to the order of the residual add, bf16 exactly."""
    K = _K()
    G, V, E, D = _graph(name)
    H = _operands(name, h, dtype)[0]
    Hn, Sn, amax_out, _ = _launch(name, h, dtype, rows, p=1.0)
    assert torch.equal(Hn.cpu(), H)
    exact = dmpnn_ref.scatter(torch.relu(H.float()), G.edge_index[1], V, "sum").to(dtype)
    assert torch.equal(Sn.cpu(), exact)
    if amax_out is not None:
        assert amax_out[0].item() == H.abs().max().item()
    H0, S0, _, _ = _launch(name, h, dtype, rows, p=0.0)
    ref, _ = _ref(name, h, dtype, "relu", True, p=0.0)
    assert_parity(H0.cpu(), ref, TOL if dtype == torch.float32 else BLOCK_TOL, "p = 0")


def test_fused_dropout_mask_index_is_dense_under_a_row_pitch():
    """fp32 rows 304 floats apart (h = 300): the mask is indexed by e h + j, so the padded launch has
    the bits of the dense one."""
    Hd, Sd, amd, _ = _launch("qm9-24", 300, torch.float32, 64)
    Hp, Sp, amp, _ = _launch("qm9-24", 300, torch.float32, 64, pitch=304)
    assert Hp.stride(0) == 304 and Sp.stride(0) == 304
    assert torch.equal(Hp.contiguous(), Hd) and torch.equal(Sp.contiguous(), Sd) and torch.equal(amd, amp)


@pytest.mark.parametrize("rows", [64, 128])
@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_fused_dropout_hub_partials(rows, reduce):
    """b33 (one node of in-degree 33: a hub cut into sub-runs): the dropout launch writes the sub-runs'
    partials from the dropped H_out and hub_combine finishes the hub's row."""
    from notorch_amd.nn.gnn import _engine

    K = _K()
    h = 48
    Gc, V, E, _ = _graph("b33")
    Gd = T.block_graph("b33").collate("nodes").to(DEV)
    lay = Gd._nt_layout
    H, S, W, b = (t.to(DEV) for t in _operands("b33", h, torch.float32))
    src, rev = Gd.edge_index[0].contiguous(), Gd.rev_index
    relu = K.act_code(nn.ReLU())
    rows = min(rows, K.fused_tile_rows(h, torch.float32, relu, reduce, relu))
    tile_ptr, ntiles, dsts, zf = _engine.fused_plan(lay, V, E, rows)
    maxdeg = _engine.fused_max_in_degree(lay)
    rt0 = K.dmpnn_row_table(lay.dst_perm, dsts, src, rev, V)
    rt, nslots, hubs, slot_ptr = K.hub_runs(rt0, lay.dst_ptr, dsts, tile_ptr, _engine.HUB_DEGREE, maxdeg)
    assert nslots > 0 and hubs.numel() >= 1
    part = torch.empty(nslots, h, device=DEV)
    amax_out = torch.zeros(2, device=DEV)
    Hn, Sn = K.dmpnn_update_fused(H, S, src, rev, K.pack_weights(W), b, act=relu, plan=(tile_ptr, ntiles, dsts),
                                  tile_rows=rows, max_in_degree=maxdeg, perm=lay.dst_perm, reduce=reduce,
                                  agg_act=relu, zero_fill=True, amax_out=amax_out, row_table=rt, S_part=part,
                                  dropout=(P, SEED, OFFSET))
    assert "dropout in the epilogue" in _last_kernel()
    K.hub_combine(part, hubs, slot_ptr, lay.dst_ptr, Sn, reduce=reduce, amax=amax_out[1:2])
    ref, kept = _ref("b33", h, torch.float32, "relu", True)
    got = Hn.cpu()
    assert torch.equal(got[~kept], H.cpu()[~kept])
    assert_parity(got, ref, TOL, "H b33")
    exact = dmpnn_ref.scatter(torch.relu(got), Gc.edge_index[1], V, reduce)
    assert_parity(Sn, exact, TOL, f"S_out with hub partials ({reduce})")
    plain = torch.ones(V, dtype=torch.bool)
    plain[hubs.long().cpu()] = False
    assert torch.equal(Sn.cpu()[plain], exact[plain])  # the non-hub rows: the scan's own bits
    if reduce == "max":
        assert torch.equal(Sn.cpu(), exact)
    assert amax_out[0].item() == Hn.abs().max().item()
    assert amax_out[1].item() >= Sn.abs().max().item() > 0


# ------------------------------------------------------------------------------------ modules
def _features(G, h, seed=0):
    torch.manual_seed(seed)
    Xv = nn.EmbeddingBag(42, h, mode="sum")(G.node_feats).detach()
    Xe = nn.EmbeddingBag(13, h, mode="sum")(G.edge_feats).detach()
    return Xv, Xe


def _block_masks(draw_seed, p, E, h, depth):
    from notorch_amd.nn.gnn import _engine

    torch.manual_seed(draw_seed)
    s = _engine.draw_dropout_seed()
    return [_mask(E, h, p, s, _engine.dropout_offset(l, E, h))[0] for l in range(depth)]


def _train_step(blk, G, Xv, Xe, draw_seed):
    """One training forward + backward of the block: (node, edge, dXv, dXe, [dW], [db], path record)."""
    from notorch_amd.nn.gnn import _engine

    for q in blk.parameters():
        q.grad = None
    Xv_d, Xe_d = Xv.to(DEV).requires_grad_(True), Xe.to(DEV).requires_grad_(True)
    _engine.LAST_UPDATE_INFO.clear()
    torch.manual_seed(draw_seed)
    out = blk(G.update(node_feats=Xv_d, edge_feats=Xe_d).to(DEV))
    info = dict(_engine.LAST_UPDATE_INFO)
    wts = torch.linspace(-1, 1, Xv.shape[1], device=DEV)
    (out.node_feats.pow(2).sum() + (out.edge_feats * wts).sum()).backward()
    layers = blk._chemprop_layers()
    return (out.node_feats.detach(), out.edge_feats.detach(), Xv_d.grad, Xe_d.grad,
            [l.linear.weight.grad for l in layers], [l.linear.bias.grad for l in layers], info)


def _oracle_step(blk, G, Xv, Xe, masks, reduce, residual, act=torch.relu):
    Ws, bs = dmpnn_ref.block_params(blk)
    Ws = [W.detach().double().cpu().requires_grad_(True) for W in Ws]
    bs = [b.detach().double().cpu().requires_grad_(True) for b in bs]
    Xv_r, Xe_r = Xv.double().requires_grad_(True), Xe.double().requires_grad_(True)
    n_r, e_r = dmpnn_ref.chemprop_block(Xv_r, Xe_r, G.edge_index, G.rev_index, Ws, bs, act=act, residual=residual,
                                        reduce=reduce, dropout_masks=masks)
    wts = torch.linspace(-1, 1, Xv.shape[1], dtype=torch.float64)
    (n_r.pow(2).sum() + (e_r * wts).sum()).backward()
    return n_r.detach(), e_r.detach(), Xv_r.grad, Xe_r.grad, [W.grad for W in Ws], [b.grad for b in bs]


def _assert_step(got, ref, case):
    names = ["node", "edge", "dXv", "dXe"]
    pairs = list(zip(names, got[:4], ref[:4]))
    for l, (a, b) in enumerate(zip(got[4], ref[4])):
        pairs.append((f"dW[{l}]", a, b))
    for l, (a, b) in enumerate(zip(got[5], ref[5])):
        pairs.append((f"db[{l}]", a, b))
    for what, a, b in pairs:
        print(f"FUSEDDROP block {norm_err(a, b):.3e} {what} {case}")
        assert_parity(a, b, TOL, f"{what} {case}")


@pytest.mark.parametrize("reduce,residual", [("sum", True), ("mean", True), ("max", True), ("sum", False),
                                             ("mean", False), ("max", False)])
@pytest.mark.parametrize("h,n", [(48, 24), (400, 8)])
def test_block_fused_dropout_forward_and_grads(h, n, reduce, residual):
    """fp32 ChempropBlock in train(): one fused launch per layer (as without dropout), forward and all
    gradients against the fp64 oracle with the same masks."""
    from notorch_amd.nn import ChempropBlock

    G = _graph(f"qm9-{n}")[0]
    depth = 3 if h == 48 else 2
    Xv, Xe = _features(G, h)
    torch.manual_seed(1)
    blk = ChempropBlock(h, depth=depth, dropout=P, reduce=reduce, residual=residual).to(DEV).train()
    got = _train_step(blk, G, Xv, Xe, 99)
    info = got[-1]
    assert info["fused"] is True and "dropout in the epilogue" in info["kernel"], info
    masks = _block_masks(99, P, G.num_edges, h, depth)
    assert all(0.6 < (m != 0).double().mean().item() < 0.9 for m in masks)
    _assert_step(got, _oracle_step(blk, G, Xv, Xe, masks, reduce, residual), f"h={h} {reduce} residual={residual}")


@pytest.mark.parametrize("name,h", [("qm9-24", 48), ("b32", 48), ("b33", 48), ("dir", 48)])
def test_block_fused_dropout_128_row_walk_and_topologies(monkeypatch, name, h):
    """NW4_MAX_EDGES = 0 sends h <= 320 to the 128-row walk; b33 runs the hub sub-runs + hub_combine,
    dir the zero fills."""
    from notorch_amd.nn.gnn import _engine

    monkeypatch.setattr(_engine, "NW4_MAX_EDGES", 0)
    top = None if name.startswith("qm9") else T.block_graph(name)
    G = _graph(name)[0]
    Xv, Xe = T.embed(G.node_feats, G.edge_feats, h)
    blk = T.make_block(h, 2, "ReLU", "sum", w_var=1 / 16, dropout=P).to(DEV).train()
    got = _train_step(blk, G, Xv, Xe, 99)
    info = got[-1]
    assert info["fused"] is True and "128-row tiles, dropout in the epilogue" in info["kernel"], info
    masks = _block_masks(99, P, G.num_edges, h, 2)
    assert top is None or top.E == G.num_edges
    _assert_step(got, _oracle_step(blk, G, Xv, Xe, masks, "sum", True), f"{name} 128-row")


@pytest.mark.parametrize("dtype,h,n", [(torch.float32, 48, 24), (torch.float32, 400, 8), (BF, 64, 24), (BF, 640, 8)])
def test_path_taken_switch_and_old_path_agreement(monkeypatch, dtype, h, n):
    """A train() block with dropout is fused wherever the same block without dropout is (bf16 above
    h = 512 only with the engine's gate BF16_FUSED_DROPOUT_MAX_H raised: that class is not timed, and by
    default keeps the unfused path); NT_FUSED_DROPOUT=0 restores the unfused update +
    nt_dropout_residual, whose forward agrees."""
    from notorch_amd.nn import ChempropBlock
    from notorch_amd.nn.gnn import _engine

    gated = dtype == BF and h > 512
    assert _engine.BF16_FUSED_DROPOUT_MAX_H == 512

    G = _graph(f"qm9-{n}")[0]
    Xv, Xe = (t.to(dtype) for t in _features(G, h))
    torch.manual_seed(1)
    blk = ChempropBlock(h, depth=2, dropout=P).to(DEV, dtype).train()
    plain = ChempropBlock(h, depth=2, dropout=0.0).to(DEV, dtype).train()
    plain.load_state_dict(blk.state_dict())
    Gd = G.update(node_feats=Xv, edge_feats=Xe).to(DEV)

    def run(b, seed=5):
        _engine.LAST_UPDATE_INFO.clear()
        torch.manual_seed(seed)
        with torch.no_grad():
            o = b(Gd)
        return o.node_feats, o.edge_feats, dict(_engine.LAST_UPDATE_INFO)

    monkeypatch.delenv("NT_FUSED_DROPOUT", raising=False)
    _, _, info_plain = run(plain)
    if gated:  # the default gate: the unfused update on the column-pass kernel, as before
        info_d = run(blk)[2]
        assert info_d["fused"] is False and "dropout" not in info_d["kernel"] and "wide" in info_d["kernel"], info_d
        monkeypatch.setattr(_engine, "BF16_FUSED_DROPOUT_MAX_H", 8192)
    node, edge, info = run(blk)
    assert info_plain["fused"] is True and info["fused"] is True, (info_plain, info)
    assert info["rows"] == info_plain["rows"] and "dropout in the epilogue" in info["kernel"], info
    assert "dropout" not in info_plain["kernel"]
    monkeypatch.setenv("NT_FUSED_DROPOUT", "0")
    node_u, edge_u, info_u = run(blk)
    assert info_u["fused"] is False and "dropout" not in info_u["kernel"], info_u
    tol = TOL if dtype == torch.float32 else BLOCK_TOL
    assert_parity(node.float(), node_u.float(), tol, "node vs NT_FUSED_DROPOUT=0")
    assert_parity(edge.float(), edge_u.float(), tol, "edge vs NT_FUSED_DROPOUT=0")
    # NT_FUSED=0 still forces the unfused path, whatever NT_FUSED_DROPOUT says
    monkeypatch.setenv("NT_FUSED", "0")
    monkeypatch.delenv("NT_FUSED_DROPOUT", raising=False)
    assert run(blk)[2]["fused"] is False


def test_bf16_hub_graph_stays_unfused():
    """bf16 hub graphs have no tile plan: dropout stays on the unfused path there."""
    from test_gpu_bf16_wide import _block_vs_torch_bf16

    info = _block_vs_torch_bf16("polymer", 2, 64, 2, seed=5, dropout_seed=99, dropout=P)
    assert info["fused"] is False and "dropout" not in info["kernel"], info


@pytest.mark.parametrize("h,n", [(64, 24), (640, 8)])
@pytest.mark.parametrize("opts", [dict(), dict(reduce="mean", residual=False)])
def test_block_fused_dropout_bf16_storage(monkeypatch, h, n, opts):
    """bf16 storage: no further from fp64 than 2 x torch's own bf16 evaluation with the same masks, and
    within the absolute block tolerance (tests/test_gpu_bf16_wide.py's yardstick).  h = 640 with the
    engine's gate raised (by default that class stays unfused)."""
    from notorch_amd.nn.gnn import _engine
    from test_gpu_bf16_wide import _block_vs_torch_bf16

    monkeypatch.setattr(_engine, "BF16_FUSED_DROPOUT_MAX_H", 8192)
    info = _block_vs_torch_bf16("qm9", n, h, 3, seed=4, dropout_seed=99, dropout=P, **opts)
    assert info["fused"] is True and info["kernel_short"] == "update_bf16", info
    assert "dropout in the epilogue" in info["kernel"] and (h <= 512 or "wide" in info["kernel"]), info


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("h,n", [(64, 24), (640, 8)])
def test_block_fused_dropout_under_bf16_autocast(monkeypatch, h, n):
    """An fp32 block under torch.autocast(bfloat16): the bf16 kernels with dropout in the epilogue;
    the forward by the bf16 yardstick on the unrounded fp32 values, fp32 leaves get fp32 gradients.
    h = 640 with the engine's gate raised (by default that class stays unfused)."""
    from notorch_amd.nn import ChempropBlock
    from notorch_amd.nn.gnn import _engine

    monkeypatch.setattr(_engine, "BF16_FUSED_DROPOUT_MAX_H", 8192)
    G = _graph(f"qm9-{n}")[0]
    depth = 2
    Xv, Xe = _features(G, h)
    torch.manual_seed(1)
    blk = ChempropBlock(h, depth=depth, dropout=P).to(DEV).train()
    masks = _block_masks(99, P, G.num_edges, h, depth)
    Ws, bs = dmpnn_ref.block_params(blk)
    ei, rev = G.edge_index.to(DEV), G.rev_index.to(DEV)

    def restated(dtype):
        with torch.inference_mode():
            return dmpnn_ref.chemprop_block(Xv.to(DEV, dtype), Xe.to(DEV, dtype), ei, rev,
                                            [W.detach().to(DEV, dtype) for W in Ws],
                                            [b.detach().to(DEV, dtype) for b in bs],
                                            dropout_masks=[m.to(DEV, dtype) for m in masks])

    truth, torch_bf16 = restated(torch.float64), restated(BF)
    Xv_d, Xe_d = Xv.to(DEV).requires_grad_(True), Xe.to(DEV).requires_grad_(True)
    _engine.LAST_UPDATE_INFO.clear()
    torch.manual_seed(99)
    with torch.autocast("cuda", dtype=BF):
        out = blk(G.update(node_feats=Xv_d, edge_feats=Xe_d).to(DEV))
    info = dict(_engine.LAST_UPDATE_INFO)
    assert info["fused"] is True and info["kernel_short"] == "update_bf16", info
    assert "dropout in the epilogue" in info["kernel"], info
    for what, d, t, ref in zip(("node", "edge"), (out.node_feats, out.edge_feats), torch_bf16, truth):
        assert d.dtype == BF, what
        e_dev, e_t, l_dev, l_t = norm_err(d, ref), norm_err(t, ref), _rel_l2(d, ref), _rel_l2(t, ref)
        print(f"FUSEDDROP autocast h={h} {what}: device max {e_dev:.3e} L2 {l_dev:.3e}; torch bf16 max {e_t:.3e} "
              f"L2 {l_t:.3e}")
        assert e_dev <= BF16_FACTOR * e_t and l_dev <= BF16_FACTOR * l_t, what
        assert e_dev <= BLOCK_TOL, what
    wts = torch.linspace(-1, 1, h, device=DEV)
    (out.node_feats.float().pow(2).sum() + (out.edge_feats.float() * wts).sum()).backward()
    leaves = [Xv_d, Xe_d] + [q for l in blk._chemprop_layers() for q in (l.linear.weight, l.linear.bias)]
    for q in leaves:
        assert q.grad is not None and q.grad.dtype == torch.float32 and torch.isfinite(q.grad).all()
        assert q.grad.abs().max().item() > 0


@pytest.mark.parametrize("dtype,h", [(torch.float32, 48), (BF, 64)])
def test_fused_dropout_reproducibility_and_eval(dtype, h):
    """torch.manual_seed reproduces the masks bit for bit; another seed gives others; eval() is the
    dropout-free block."""
    from notorch_amd.nn import ChempropBlock
    from notorch_amd.nn.gnn import _engine

    G = _graph("qm9-8")[0]
    Xv, Xe = (t.to(dtype) for t in _features(G, h))
    Gd = G.update(node_feats=Xv, edge_feats=Xe).to(DEV)
    torch.manual_seed(1)
    blk = ChempropBlock(h, depth=2, dropout=0.5).to(DEV, dtype)
    plain = ChempropBlock(h, depth=2, dropout=0.0).to(DEV, dtype)
    plain.load_state_dict(blk.state_dict())
    with torch.no_grad():
        ev = blk.eval()(Gd)
        ref = plain.eval()(Gd)
        assert torch.equal(ev.edge_feats, ref.edge_feats) and torch.equal(ev.node_feats, ref.node_feats)
        torch.manual_seed(3)
        t1 = blk.train()(Gd)
        assert _engine.LAST_UPDATE_INFO["fused"] is True and "dropout" in _engine.LAST_UPDATE_INFO["kernel"]
        torch.manual_seed(3)
        t2 = blk(Gd)
        torch.manual_seed(4)
        t3 = blk(Gd)
    assert torch.equal(t1.edge_feats, t2.edge_feats) and torch.equal(t1.node_feats, t2.node_feats)
    assert not torch.equal(t1.edge_feats, t3.edge_feats) and not torch.equal(t1.edge_feats, ev.edge_feats)


@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_embedded_block_fused_dropout(reduce):
    """EmbeddedChempropBlock with dropout: the fused launch per layer, gradients (tables included)
    against the fp64 oracle with the block's masks, as tests/test_gpu_embed_backward.py."""
    from notorch_amd.nn import ChempropBlock, EmbeddedChempropBlock, GraphEmbedding, Sum
    from notorch_amd.nn.gnn import _engine

    from notorch_amd.data.synth import make_batch

    G, Gd = make_batch("qm9", 24, seed=4).collate("nodes"), make_batch("qm9", 24, seed=4).collate("nodes").to(DEV)
    h, depth = 48, 2
    torch.manual_seed(3)
    emb = GraphEmbedding(42, 13, h)
    blk = ChempropBlock(hidden_dim=h, depth=depth, dropout=P, reduce=reduce)
    enc = EmbeddedChempropBlock(emb, blk).to(DEV).train()
    _engine.LAST_UPDATE_INFO.clear()
    torch.manual_seed(11)
    out = enc(Gd)
    info = dict(_engine.LAST_UPDATE_INFO)
    assert info["fused"] is True and "dropout in the epilogue" in info["kernel"], info
    Sum()(out).float().pow(2).sum().backward()
    layers = blk._chemprop_layers()
    params = ([emb.node.weight, emb.edge.weight] + [l.linear.weight for l in layers] + [l.linear.bias for l in layers])
    masks = _block_masks(11, P, G.num_edges, h, depth)
    ps = [q.detach().double().cpu().requires_grad_(True) for q in params]
    Tv, Te, Ws, bs = ps[0], ps[1], ps[2:2 + depth], ps[2 + depth:]
    n, _ = dmpnn_ref.chemprop_block(Tv[G.node_feats].sum(1), Te[G.edge_feats].sum(1), G.edge_index, G.rev_index, Ws,
                                    bs, reduce=reduce, dropout_masks=masks)
    assert_parity(out.node_feats, n, TOL, "node")
    dmpnn_ref.readout(n, G.batch_node_index, len(G), "sum").pow(2).sum().backward()
    for i, (q, r) in enumerate(zip(params, ps)):
        assert_parity(q.grad, r.grad, TOL, f"embedded grad {i}")


def test_standalone_layer_fused_dropout_matches_oracle():
    from notorch_amd.nn import ChempropLayer
    from notorch_amd.nn.gnn import _engine

    G = _graph("qm9-8")[0]
    h, p = 48, 0.25
    torch.manual_seed(0)
    H = torch.randn(G.num_edges, h)
    layer = ChempropLayer(h, dropout=p).to(DEV).train()
    (mask,) = _block_masks(7, p, G.num_edges, h, 1)
    ei, rev = G.edge_index.clone(), G.rev_index.clone()
    _engine.LAST_UPDATE_INFO.clear()
    torch.manual_seed(7)
    with torch.no_grad():
        got = layer(H.to(DEV), torch.zeros(G.num_nodes, h, device=DEV), ei.to(DEV), rev.to(DEV))
    info = dict(_engine.LAST_UPDATE_INFO)
    assert info["fused"] is True and "dropout in the epilogue" in info["kernel"], info
    W = layer.linear.weight.detach().double().cpu()
    b = layer.linear.bias.detach().double().cpu()
    ref = dmpnn_ref.chemprop_layer(H.double(), torch.zeros(G.num_nodes, h, dtype=torch.float64), ei, rev, W, b) * mask
    assert torch.equal(got.cpu()[mask == 0], torch.zeros_like(got.cpu()[mask == 0]))
    assert_parity(got, ref, TOL, "layer dropout")
