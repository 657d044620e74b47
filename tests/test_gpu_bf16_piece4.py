"""GPU: the bf16 layer kernel on rows of whole 8-byte pieces (csrc/bf16.hip, update_bf16_kernel<.., W = 4, ..>:
h % 4 == 0, h <= 512) and the W = 4 element kernels of the same forward.

The yardstick of every launch is code older than these instances: the same launch at hp = h + 4 on the
16-byte instances (h % 8 == 4, so hp % 8 == 0), with H, S, W (both dimensions) and the bias zero-padded
to hp.  For every h used here both shapes have the same KS = ceil(h / 32) and NTn = ceil(h / 16), and
the padded operands are the zeros the kernel supplies itself past a row's end, so every MFMA sees
identical fragments: the first h columns of H_out and S_out must be equal bit for bit (compared as
int16).  Activations with act(0) = 0 only (ReLU, Identity, SiLU): the padded columns of the message stay 0.
"""
import functools

import pytest
import torch
import torch.nn as nn

import topology
from oracle import dmpnn_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
H_LIST = [4, 12, 36, 68, 260, 300, 508]
PIECE4 = b"update_bf16_kernel: two 4-wave workgroups per CU, 64-edge tiles, 8-byte row pieces"
PLAIN = b"update_bf16_kernel: two 4-wave workgroups per CU, 64-edge tiles"  # the 16-byte and the scalar instances
_ACTS = {"relu": nn.ReLU, "identity": nn.Identity, "silu": nn.SiLU}


def _K():
    from notorch_amd import kernels

    return kernels


def _last_kernel():
    return _K()._lib.load().nt_last_kernel()


def _rand_bf16(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(BF)


def _pad(t, hp, dims=(-1,)):
    """t zero-padded to hp along dims."""
    for d in dims:
        shape = list(t.shape)
        shape[d] = hp - t.shape[d]
        t = torch.cat([t, torch.zeros(shape, dtype=t.dtype, device=t.device)], dim=d)
    return t.contiguous()


def _bits(t, h):
    return t[:, :h].contiguous().view(torch.int16)


def _same_ks_ntn(h):
    hp = h + 4
    assert h % 8 == 4 and (h + 31) // 32 == (hp + 31) // 32 and (h + 15) // 16 == (hp + 15) // 16
    return hp


class _Graph:
    """A graph on the device with its dst CSR and 64-row tile plan."""

    def __init__(self, G):
        K = _K()
        self.V, self.E = G.num_nodes, G.num_edges
        self.src_cpu, self.dst_cpu, self.rev_cpu = G.edge_index[0], G.edge_index[1], G.rev_index
        self.src, self.rev = self.src_cpu.to(DEV), self.rev_cpu.to(DEV)
        self.dst_ptr, self.perm = K.csr_build(self.dst_cpu.contiguous().to(DEV), self.V)
        deg = (self.dst_ptr[1:] - self.dst_ptr[:-1]).cpu()
        self.maxdeg = int(deg.max())
        self.plan = K.tile_plan(self.dst_ptr, self.E, self.maxdeg)
        self.zero_fill = bool((deg == 0).any())


@functools.lru_cache(maxsize=None)
def _graph(name):
    from notorch_amd.data.models.graph import BatchedGraph, Graph
    from notorch_amd.data.synth import make_batch

    if name == "zinc":
        g = _Graph(make_batch("zinc", 40, seed=3).collate("nodes"))
        assert g.E % 64 != 0 and not g.zero_fill
        return g
    if name == "isolated":  # nodes without in-edges (and one graph without edges)
        gs = [
            Graph(torch.zeros(3, 7, dtype=torch.long), torch.zeros(4, 2, dtype=torch.long),
                  torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), torch.tensor([1, 0, 3, 2])),
            Graph(torch.zeros(1, 7, dtype=torch.long), torch.zeros(0, 2, dtype=torch.long),
                  torch.zeros(2, 0, dtype=torch.long), torch.zeros(0, dtype=torch.long)),
            Graph(torch.zeros(2, 7, dtype=torch.long), torch.zeros(2, 2, dtype=torch.long),
                  torch.tensor([[0, 1], [1, 0]]), torch.tensor([1, 0])),
        ]
        g = _Graph(BatchedGraph.from_graphs(gs, rev_offset="edges"))
        assert g.zero_fill
        return g
    if name == "deg32":  # directed, in-degrees 0..32: runs of one node that fill half a tile
        g = _Graph(topology.directed([32, 1, 17, 0, 5, 31, 2, 9, 32, 3, 0, 12, 24, 7, 1, 16, 32, 4], seed=5).collate())
        assert g.maxdeg == 32
        return g
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _operands(name, h):
    """(H, S, W, b) in bf16 on the device for graph `name`, and their zero-padded copies at hp = h + 4."""
    g = _graph(name)
    hp = _same_ks_ntn(h)
    H, S = _rand_bf16(g.E, h, seed=4 + h).to(DEV), _rand_bf16(g.V, h, seed=5 + h).to(DEV)
    W = (_rand_bf16(h, h, seed=6 + h).float() / h ** 0.5).to(BF).to(DEV)
    b = _rand_bf16(h, seed=7 + h).to(DEV)
    return (H, S, W, b), (_pad(H, hp), _pad(S, hp), _pad(W, hp, (0, 1)), _pad(b, hp))


def _fused(g, ops, act, agg, reduce, resbias, kernel, out=None, S_out=None):
    """One fused launch over g's 64-row plan: (H_out, S_out)."""
    K = _K()
    H, S, W, b = ops
    Hn, Sn = K.dmpnn_update_fused(H, S, g.src, g.rev, K.pack_weights(W), b if resbias else None, residual=resbias,
                                  act=K.act_code(_ACTS[act]()), plan=g.plan, tile_rows=64, max_in_degree=g.maxdeg,
                                  perm=g.perm, reduce=reduce, agg_act=K.act_code(_ACTS[agg]()),
                                  zero_fill=g.zero_fill, out=out, S_out=S_out)
    assert _last_kernel() == kernel, _last_kernel()
    return Hn, Sn


def _check_fused(name, h, act, agg, reduce, resbias):
    g = _graph(name)
    ops, padded = _operands(name, h)
    Hn, Sn = _fused(g, ops, act, agg, reduce, resbias, PIECE4)
    Hy, Sy = _fused(g, padded, act, agg, reduce, resbias, PLAIN)
    assert Hn.dtype == BF and Hn.shape == (g.E, h) and Sn.shape == (g.V, h)
    assert torch.equal(_bits(Hn, h), _bits(Hy, h)), f"H_out {name} h={h} {act} {agg} {reduce} {resbias}"
    assert torch.equal(_bits(Sn, h), _bits(Sy, h)), f"S_out {name} h={h} {act} {agg} {reduce} {resbias}"
    assert torch.isfinite(Hn.float()).all() and torch.isfinite(Sn.float()).all()
    return Sn


# ------------------------------------------------------------------ 1. fused launch
# agg = act: the next layer's aggregation (AGG 2); agg = identity: the final node scatter (AGG 1)
@pytest.mark.parametrize("resbias", [True, False])
@pytest.mark.parametrize("agg_is_act", [True, False])
@pytest.mark.parametrize("act", ["relu", "silu"])
@pytest.mark.parametrize("h", [36, 300])
def test_fused_every_mode(h, act, agg_is_act, resbias):
    for reduce in ("sum", "mean", "max", "min"):
        _check_fused("zinc", h, act, act if agg_is_act else "identity", reduce, resbias)


# 4: a lone half piece; 12: a whole piece + a half; 68: the wave's second column tile; 260: a second
# 256-column epilogue pass of 4 columns; 508: eight column tiles per wave, both passes, half piece last
@pytest.mark.parametrize("agg", ["relu", "identity"])
@pytest.mark.parametrize("h", [4, 12, 68, 260, 508])
def test_fused_other_sizes(h, agg):
    _check_fused("zinc", h, "relu", agg, "sum", True)


@pytest.mark.parametrize("h", [12, 300])
def test_fused_nodes_without_in_edges(h):
    Sn = _check_fused("isolated", h, "relu", "relu", "sum", True)
    assert (Sn[3] == 0).all()  # the edgeless graph's node


@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_fused_in_degrees_up_to_32(reduce):
    _check_fused("deg32", 300, "relu", "relu", reduce, True)
    _check_fused("deg32", 36, "identity", "identity", reduce, False)


# ------------------------------------------------------------------ 2. plain and dense modes
@pytest.mark.parametrize("h", H_LIST)
def test_plain_update(h):
    K = _K()
    g = _graph("zinc")
    relu = K.act_code(nn.ReLU())
    for resbias in (True, False):
        outs = []
        for (H, S, W, b), kernel in zip(_operands("zinc", h), (PIECE4, PLAIN)):
            outs.append(K.dmpnn_update(H, S, g.src, g.rev, K.pack_weights(W), b if resbias else None,
                                       residual=resbias, act=relu))
            assert _last_kernel() == kernel, _last_kernel()
        assert torch.equal(_bits(outs[0], h), _bits(outs[1], h)), f"h={h} resbias={resbias}"


@pytest.mark.parametrize("h", [36, 300])
def test_plain_update_equals_the_scalar_rows_kernel(h):
    """The plain launch on 8-byte pieces gives the bits of the element-by-element instance (W = 1), which
    rows that are not 16-byte aligned still take: the same operands 8 bytes into their allocations."""
    K = _K()
    g = _graph("zinc")
    (H, S, W, b), _ = _operands("zinc", h)

    def off(t):  # the same values, 8 bytes past a 16-byte boundary
        buf = torch.empty(t.numel() + 4, dtype=BF, device=DEV)
        v = buf[4:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 8 and v.is_contiguous()
        return v

    Wp = K.pack_weights(W)
    for act in ("relu", "silu"):
        a = K.act_code(_ACTS[act]())
        vec = K.dmpnn_update(H, S, g.src, g.rev, Wp, b, residual=True, act=a)
        assert _last_kernel() == PIECE4
        scalar = K.dmpnn_update(off(H), off(S), g.src, g.rev, Wp, off(b), residual=True, act=a)
        assert _last_kernel() == PLAIN
        assert torch.equal(vec.view(torch.int16), scalar.view(torch.int16)), (h, act)


@pytest.mark.parametrize("h", H_LIST)
def test_dense_matmul(h):
    K = _K()
    (H, _, W, _), (Hp, _, Wpad, _) = _operands("zinc", h)
    assert H.shape[0] % 64 != 0
    got = K.dense_matmul(H, K.pack_weights(W))
    assert _last_kernel() == PIECE4
    yard = K.dense_matmul(Hp, K.pack_weights(Wpad))
    assert _last_kernel() == PLAIN
    assert torch.equal(_bits(got, h), _bits(yard, h))
    ref = H.float().cpu() @ W.float().cpu().T
    # the operands are bf16 already: one bf16 rounding of the result (<= 2^-9 of the element) + the fp32 order
    assert (got.float().cpu() - ref).abs().max() <= 2.0 ** -8 * ref.abs().max()


# ------------------------------------------------------------------ 3. several tiles per workgroup
def test_fused_persistent_walk():
    """More tiles than resident workgroups (two per CU) and ntiles % 8 != 0: ragged per-XCD chunks and
    several tiles per workgroup, the index pipeline running from tile to tile."""
    from notorch_amd.data.synth import make_batch

    K = _K()
    h = 36
    hp = _same_ks_ntn(h)
    slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    per_mol = make_batch("qm9", 64, seed=11).collate("nodes").num_edges / 64
    n0 = int((slots + 4) * 64 / per_mol)
    for n in range(n0, 2 * n0, 7):
        g = _Graph(make_batch("qm9", n, seed=11).collate("nodes"))
        if g.plan[1] % 8 != 0 and g.plan[1] > slots + 3:
            break
    else:
        pytest.fail("no batch size in range gives the wanted tile count")
    H, S = _rand_bf16(g.E, h, seed=n).to(DEV), _rand_bf16(g.V, h, seed=n + 1).to(DEV)
    W = (_rand_bf16(h, h, seed=2).float() / h ** 0.5).to(BF).to(DEV)
    b = _rand_bf16(h, seed=3).to(DEV)
    Hn, Sn = _fused(g, (H, S, W, b), "relu", "relu", "sum", True, PIECE4)
    Hy, Sy = _fused(g, (_pad(H, hp), _pad(S, hp), _pad(W, hp, (0, 1)), _pad(b, hp)), "relu", "relu", "sum", True,
                    PLAIN)
    assert torch.equal(_bits(Hn, h), _bits(Hy, h)), f"walk H ntiles={g.plan[1]}"
    assert torch.equal(_bits(Sn, h), _bits(Sy, h)), f"walk S ntiles={g.plan[1]}"


# ------------------------------------------------------------------ 4. bounds
@pytest.mark.parametrize("h", [12, 300])
def test_fused_stays_inside_its_rows(h):
    """H, S, H_out and S_out as the leading rows of allocations two rows longer: NaN behind the inputs,
    a sentinel behind the outputs."""
    g = _graph("zinc")
    (H, S, W, b), _ = _operands("zinc", h)
    sentinel = -7.0

    def longer(t, fill):
        buf = torch.full((t.shape[0] + 2, h), fill, dtype=BF, device=DEV)
        buf[:t.shape[0]].copy_(t)
        return buf

    Hb, Sb = longer(H, float("nan")), longer(S, float("nan"))
    for agg in ("relu", "identity"):
        Hn, Sn = _fused(g, (H, S, W, b), "relu", agg, "sum", True, PIECE4)
        Ob = torch.full((g.E + 2, h), sentinel, dtype=BF, device=DEV)
        SOb = torch.full((g.V + 2, h), sentinel, dtype=BF, device=DEV)
        Hm, Sm = _fused(g, (Hb[:g.E], Sb[:g.V], W, b), "relu", agg, "sum", True, PIECE4, out=Ob[:g.E],
                        S_out=SOb[:g.V])
        assert torch.equal(Hm.view(torch.int16), Hn.view(torch.int16))
        assert torch.equal(Sm.view(torch.int16), Sn.view(torch.int16))
        assert (Ob[g.E:] == sentinel).all() and (SOb[g.V:] == sentinel).all()


# ------------------------------------------------------------------ 5. masking of the half piece
def _compare_except(g, h, ops, padded, bad_rows, resbias):
    """Fused launch against the padded yardstick on every row but bad_rows (edges) and their
    destination nodes; the compared rows are finite."""
    Hn, Sn = _fused(g, ops, "relu", "relu", "sum", resbias, PIECE4)
    Hy, Sy = _fused(g, padded, "relu", "relu", "sum", resbias, PLAIN)
    keep_e = torch.ones(g.E, dtype=torch.bool)
    keep_e[bad_rows] = False
    keep_v = torch.ones(g.V, dtype=torch.bool)
    keep_v[g.dst_cpu[bad_rows]] = False
    assert keep_e.sum() >= g.E - 4 and keep_v.sum() >= g.V - 4
    keep_e, keep_v = keep_e.to(DEV), keep_v.to(DEV)
    assert torch.isfinite(Hn[keep_e].float()).all() and torch.isfinite(Sn[keep_v].float()).all()
    assert torch.equal(_bits(Hn, h)[keep_e], _bits(Hy, h)[keep_e])
    assert torch.equal(_bits(Sn, h)[keep_v], _bits(Sy, h)[keep_v])
    assert not torch.isfinite(Hn[~keep_e].float()).all()  # the excluded rows did read the Inf


@pytest.mark.parametrize("h", [12, 300])
def test_half_piece_never_reads_the_next_row_of_S(h):
    """S[v, :4] = +Inf sits where the second half of row v - 1's last piece would be."""
    g = _graph("zinc")
    hp = _same_ks_ntn(h)
    (H, S, W, b), _ = _operands("zinc", h)
    outdeg = torch.bincount(g.src_cpu, minlength=g.V)
    v = next(v for v in range(1, g.V) if 1 <= outdeg[v] <= 4 and outdeg[v - 1] > 0)
    S = S.clone()
    S[v, :4] = float("inf")
    bad = torch.nonzero(g.src_cpu == v).flatten()
    _compare_except(g, h, (H, S, W, b), (_pad(H, hp), _pad(S, hp), _pad(W, hp, (0, 1)), _pad(b, hp)), bad, True)


@pytest.mark.parametrize("h", [12, 300])
def test_half_piece_never_reads_the_next_row_of_H(h):
    """H[q, :4] = +Inf behind row q - 1; without the residual, so that only the rows with rev == q see it."""
    g = _graph("zinc")
    hp = _same_ks_ntn(h)
    (H, S, W, b), _ = _operands("zinc", h)
    q = next(q for q in range(1, g.E) if (g.rev_cpu == q - 1).any() and (g.rev_cpu == q).any())
    H = H.clone()
    H[q, :4] = float("inf")
    bad = torch.nonzero(g.rev_cpu == q).flatten()
    _compare_except(g, h, (H, S, W, b), (_pad(H, hp), _pad(S, hp), _pad(W, hp, (0, 1)), _pad(b, hp)), bad, False)


# ------------------------------------------------------------------ 6. element kernels
@pytest.mark.parametrize("h", [4, 12, 36, 300])
def test_element_kernels(h):
    """dmpnn_init, segment_reduce and dmpnn_init_mixed on 8-byte pieces: the CPU formulas of
    tests/test_gpu_bf16.py and tests/test_gpu_autocast.py (one rounding of the fp32 sum), and the padded
    launch on 16-byte pieces."""
    K = _K()
    g = _graph("zinc")
    hp = h + 4
    src, dst = g.src_cpu, g.dst_cpu
    relu = K.act_code(nn.ReLU())
    Xv, Xe = _rand_bf16(g.V, h, seed=1 + h), _rand_bf16(g.E, h, seed=2 + h)
    ref_H0 = (Xv.float()[src] + Xe.float()).to(BF)
    H0, S = K.dmpnn_init(Xv.to(DEV), Xe.to(DEV), g.src, g.dst_ptr, g.perm)
    assert torch.equal(H0.cpu(), ref_H0)
    assert torch.equal(S.cpu(), dmpnn_ref.scatter(torch.relu(ref_H0.float()), dst, g.V, "sum").to(BF))
    H0p, Sp = K.dmpnn_init(_pad(Xv, hp).to(DEV), _pad(Xe, hp).to(DEV), g.src, g.dst_ptr, g.perm)
    assert torch.equal(_bits(H0, h), _bits(H0p, h)) and torch.equal(_bits(S, h), _bits(Sp, h))
    H0_only, none = K.dmpnn_init(Xv.to(DEV), Xe.to(DEV), g.src)
    assert none is None and torch.equal(H0_only.cpu(), ref_H0)

    X = _rand_bf16(g.E, h, seed=3 + h)
    for reduce in ("sum", "mean", "max", "min"):
        out = K.segment_reduce(X.to(DEV), g.dst_ptr, g.perm, g.V, reduce=reduce, act=relu)
        assert torch.equal(out.cpu(), dmpnn_ref.scatter(torch.relu(X.float()), dst, g.V, reduce).to(BF)), reduce
        outp = K.segment_reduce(_pad(X, hp).to(DEV), g.dst_ptr, g.perm, g.V, reduce=reduce, act=relu)
        assert torch.equal(_bits(out, h), _bits(outp, h)), reduce

    gen = torch.Generator().manual_seed(9 + h)
    Fv, Fe = torch.randn(g.V, h, generator=gen), torch.randn(g.E, h, generator=gen)
    ref_M0 = (Fv[src] + Fe).to(BF)  # added in fp32, rounded once
    for reduce in ("sum", "max"):
        M0, MS = K.dmpnn_init_mixed(Fv.to(DEV), Fe.to(DEV), g.src, g.dst_ptr, g.perm, act=relu, reduce=reduce)
        assert torch.equal(M0.cpu(), ref_M0)
        assert torch.equal(MS.cpu(), dmpnn_ref.scatter(torch.relu(ref_M0.float()), dst, g.V, reduce).to(BF))
        M0p, MSp = K.dmpnn_init_mixed(_pad(Fv, hp).to(DEV), _pad(Fe, hp).to(DEV), g.src, g.dst_ptr, g.perm, act=relu,
                                      reduce=reduce)
        assert torch.equal(_bits(M0, h), _bits(M0p, h)) and torch.equal(_bits(MS, h), _bits(MSp, h))
    M0_only, none = K.dmpnn_init_mixed(Fv.to(DEV), Fe.to(DEV), g.src)
    assert none is None and torch.equal(M0_only.cpu(), ref_M0)


# ------------------------------------------------------------------ 7. through the modules
def _block_run(blk, Gd, autocast=False):
    from notorch_amd.nn.gnn import _engine

    _engine.LAST_UPDATE_INFO.clear()
    with torch.no_grad(), torch.autocast("cuda", dtype=BF, enabled=autocast):
        out = blk(Gd)
    return out, dict(_engine.LAST_UPDATE_INFO), _last_kernel()


def _block_case(h, reduce, dtype, **opts):
    from notorch_amd.data.synth import make_batch
    from notorch_amd.nn import ChempropBlock

    G = make_batch("zinc", 40, seed=9).collate("nodes")
    torch.manual_seed(2)
    blk = ChempropBlock(hidden_dim=h, depth=3, reduce=reduce, **opts).eval().to(dtype).to(DEV)
    Xv, Xe = torch.randn(G.num_nodes, h).to(dtype), torch.randn(G.num_edges, h).to(dtype)
    return blk, G.update(node_feats=Xv, edge_feats=Xe).to(DEV)


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("h", [36, 300])
def test_block_bf16_fused_bit_identical_to_unfused(monkeypatch, h, reduce):
    from notorch_amd.nn.gnn import _engine

    blk, Gd = _block_case(h, reduce, BF)
    fused, info, last = _block_run(blk, Gd)
    assert info["fused"] is True and last.endswith(b"8-byte row pieces"), (info, last)
    with monkeypatch.context() as m:
        m.setenv("NT_FUSED", "0")
        unfused, info0, _ = _block_run(blk, Gd)
    assert info0["fused"] is False
    assert torch.equal(fused.edge_feats, unfused.edge_feats) and torch.equal(fused.node_feats, unfused.node_feats)
    # the gate down: the block routes as before it existed, to the same bits
    monkeypatch.setattr(_engine, "BF16_FUSED_PIECE4", False)
    gated, info1, _ = _block_run(blk, Gd)
    assert info1["fused"] is False
    assert torch.equal(fused.edge_feats, gated.edge_feats) and torch.equal(fused.node_feats, gated.node_feats)


def test_block_autocast_h300_fused_bit_identical_to_unfused(monkeypatch):
    from notorch_amd.nn.gnn import _engine

    blk, Gd = _block_case(300, "sum", torch.float32)
    fused, info, last = _block_run(blk, Gd, autocast=True)
    assert fused.edge_feats.dtype == BF
    assert info["fused"] is True and last.endswith(b"8-byte row pieces"), (info, last)
    with monkeypatch.context() as m:
        m.setenv("NT_FUSED", "0")
        unfused, info0, _ = _block_run(blk, Gd, autocast=True)
    assert info0["fused"] is False
    assert torch.equal(fused.edge_feats, unfused.edge_feats) and torch.equal(fused.node_feats, unfused.node_feats)
    monkeypatch.setattr(_engine, "BF16_FUSED_PIECE4", False)
    gated, info1, _ = _block_run(blk, Gd, autocast=True)
    assert info1["fused"] is False
    assert torch.equal(fused.edge_feats, gated.edge_feats) and torch.equal(fused.node_feats, gated.node_feats)


def test_block_with_dropout_stays_unfused():
    from notorch_amd.nn.gnn import _engine

    blk, Gd = _block_case(36, "sum", BF, dropout=0.25)
    blk.train()
    _engine.LAST_UPDATE_INFO.clear()
    torch.manual_seed(5)
    with torch.no_grad():
        out = blk(Gd)
    assert _engine.LAST_UPDATE_INFO["fused"] is False, _engine.LAST_UPDATE_INFO
    assert torch.isfinite(out.edge_feats.float()).all()


def test_training_step_under_autocast_keeps_the_library_backward(monkeypatch):
    """h = 36 under bf16 autocast: the training forward takes the fused launch (the no-grad forward's
    bits); the backward keeps dA and dW on the library GEMMs, as before the 8-byte instances."""
    from notorch_amd import kernels as K
    from notorch_amd.nn import Sum
    from notorch_amd.nn.gnn import _engine

    blk, Gd = _block_case(36, "sum", torch.float32)
    ref, info, _ = _block_run(blk, Gd, autocast=True)
    assert info["fused"] is True

    calls = []
    real = _engine.block_backward
    monkeypatch.setattr(_engine, "block_backward", lambda *a, **k: calls.append(1) or real(*a, **k))

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"{name} called: the backward left the library route")
        return f

    blk.train()
    Xv = Gd.node_feats.clone().requires_grad_(True)
    Xe = Gd.edge_feats.clone().requires_grad_(True)
    Gt = Gd.update(node_feats=Xv, edge_feats=Xe)
    _engine.LAST_UPDATE_INFO.clear()
    with torch.autocast("cuda", dtype=BF):
        out = blk(Gt)
    assert _engine.LAST_UPDATE_INFO["fused"] is True
    assert torch.equal(out.edge_feats, ref.edge_feats) and torch.equal(out.node_feats, ref.node_feats)
    loss = Sum()(out).float().pow(2).sum() + out.edge_feats.float().sum()
    monkeypatch.setattr(K, "weight_grad", refuse("weight_grad"))
    monkeypatch.setattr(K, "dense_matmul", refuse("dense_matmul"))
    loss.backward()
    assert calls == [1]
    for name, leaf in [("Xv", Xv), ("Xe", Xe)] + list(blk.named_parameters()):
        assert leaf.grad is not None and leaf.grad.dtype == leaf.dtype == torch.float32, name
        assert torch.isfinite(leaf.grad).all(), name
