"""GPU parity of the fp32 layer kernel (update_fk_kernel, two-part fp16 split) above hidden 384: the
64-row variant with four column tiles per wave (nt_for(h) > 24) and, above 512, its loop over column
chunks of 32 column tiles (launch_update_fk: nchunks = (NT + 31) / 32), at widths that are no
multiple of the 16-column tile or the 32-deep k-step.

What the widths exercise (NT = nt_for(h) column tiles, ks = ks_for(h) k-steps, KS = ks rounded up to even):

* 388  NT = 25: the first width on the 4-tiles-per-wave variant, one chunk; the last column tile has 4
       valid columns (partial-tile clamp in fk_resid_load / fk_bias_load, masked store); ks = 13 ->
       KS = 14: one padded k-step past the weight image, K tail of 4 (fk_gather clamp, fk_split mask).
* 516  NT = 33: two chunks, the second holding ONE column tile with 4 valid columns, so seven of the
       eight waves are idle in it (fk_load_w's out-of-range offsets); ks = 17 -> KS = 18: the padded
       k-step runs once per chunk; K tail of 4; the engine's row pitch is 520.
* 1028 NT = 65: three chunks, the third a 4-column sliver; ks = 33 -> KS = 34.
* 2400 NT = 150: five chunks, the last with 22 column tiles (waves hold 3 and 2); ks = 75 -> KS = 76.
* 8192 NT = 512: the upper limit, 16 full chunks and 256 k-steps (E = 3, plain launch only).

Oracle: fp64 evaluation of chemprop.py:36-43 / residual.py:27-28 on the CPU (oracle/dmpnn_ref.py for
scatter, block and readout); node values bit-identical to the CPU scatter of the kernel's own H_out
(chemprop.py:37-39); fp32 contract FP32_NORM_TOL throughout.  Every test prints its measured
normalised error.  Measured on an MI355X, plain launch: 4.8e-7 (388), 6.2e-7 (516), 1.2e-6 (1028),
1.4e-6 (2400), 2.2e-6 (8192); fused H_out / S_out: 6.9e-7 / 2.8e-7 .. 8.3e-7 (516), 1.1e-6 / 4.3e-7 ..
1.1e-6 (1028): the error grows about as sqrt(K) and stays under the contract up to the ABI's limit."""
import functools

import pytest
import torch
import torch.nn as nn

from helpers import FP32_NORM_TOL, assert_parity, norm_err
from oracle import dmpnn_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
SENTINEL = -12345.625  # exact in fp32; no kernel output of these tests comes near it

_ACTS = {"relu": (nn.ReLU, torch.relu), "identity": (nn.Identity, lambda x: x),
         "silu": (nn.SiLU, nn.functional.silu), "gelu": (nn.GELU, nn.functional.gelu)}


def _K():
    from notorch_amd import kernels

    return kernels


def _graph(kind="qm9", n=40, seed=0, rev_offset="nodes"):
    from notorch_amd.data.synth import make_batch

    return make_batch(kind, n, seed=seed).collate(rev_offset)


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _check(got, ref, what):
    e = norm_err(got, ref)
    print(f"{what}: normalised max error {e:.3e}")
    assert_parity(got, ref, FP32_NORM_TOL, what)
    return e


def _last_kernel():
    return _K()._lib.load().nt_last_kernel()


def _layout(G):
    """dst CSR, 64-row tile plan, largest in-degree, "some node has no in-edge".  The plan is cut for
    the largest tiles (ncu = 0), not balanced over the CUs: on these small graphs a balanced plan has
    tiles of a few rows, and the four row tiles of a tile and the scan carries between them would not
    run (the block tests run the engine's balanced plans)."""
    K = _K()
    dst_ptr, perm = K.csr_build(G.edge_index[1].contiguous().to(DEV), G.num_nodes)
    deg = (dst_ptr[1:] - dst_ptr[:-1]).cpu()
    maxdeg = int(deg.max())
    plan = K.tile_plan(dst_ptr, G.num_edges, maxdeg, rows=64, ncu=0)
    return dst_ptr, perm, plan, maxdeg, bool((deg == 0).any())


def _ref_layer(G, H, S, W, b, residual, act, agg_act=None, reduce="sum"):
    """fp64 layer: H_out, and S_out = scatter(agg_act(H_out)) when agg_act is given."""
    src, dst, rev = G.edge_index[0], G.edge_index[1], G.rev_index
    A = S.double()[src] - act(H.double())[rev]
    U = nn.functional.linear(A, W.double(), None if b is None else b.double())
    Hn = H.double() + U if residual else U
    return Hn, None if agg_act is None else dmpnn_ref.scatter(agg_act(Hn), dst, G.num_nodes, reduce)


# ------------------------------------------------------------------ 1. one plain launch
@functools.lru_cache(maxsize=None)
def _plain_case(h):
    """Inputs of one plain launch, shared by the cases of one width (E = 746: E % 64 = 42, a partial last
    row tile).  Random S: its first row, which the bias prefetch reads when bias is NULL, is non-zero."""
    G = _graph("qm9", 40, seed=3)
    E, V = G.num_edges, G.num_nodes
    assert E % 64 != 0
    H, S = _rand(E, h, seed=h + 1), _rand(V, h, seed=h + 2)
    W, b = _rand(h, h, seed=h + 3) / h ** 0.5, _rand(h, seed=h + 4)
    assert S[0].abs().min() > 0
    return G, H, S, W, b


@functools.lru_cache(maxsize=None)
def _plain_product(h, act):
    G, H, S, W, b = _plain_case(h)
    A = S.double()[G.edge_index[0]] - _ACTS[act][1](H.double())[G.rev_index]
    return A @ W.double().t()


def _check_plain(h, residual, bias, act="relu"):
    K = _K()
    G, H, S, W, b = _plain_case(h)
    got = K.dmpnn_update(H.to(DEV), S.to(DEV), G.edge_index[0].to(DEV), G.rev_index.to(DEV),
                         K.pack_weights(W.to(DEV)), b.to(DEV) if bias else None, residual=residual,
                         act=K.act_code(_ACTS[act][0]()))
    assert _last_kernel().startswith(b"update_fk_kernel: one 8-wave workgroup per CU, 64-row tiles")
    ref = _plain_product(h, act)
    if bias:
        ref = ref + b.double()
    if residual:
        ref = ref + H.double()
    _check(got, ref, f"update fp32 h={h} act={act} residual={residual} bias={bias}")


# 388: NT = 25, one chunk of the CT = 4 variant, partial last column tile, odd ks, K tail;
# 516: two chunks, the second a lone 4-column tile (seven idle waves), odd ks once per chunk, K tail;
# 1028: three chunks with a 4-column sliver, odd ks; 2400: five chunks, 22 tiles in the last, odd ks.
# (False, None): no bias, so the per-chunk bias prefetch reads S's first row and must not use it.
@pytest.mark.parametrize("h", [388, 516, 1028, 2400])
@pytest.mark.parametrize("residual,bias", [(True, True), (False, None)])
def test_update_fk_wide(h, residual, bias):
    _check_plain(h, residual, bias)


def test_update_fk_wide_runtime_activation():
    """SiLU (the run-time activation variant, ACT = -1) at 516."""
    _check_plain(516, True, True, "silu")


def test_update_fk_wide_h8192():
    """The upper limit the ABI states: 16 full chunks x 256 k-steps, E = 3 (one partial row tile)."""
    K = _K()
    h, V = 8192, 2
    src, rev = torch.tensor([0, 1, 1]), torch.tensor([1, 0, 2])
    H, S = _rand(3, h, seed=1), _rand(V, h, seed=2)
    W, b = _rand(h, h, seed=3) / h ** 0.5, _rand(h, seed=4)
    got = K.dmpnn_update(H.to(DEV), S.to(DEV), src.to(DEV), rev.to(DEV), K.pack_weights(W.to(DEV)), b.to(DEV),
                         residual=True, act=K.act_code(nn.ReLU()))
    assert _last_kernel().startswith(b"update_fk_kernel")
    A = S.double()[src] - torch.relu(H.double())[rev]
    ref = H.double() + A @ W.double().t() + b.double()
    _check(got, ref, f"update fp32 h={h} E=3")


# ------------------------------------------------------------------ 2. fused launch
@functools.lru_cache(maxsize=None)
def _fused_case(h):
    G = _graph("qm9", 48, seed=h)  # E = 886 (not a multiple of 64), 15 tiles: one per workgroup
    E, V = G.num_edges, G.num_nodes
    H, S = _rand(E, h, seed=h + 11), _rand(V, h, seed=h + 12)
    W, b = _rand(h, h, seed=h + 13) / h ** 0.5, _rand(h, seed=h + 14)
    return G, H, S, W, b


def _check_fused(G, H, S, W, b, act, reduce, agg):
    """One fused 64-row launch: H_out, S_out against fp64, S_out bit-identical to the CPU scatter of the
    kernel's own H_out, amax_out = (max|H_out|, max|S_out|) exactly.  Returns (zero_fill, S_out)."""
    K = _K()
    h, V = H.shape[1], G.num_nodes
    act_c, agg_c = K.act_code(_ACTS[act][0]()), K.act_code(_ACTS[agg][0]())
    assert K.fused_tile_rows(h, F32, act_c, reduce, agg_c) == 64
    _, perm, plan, maxdeg, zf = _layout(G)
    amax_out = torch.zeros(2, device=DEV)
    Hn, Sn = K.dmpnn_update_fused(
        H.to(DEV), S.to(DEV), G.edge_index[0].to(DEV), G.rev_index.to(DEV), K.pack_weights(W.to(DEV)), b.to(DEV),
        residual=True, act=act_c, plan=plan, tile_rows=64, max_in_degree=maxdeg, perm=perm, reduce=reduce,
        agg_act=agg_c, zero_fill=zf, amax_out=amax_out)
    assert _last_kernel().startswith(b"update_fk_kernel: one 8-wave workgroup per CU, 64-row tiles")
    rH, rS = _ref_layer(G, H, S, W, b, True, _ACTS[act][1], _ACTS[agg][1], reduce)
    what = f"fused fp32 h={h} {act}/{reduce}/{agg}"
    _check(Hn, rH, what + " H_out")
    _check(Sn, rS, what + " S_out")
    exact = dmpnn_ref.scatter(_ACTS[agg][1](Hn.cpu()), G.edge_index[1], V, reduce)
    assert torch.equal(Sn.cpu(), exact), what
    assert amax_out[0].item() == Hn.abs().max().item(), what
    assert amax_out[1].item() == Sn.abs().max().item(), what
    return zf, Sn


# 516: the lone sliver tile of chunk 1 goes through every epilogue variant (sum-only scan, the generic
# mean / max / min scan with its count carry, run-time act); 1028: three chunks per tile.
# Anything but (relu, sum, relu) above 512 runs here for the first time.
@pytest.mark.parametrize("h", [516, 1028])
@pytest.mark.parametrize("act,reduce,agg", [("relu", "sum", "relu"), ("relu", "sum", "identity"),
                                            ("relu", "mean", "relu"), ("relu", "max", "relu"),
                                            ("relu", "min", "identity"), ("silu", "sum", "relu")])
def test_update_fused_fk_wide(h, act, reduce, agg):
    _check_fused(*_fused_case(h), act, reduce, agg)


@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_update_fused_fk_wide_zero_in_degree_nodes(reduce):
    """A 3-atom chain, a lone atom (zero-bond molecule: no in-edge) and a diatomic: the lone atom's
    S_out row is exactly 0 in every chunk, the others follow the CPU scatter."""
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
    h = 516
    H, S = _rand(G.num_edges, h, seed=21), _rand(G.num_nodes, h, seed=22)
    W, b = _rand(h, h, seed=23) / h ** 0.5, _rand(h, seed=24)
    zf, Sn = _check_fused(G, H, S, W, b, "relu", reduce, "relu")
    assert zf and torch.count_nonzero(Sn[3]) == 0


# ------------------------------------------------------------------ 3. no stray writes
def _guarded(rows, h, pitch):
    """(buffer, view): rows x h inside a (64 + rows + 64) x pitch buffer filled with the sentinel."""
    buf = torch.full((rows + 128, pitch), SENTINEL, device=DEV)
    return buf, buf[64:64 + rows, :h]


def _assert_guards_intact(buf, rows, h, what):
    assert (buf[:64] == SENTINEL).all(), f"{what}: a guard row before the output was written"
    assert (buf[64 + rows:] == SENTINEL).all(), f"{what}: a guard row after the output was written"
    assert (buf[:, h:] == SENTINEL).all(), f"{what}: a pad column was written"
    assert not (buf[64:64 + rows, :h] == SENTINEL).any(), f"{what}: an output element was left unwritten"


def test_update_fk_wide_plain_writes_only_its_rows():
    """h = 516, E % 64 = 42: the partial last row tile and the 4-column sliver store nothing outside the
    E x h output (dense rows between 64 guard rows on either side)."""
    K = _K()
    h = 516
    G, H, S, W, b = _plain_case(h)
    E = G.num_edges
    buf, out = _guarded(E, h, h)
    got = K.dmpnn_update(H.to(DEV), S.to(DEV), G.edge_index[0].to(DEV), G.rev_index.to(DEV),
                         K.pack_weights(W.to(DEV)), b.to(DEV), residual=True, act=K.act_code(nn.ReLU()), out=out)
    assert got.data_ptr() == out.data_ptr()
    _assert_guards_intact(buf, E, h, "plain H_out")
    _check(out, _plain_product(h, "relu") + b.double() + H.double(), "guarded plain h=516")


def test_update_fused_fk_wide_writes_only_its_rows():
    """h = 516 on outputs of pitch 520: neither H_out's nor S_out's pad columns (the 4-column sliver's
    three masked pieces fall on them) nor the guard rows are written."""
    K = _K()
    h, pitch = 516, 520
    G, H, S, W, b = _fused_case(h)
    E, V = G.num_edges, G.num_nodes
    _, perm, plan, maxdeg, zf = _layout(G)
    bufH, out = _guarded(E, h, pitch)
    bufS, S_out = _guarded(V, h, pitch)
    relu = K.act_code(nn.ReLU())
    Hn, Sn = K.dmpnn_update_fused(
        H.to(DEV), S.to(DEV), G.edge_index[0].to(DEV), G.rev_index.to(DEV), K.pack_weights(W.to(DEV)), b.to(DEV),
        residual=True, act=relu, plan=plan, tile_rows=64, max_in_degree=maxdeg, perm=perm, reduce="sum",
        agg_act=relu, zero_fill=zf, out=out, S_out=S_out)
    assert Hn.data_ptr() == out.data_ptr() and Sn.data_ptr() == S_out.data_ptr()
    _assert_guards_intact(bufH, E, h, "fused H_out")
    _assert_guards_intact(bufS, V, h, "fused S_out")
    rH, rS = _ref_layer(G, H, S, W, b, True, torch.relu, torch.relu)
    _check(out, rH, "guarded fused h=516 H_out")
    _check(S_out, rS, "guarded fused h=516 S_out")


# ------------------------------------------------------------------ 4. row padding is invisible
def test_row_padded_init_and_layer_bit_identical_chunked():
    """h = 516 on pitch 520 (what the engine's inference forward runs), 64-row plan, two column chunks:
    init, a padded -> padded layer and a padded -> dense layer give the dense-row run's bits, amax
    chain included."""
    K = _K()
    h, pitch = 516, 520
    G = _graph("qm9", 200, seed=21)
    V, E = G.num_nodes, G.num_edges
    dst_ptr, perm, plan, deg, zf = _layout(G)
    torch.manual_seed(3)
    Xv, Xe = torch.randn(V, h, device=DEV), torch.randn(E, h, device=DEV)
    W, b = torch.randn(h, h, device=DEV) / h ** 0.5, torch.randn(h, device=DEV)
    Wp = K.pack_weights(W)
    src, rev = G.edge_index[0].contiguous().to(DEV), G.rev_index.to(DEV)
    relu, ident = K.act_code(nn.ReLU()), K.act_code(nn.Identity())
    rt = K.dmpnn_row_table(perm, plan[2], src, rev, V)
    outs = {}
    for ld in (h, pitch):
        am = torch.zeros(3, 2, device=DEV)
        H0, S0 = K.dmpnn_init(Xv, Xe, src, dst_ptr, perm, act=relu, amax=am[0], pitch=ld)
        assert H0.shape == (E, h) and H0.stride(0) == ld and S0.stride(0) == ld
        H1, S1 = K.dmpnn_update_fused(H0, S0, src, rev, Wp, b, act=relu, plan=plan, tile_rows=64,
                                      max_in_degree=deg, perm=perm, agg_act=relu, zero_fill=zf, amax_in=am[0],
                                      amax_out=am[1], row_table=rt, pitch_out=ld)
        assert H1.stride(0) == ld and S1.stride(0) == ld
        H2, S2 = K.dmpnn_update_fused(H1, S1, src, rev, Wp, b, act=relu, plan=plan, tile_rows=64,
                                      max_in_degree=deg, perm=perm, agg_act=ident, zero_fill=zf, amax_in=am[1],
                                      amax_out=am[2], row_table=rt)
        assert H2.is_contiguous() and S2.is_contiguous()
        outs[ld] = [t.contiguous() for t in (H0, S0, H1, S1, H2, S2)] + [am]
    for name, a, c in zip(("H0", "S0", "H1", "S1", "H2", "S2", "amax"), outs[h], outs[pitch]):
        assert torch.equal(a, c), name
    # and the values are the layer's (a wrong pitch on both runs alike would pass the comparison above)
    Hc, Sc = outs[h][0].cpu(), outs[h][1].cpu()
    rH, rS = _ref_layer(G, Hc, Sc, W.cpu(), b.cpu(), True, torch.relu, torch.relu)
    _check(outs[pitch][2], rH, "padded h=516 H1")
    _check(outs[pitch][3], rS, "padded h=516 S1")


@pytest.mark.parametrize("rev_offset", ["nodes", "edges"])
def test_block_h516(rev_offset):
    """ChempropBlock(516) + Sum in eval mode (intermediate layers on pitch 520) against the fp64 oracle."""
    from notorch_amd.nn import ChempropBlock, Sum
    from notorch_amd.nn.gnn import _engine

    h = 516
    assert _engine.row_pitch(h, F32) == 520
    G = _graph("qm9", 48, seed=h, rev_offset=rev_offset)
    torch.manual_seed(h)
    Xv, Xe = torch.randn(G.num_nodes, h), torch.randn(G.num_edges, h)
    blk = ChempropBlock(hidden_dim=h, depth=3).eval()
    Ws, bs = dmpnn_ref.block_params(blk)
    ref_n, ref_e = dmpnn_ref.chemprop_block(Xv.double(), Xe.double(), G.edge_index, G.rev_index,
                                            [w.detach().double() for w in Ws], [b.detach().double() for b in bs])
    ref_r = dmpnn_ref.readout(ref_n, G.batch_node_index, len(G), "sum")
    with torch.no_grad():
        out = blk.to(DEV)(G.update(node_feats=Xv, edge_feats=Xe).to(DEV))
        r = Sum()(out)
    assert _engine.LAST_UPDATE_INFO["kernel_short"] == "update_fk", _engine.LAST_UPDATE_INFO
    _check(out.edge_feats, ref_e, f"block h={h} {rev_offset} edge")
    _check(out.node_feats, ref_n, f"block h={h} {rev_offset} node")
    _check(r, ref_r, f"block h={h} {rev_offset} readout")


# ------------------------------------------------------------------ 5. persistent walk with chunks
def test_update_fused_fk_wide_persistent_walk():
    """h = 516, more than 5 x CUs + 3 tiles of 64 rows and ntiles % 8 != 0: ragged per-XCD chunks, five
    or six tiles x two column chunks per workgroup.  The (tile, chunk) unit walk, the gather three
    steps ahead from the last chunk of tile i into chunk 0 of tile i + 1, the 4-slot row-info ring
    (it wraps at the fifth tile) and the epilogue's prefetch of the next unit's residual and bias."""
    K = _K()
    h = 516
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_mol = _graph("qm9", 64, seed=11).num_edges / 64
    n0 = int((5 * cus + 4) * 64 / per_mol)
    for n in range(n0, 2 * n0, 7):
        G = _graph("qm9", n, seed=11)
        _, perm, plan, maxdeg, zf = _layout(G)
        if plan[1] % 8 != 0 and plan[1] > 5 * cus + 3:
            break
    else:
        pytest.fail("no batch size in range gives the wanted tile count")
    E, V = G.num_edges, G.num_nodes
    H, S = _rand(E, h, seed=n), _rand(V, h, seed=n + 1)
    W, b = _rand(h, h, seed=2) / h ** 0.5, _rand(h, seed=3)
    relu = K.act_code(nn.ReLU())
    assert K.fused_tile_rows(h, F32, relu, "sum", relu) == 64
    Hn, Sn = K.dmpnn_update_fused(H.to(DEV), S.to(DEV), G.edge_index[0].to(DEV), G.rev_index.to(DEV),
                                  K.pack_weights(W.to(DEV)), b.to(DEV), residual=True, act=relu, plan=plan,
                                  tile_rows=64, max_in_degree=maxdeg, perm=perm, agg_act=relu, zero_fill=zf)
    rH, rS = _ref_layer(G, H, S, W, b, True, torch.relu, torch.relu)
    _check(Hn, rH, f"walk h={h} ntiles={plan[1]} H_out")
    _check(Sn, rS, f"walk h={h} ntiles={plan[1]} S_out")
    assert torch.equal(Sn.cpu(), dmpnn_ref.scatter(torch.relu(Hn.cpu()), G.edge_index[1], V, "sum"))


def test_dense_matmul_fk_wide_persistent_walk():
    """Dense mode at h = 516 over 2 x CUs + 1 row tiles (two or three per workgroup, the last one of 37
    rows): fixed tiles in row order with two column chunks each."""
    K = _K()
    h = 516
    M = 64 * 2 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    X, W = _rand(M, h, seed=M), _rand(h, h, seed=h) / h ** 0.5
    out = K.dense_matmul(X.to(DEV), K.pack_weights(W.t().contiguous().to(DEV)))
    assert _last_kernel().startswith(b"update_fk_kernel")
    _check(out, X.double() @ W.double(), f"dense walk h={h} M={M}")


# ------------------------------------------------------------------ 6. dense mode, backward pieces
# (516, 1): one row; (516, 700): 11 tiles, the last of 60 rows; (1028, 130): three chunks, a 2-row tile
@pytest.mark.parametrize("h,M", [(516, 1), (516, 700), (1028, 130)])
def test_dense_matmul_fk_wide(h, M):
    K = _K()
    X, W = _rand(M, h, seed=M + h), _rand(h, h, seed=h) / h ** 0.5
    out = K.dense_matmul(X.to(DEV), K.pack_weights(W.t().contiguous().to(DEV)))
    _check(out, X.double() @ W.double(), f"dense fp32 h={h} M={M}")


# the generic fp32 weight-gradient kernel (no amax arguments) on 64 x 64 output tiles: 516 and 1028
# leave a 4-wide last tile in both dimensions; E = 33 and 4097 leave a 1-edge last k-step
@pytest.mark.parametrize("h,E,act", [(516, 33, "relu"), (1028, 4097, "gelu")])
def test_weight_grad_generic_wide(h, E, act):
    K = _K()
    mod, fn = _ACTS[act][0](), _ACTS[act][1]
    g = torch.Generator().manual_seed(E + h)
    V = max(E // 2, 1)
    Gr, H, S = torch.randn(E, h, generator=g), torch.randn(E, h, generator=g), torch.randn(V, h, generator=g)
    src, rev = torch.randint(0, V, (E,), generator=g), torch.randint(0, E, (E,), generator=g)
    args = (Gr.to(DEV), H.to(DEV), S.to(DEV), src.to(DEV), rev.to(DEV))
    dW, db = K.weight_grad(*args, act=K.act_code(mod))
    A = S.double()[src] - fn(H.double())[rev]
    _check(dW, Gr.double().t() @ A, f"dW h={h} E={E} {act}")
    _check(db, Gr.double().sum(0), f"db h={h} E={E}")
    dW2, db2 = K.weight_grad(*args, act=K.act_code(mod))
    assert torch.equal(dW, dW2) and torch.equal(db, db2)


# ------------------------------------------------------------------ 7. training at 516
def test_block_h516_gradients():
    """Training at h = 516 with SiLU: kernel forward and backward (fk dense dA, generic weight-gradient
    kernel) against fp64 oracle autograd."""
    from notorch_amd.nn import ChempropBlock

    h = 516
    G = _graph("qm9", 16, seed=9)
    torch.manual_seed(1)
    Xv, Xe = torch.randn(G.num_nodes, h), torch.randn(G.num_edges, h)
    blk = ChempropBlock(hidden_dim=h, act=nn.SiLU, depth=2).train()
    Ws, bs = dmpnn_ref.block_params(blk)
    Xv64, Xe64 = Xv.double().requires_grad_(), Xe.double().requires_grad_()
    W64 = [w.detach().double().requires_grad_() for w in Ws]
    b64 = [b.detach().double().requires_grad_() for b in bs]
    n64, e64 = dmpnn_ref.chemprop_block(Xv64, Xe64, G.edge_index, G.rev_index, W64, b64, act=nn.SiLU())
    (n64.sum() + (e64 ** 2).mean()).backward()
    blk = blk.to(DEV)
    Xv_d, Xe_d = Xv.to(DEV).requires_grad_(), Xe.to(DEV).requires_grad_()
    out = blk(G.update(node_feats=Xv_d, edge_feats=Xe_d).to(DEV))
    (out.node_feats.sum() + (out.edge_feats ** 2).mean()).backward()
    _check(out.edge_feats, e64, "train h=516 edge")
    _check(Xv_d.grad, Xv64.grad, "train h=516 dXv")
    _check(Xe_d.grad, Xe64.grad, "train h=516 dXe")
    for i, m in enumerate(blk._chemprop_layers()):
        _check(m.linear.weight.grad, W64[i].grad, f"train h=516 dW{i}")
        _check(m.linear.bias.grad, b64[i].grad, f"train h=516 db{i}")
