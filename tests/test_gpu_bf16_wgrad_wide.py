"""GPU parity of the bf16 weight-gradient kernel above hidden 512 (csrc/wgrad.hip,
wgrad_bf16_wide_kernel: dW tiled in 256 x 256 blocks, one workgroup per (edge chunk, i-block, j-block),
split-K over edge chunks with the fixed-order reduction).

Criteria are those of tests/test_gpu_bf16_backward.py:
* kernel: dW and db in fp32 within FP32_NORM_TOL of the fp64 product of the same bf16 operands (A read
  back from nt_dmpnn_message: the kernel forms it bit-identically), a second call bit-identical;
* tails: columns past h and edges past E contribute exact zeros;
* block: every gradient no further from the fp64 oracle than BF16_FACTOR x the torch-op recompute
  (NT_BWD=torch), or than the floor BF16_FLOOR, on the normalised max and the relative L2 error.
"""
import pytest
import torch
import torch.nn as nn

from helpers import FP32_NORM_TOL, assert_parity, norm_err
from oracle import dmpnn_ref
from test_gpu_bf16_wide import BF16_FACTOR, BF16_FLOOR, _graph, _rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
_MODS = {"relu": nn.ReLU, "identity": nn.Identity, "gelu": nn.GELU, "tanh": nn.Tanh}


def _K():
    from notorch_amd import kernels

    return kernels


def _operands(h, E, seed=None):
    g = torch.Generator().manual_seed(E + h if seed is None else seed)
    V = max(E // 2, 1)
    Gr = torch.randn(E, h, generator=g).to(BF)
    H, S = torch.randn(E, h, generator=g).to(BF), torch.randn(V, h, generator=g).to(BF)
    src = torch.randint(0, V, (E,), generator=g)
    rev = torch.randint(0, E, (E,), generator=g)
    return Gr, H, S, src, rev


# ------------------------------------------------------------------ the kernel against fp64
# 520: just over the old limit, 8-column tails, a single edge; 640: one full step plus one edge;
# 1032: tails in both dimensions, many chunks, the generic-activation instance; 1024: exact blocks, the
# full split-K plan; 2048: many tiles, more chunks planned than steps; 8192: the upper limit;
# 904: a 136-column tail (the last block's second i-wave and third j-wave hold partial tiles)
@pytest.mark.parametrize("h,E,act", [(520, 1, "relu"), (640, 33, "identity"), (1032, 4097, "gelu"),
                                     (1024, 20_000, "relu"), (2048, 300, "tanh"), (8192, 33, "relu"),
                                     (904, 77, "relu")])
def test_weight_grad_bf16_wide(h, E, act):
    K = _K()
    mod = _MODS[act]()
    Gr, H, S, src, rev = _operands(h, E)
    args = (Gr.to(DEV), H.to(DEV), S.to(DEV), src.to(DEV), rev.to(DEV))
    dW, db = K.weight_grad(*args, act=K.act_code(mod))
    A = K.dmpnn_message(args[1], args[2], args[3], args[4], act=K.act_code(mod)).cpu()  # bf16 message
    assert dW.dtype == torch.float32 and db.dtype == torch.float32
    assert_parity(dW, Gr.double().t() @ A.double(), FP32_NORM_TOL, f"dW h={h} E={E} {act}")
    assert_parity(db, Gr.double().sum(0), FP32_NORM_TOL, f"db h={h} E={E}")
    dW2, db2 = K.weight_grad(*args, act=K.act_code(mod))
    assert torch.equal(dW, dW2) and torch.equal(db, db2)


def test_weight_grad_bf16_wide_no_edges():
    K = _K()
    h = 640
    Z = torch.empty(0, h, device=DEV, dtype=BF)
    e = torch.empty(0, dtype=torch.long, device=DEV)
    dW, db = K.weight_grad(Z, Z, torch.randn(3, h, device=DEV).to(BF), e, e)
    assert dW.shape == (h, h) and db.shape == (h,)
    assert (dW == 0).all() and (db == 0).all()


def test_weight_grad_bf16_wide_rejects_other_sizes():
    K = _K()
    e = torch.zeros(4, dtype=torch.long, device=DEV)
    for h in (644, 8200):
        X = torch.zeros(4, h, device=DEV, dtype=BF)
        with pytest.raises(ValueError, match="h % 8 == 0"):
            K.weight_grad(X, X, X, e, e)


# ------------------------------------------------------------------ tails are exact
def test_weight_grad_bf16_wide_tails_exact():
    """h = 520 = 2 x 256 + 8, E = 40 = 32 + 8: zero columns 512..519 of G (of A) give exactly zero rows
    (columns) of dW and entries of db, and leave every other element bit-identical."""
    K = _K()
    h, E, cut = 520, 40, 512
    ident = K.act_code(nn.Identity())
    Gr, H, S, src, rev = _operands(h, E)
    idx = (src.to(DEV), rev.to(DEV))
    full_dW, full_db = K.weight_grad(Gr.to(DEV), H.to(DEV), S.to(DEV), *idx, act=ident)

    Gz = Gr.clone()
    Gz[:, cut:] = 0
    dW, db = K.weight_grad(Gz.to(DEV), H.to(DEV), S.to(DEV), *idx, act=ident)
    assert (dW[cut:] == 0.0).all() and (db[cut:] == 0.0).all()
    assert torch.equal(dW[:cut], full_dW[:cut]) and torch.equal(db[:cut], full_db[:cut])

    Hz, Sz = H.clone(), S.clone()
    Hz[:, cut:] = 0
    Sz[:, cut:] = 0
    dW, db = K.weight_grad(Gr.to(DEV), Hz.to(DEV), Sz.to(DEV), *idx, act=ident)
    assert (dW[:, cut:] == 0.0).all()
    assert torch.equal(dW[:, :cut], full_dW[:, :cut]) and torch.equal(db, full_db)


# ------------------------------------------------------------------ block route and gradients
def _spy(monkeypatch, K, name, log):
    real = getattr(K, name)

    def wrapped(*a, **k):
        log.append(a)
        return real(*a, **k)

    monkeypatch.setattr(K, name, wrapped)


def _block_grads(monkeypatch, h, depth, kind, n, dropout=0.0, seed=None):
    """fp64 truth and a device(mode) closure of one block + Sum readout (the recipe of
    tests/test_gpu_bf16_wide.py::test_block_grads_bf16_wide; with dropout the truth gets the block's
    own masks, recovered by running nt_dropout_residual on ones)."""
    from notorch_amd.nn import ChempropBlock, Sum
    from notorch_amd.nn.gnn import _engine

    K = _K()
    G = _graph(kind, n, seed=3)
    E = G.num_edges
    torch.manual_seed(0)
    Xv = nn.EmbeddingBag(42, h, mode="sum")(G.node_feats).detach().to(BF)
    Xe = nn.EmbeddingBag(13, h, mode="sum")(G.edge_feats).detach().to(BF)
    torch.manual_seed(1)
    opts = dict(dropout=dropout) if dropout else {}
    blk = ChempropBlock(h, depth=depth, act=nn.SiLU, **opts).to(DEV, BF).train()

    kw = {}
    if dropout:
        torch.manual_seed(seed)
        drawn = _engine.draw_dropout_seed()
        ones = torch.ones(E, h, device=DEV, dtype=BF)
        kw["dropout_masks"] = [
            (K.dropout_residual(ones, dropout, drawn, _engine.dropout_offset(l, E, h)) != 0).double().cpu()
            / (1 - dropout) for l in range(depth)]
    Ws, bs = dmpnn_ref.block_params(blk)
    Ws = [W.detach().double().cpu().requires_grad_(True) for W in Ws]
    bs = [b.detach().double().cpu().requires_grad_(True) for b in bs]
    Xv_r, Xe_r = Xv.double().requires_grad_(True), Xe.double().requires_grad_(True)
    nd, e = dmpnn_ref.chemprop_block(Xv_r, Xe_r, G.edge_index, G.rev_index, Ws, bs,
                                     act=torch.nn.functional.silu, residual=True, reduce="sum", **kw)
    r = dmpnn_ref.readout(nd, G.batch_node_index, len(G), "sum")
    (r.pow(2).sum() + (e * torch.linspace(-1, 1, h, dtype=torch.float64)).sum()).backward()
    truth = [Xv_r.grad, Xe_r.grad] + [W.grad for W in Ws] + [b.grad for b in bs]

    def device(mode):
        monkeypatch.setenv("NT_BWD", mode)
        for p in blk.parameters():
            p.grad = None
        if dropout:
            torch.manual_seed(seed)  # the block draws the same seed
        Xv_d, Xe_d = Xv.to(DEV).requires_grad_(True), Xe.to(DEV).requires_grad_(True)
        out = blk(G.update(node_feats=Xv_d, edge_feats=Xe_d).to(DEV))
        ef = out.edge_feats.float()
        (Sum()(out).float().pow(2).sum() + (ef * torch.linspace(-1, 1, h, device=DEV)).sum()).backward()
        layers = blk._chemprop_layers()
        return ([Xv_d.grad, Xe_d.grad] + [l.linear.weight.grad for l in layers]
                + [l.linear.bias.grad for l in layers])

    return G, truth, device


def _check_grads(got, ref, truth, depth):
    names = ["dXv", "dXe"] + [f"dW[{l}]" for l in range(depth)] + [f"db[{l}]" for l in range(depth)]
    for name, a, rf, t in zip(names, got, ref, truth):
        assert a.dtype == BF and torch.isfinite(a.float()).all(), name
        e_max, r_max = norm_err(a.float(), t), norm_err(rf.float(), t)
        e_l2, r_l2 = _rel_l2(a, t), _rel_l2(rf, t)
        print(f"{name}: kernel max {e_max:.2e} l2 {e_l2:.2e} | torch bf16 max {r_max:.2e} l2 {r_l2:.2e}")
        assert e_max <= max(BF16_FLOOR, BF16_FACTOR * r_max), f"{name}: max {e_max:.3e} vs torch bf16 {r_max:.3e}"
        assert e_l2 <= max(BF16_FLOOR, BF16_FACTOR * r_l2), f"{name}: L2 {e_l2:.3e} vs torch bf16 {r_l2:.3e}"


@pytest.mark.parametrize("h", [640, 1024])
def test_block_grads_bf16_wide_wgrad_route(h, monkeypatch):
    """The backward of a wide bf16 block forms dW and db on K.weight_grad (no message tensor, no
    library GEMM); NT_WGRAD=library keeps the message + library GEMM route.  Both meet the criteria."""
    K = _K()
    depth = 2
    G, truth, device = _block_grads(monkeypatch, h, depth, "zinc", 16)
    ref = device("torch")
    wg, msg = [], []
    _spy(monkeypatch, K, "weight_grad", wg)
    _spy(monkeypatch, K, "dmpnn_message", msg)

    got = device("kernel")
    assert len(wg) == depth and not msg, (len(wg), len(msg))
    assert all(a[0].dtype == BF and a[0].shape == (G.num_edges, h) for a in wg)
    _check_grads(got, ref, truth, depth)

    del wg[:], msg[:]
    monkeypatch.setenv("NT_WGRAD", "library")
    got = device("kernel")
    assert not wg and len(msg) == depth, (len(wg), len(msg))
    _check_grads(got, ref, truth, depth)


# ------------------------------------------------------------------ dropout
def test_block_dropout_bf16_h640_wgrad(monkeypatch):
    """h = 640, p = 0.25 in training mode: the forward meets the criteria of
    tests/test_gpu_wide_hidden_entry.py::test_block_dropout_forward_bf16_h640, and the backward hands
    the dropout-scaled gradient (nt_dropout_residual's output) to K.weight_grad."""
    from test_gpu_bf16_wide import _block_vs_torch_bf16

    K = _K()
    h, depth, p = 640, 2, 0.25
    info = _block_vs_torch_bf16("qm9", 24, h, depth, seed=4, dropout_seed=99, dropout=p)
    assert info["kernel_short"] == "update_bf16" and "wide" in info["kernel"], info

    G, truth, device = _block_grads(monkeypatch, h, depth, "qm9", 24, dropout=p, seed=99)
    ref = device("torch")
    wg, scaled = [], []
    _spy(monkeypatch, K, "weight_grad", wg)
    real = K.dropout_residual

    def dropout_residual(*a, **k):
        out = real(*a, **k)
        scaled.append(out)  # kept alive: a later tensor cannot reuse its storage
        return out

    monkeypatch.setattr(K, "dropout_residual", dropout_residual)
    got = device("kernel")
    assert len(wg) == depth
    ptrs = {t.data_ptr() for t in scaled}
    assert all(a[0].data_ptr() in ptrs and a[0].shape == (G.num_edges, h) for a in wg)
    _check_grads(got, ref, truth, depth)
