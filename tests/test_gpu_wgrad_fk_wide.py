"""GPU parity of the fp32 fp16-split weight-gradient kernel above hidden 320 (csrc/wgrad.hip,
wgrad_fk_wide_kernel: dW tiled in 256 x 256 blocks, one workgroup per (edge chunk, i-block, j-block),
split-K over edge chunks with the fixed-order reduction, reached through nt_dmpnn_weight_grad_fk).

Criteria are those of tests/test_gpu_fused.py::test_weight_grad_fk:
* kernel: dW and db within FP32_NORM_TOL of the fp64 product, over magnitudes that need the power-of-two
  scales and with bounds above the true maxima; a second call bit-identical.  Every kernel test asserts
  through a spy on the loaded library that nt_dmpnn_weight_grad_fk itself ran (without the bounds, or
  before this kernel, K.weight_grad runs the bf16x6 kernel, which a parity check alone would pass);
* tails: columns past h and edges past E contribute exact zeros;
* block: every gradient within 1e-5 (FP32_NORM_TOL) of the fp64 oracle autograd.
"""
import pytest
import torch
import torch.nn as nn

from helpers import FP32_NORM_TOL, assert_parity, norm_err
from oracle import dmpnn_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
_MODS = {"relu": nn.ReLU, "identity": nn.Identity, "gelu": nn.GELU, "tanh": nn.Tanh, "silu": nn.SiLU}


def _K():
    from notorch_amd import kernels

    return kernels


def _graph(kind, n, seed=0):
    from notorch_amd.data.synth import make_batch

    return make_batch(kind, n, seed=seed).collate("nodes")


def _spy_entry(monkeypatch, name, log):
    """Count the calls of one C entry point of the loaded library."""
    lib = _K()._lib.load()
    real = getattr(lib, name)

    def wrapped(*a):
        log.append(name)
        return real(*a)

    monkeypatch.setattr(lib, name, wrapped)


def _operands(h, E, gs=1.0, xs=1.0):
    g = torch.Generator().manual_seed(E + h + 1)
    V = max(E // 2, 1)
    Gr = torch.randn(E, h, generator=g) * gs
    H, S = torch.randn(E, h, generator=g) * xs, torch.randn(V, h, generator=g) * xs
    src = torch.randint(0, V, (E,), generator=g)
    rev = torch.randint(0, E, (E,), generator=g)
    return Gr, H, S, src, rev


def _bounds(Gr, H, S):
    amax_G = torch.tensor([Gr.abs().max().item() * 1.7], device=DEV)
    amax_HS = torch.tensor([H.abs().max().item(), S.abs().max().item() * 1.3], device=DEV)
    return amax_G, amax_HS


# ------------------------------------------------------------------ the kernel against fp64
# 324: just over the old limit, one edge, a 4-column tail; 516: 4-wide tails in both dimensions, a 1-edge
# last step; 640: many chunks, the run-time activation instance; 904: a 136-column tail (partial i- and
# j-waves); 1024: exact blocks, the full split-K plan; 2048: more chunks planned than steps; 8192: the
# upper limit
@pytest.mark.parametrize("h,E,act,gs,xs", [(324, 1, "relu", 1.0, 1.0), (516, 33, "identity", 1e-6, 1e3),
                                            (640, 4097, "gelu", 1e4, 1e-3), (904, 77, "relu", 1.0, 1.0),
                                            (1024, 20_000, "silu", 1e-20, 1e10), (2048, 300, "tanh", 1.0, 1.0),
                                            (8192, 33, "relu", 1.0, 1.0)])
def test_weight_grad_fk_wide(h, E, act, gs, xs, monkeypatch):
    K = _K()
    mod = _MODS[act]()
    Gr, H, S, src, rev = _operands(h, E, gs, xs)
    amax_G, amax_HS = _bounds(Gr, H, S)
    args = (Gr.to(DEV), H.to(DEV), S.to(DEV), src.to(DEV), rev.to(DEV))
    calls = []
    _spy_entry(monkeypatch, "nt_dmpnn_weight_grad_fk", calls)
    _spy_entry(monkeypatch, "nt_dmpnn_weight_grad", calls)
    dW, db = K.weight_grad(*args, act=K.act_code(mod), amax_G=amax_G, amax_HS=amax_HS)
    assert calls == ["nt_dmpnn_weight_grad_fk"], calls
    A = S.double()[src] - mod(H.double())[rev]
    ref_dW, ref_db = Gr.double().t() @ A, Gr.double().sum(0)
    print(f"h={h} E={E} {act}: dW {norm_err(dW, ref_dW):.3e} db {norm_err(db, ref_db):.3e}")
    assert_parity(dW, ref_dW, FP32_NORM_TOL, f"dW h={h} E={E} {act}")
    assert_parity(db, ref_db, FP32_NORM_TOL, f"db h={h} E={E}")
    dW2, db2 = K.weight_grad(*args, act=K.act_code(mod), amax_G=amax_G, amax_HS=amax_HS)
    assert calls == ["nt_dmpnn_weight_grad_fk"] * 2, calls
    assert torch.equal(dW, dW2) and torch.equal(db, db2)


def test_weight_grad_fk_wide_no_edges(monkeypatch):
    K = _K()
    h = 640
    Z = torch.empty(0, h, device=DEV)
    e = torch.empty(0, dtype=torch.long, device=DEV)
    calls = []
    _spy_entry(monkeypatch, "nt_dmpnn_weight_grad_fk", calls)
    dW, db = K.weight_grad(Z, Z, torch.randn(3, h, device=DEV), e, e, amax_G=torch.ones(1, device=DEV),
                           amax_HS=torch.ones(2, device=DEV))
    assert calls == ["nt_dmpnn_weight_grad_fk"]
    assert dW.shape == (h, h) and db.shape == (h,)
    assert (dW == 0).all() and (db == 0).all()


# ------------------------------------------------------------------ tails are exact
def test_weight_grad_fk_wide_tails_exact(monkeypatch):
    """h = 516 = 2 x 256 + 4, E = 40 = 32 + 8: zero columns 512..515 of G (of H and S) give exactly zero
    rows (columns) of dW and entries of db, and leave every other element bit-identical (the bounds are
    those of the full operands in every call, so the scales are the same)."""
    K = _K()
    h, E, cut = 516, 40, 512
    ident = K.act_code(nn.Identity())
    Gr, H, S, src, rev = _operands(h, E)
    amax_G, amax_HS = _bounds(Gr, H, S)
    kw = dict(act=ident, amax_G=amax_G, amax_HS=amax_HS)
    idx = (src.to(DEV), rev.to(DEV))
    calls = []
    _spy_entry(monkeypatch, "nt_dmpnn_weight_grad_fk", calls)
    full_dW, full_db = K.weight_grad(Gr.to(DEV), H.to(DEV), S.to(DEV), *idx, **kw)

    Gz = Gr.clone()
    Gz[:, cut:] = 0
    dW, db = K.weight_grad(Gz.to(DEV), H.to(DEV), S.to(DEV), *idx, **kw)
    assert (dW[cut:] == 0.0).all() and (db[cut:] == 0.0).all()
    assert torch.equal(dW[:cut], full_dW[:cut]) and torch.equal(db[:cut], full_db[:cut])

    Hz, Sz = H.clone(), S.clone()
    Hz[:, cut:] = 0
    Sz[:, cut:] = 0
    dW, db = K.weight_grad(Gr.to(DEV), Hz.to(DEV), Sz.to(DEV), *idx, **kw)
    assert (dW[:, cut:] == 0.0).all()
    assert torch.equal(dW[:, :cut], full_dW[:, :cut]) and torch.equal(db, full_db)
    assert len(calls) == 3


# ------------------------------------------------------------------ every other call goes where it went
def test_fallbacks_unchanged(monkeypatch):
    """h = 322 (h % 4 != 0 above 320) and a misaligned view at h = 324 with bounds given run the bf16x6
    kernel and return the bits of the same call without bounds; h = 300 with bounds stays on
    wgrad_fk_kernel (whose device code this change leaves as it was) and repeats bit-identically."""
    K = _K()
    relu = K.act_code(nn.ReLU())
    calls = []
    _spy_entry(monkeypatch, "nt_dmpnn_weight_grad_fk", calls)
    _spy_entry(monkeypatch, "nt_dmpnn_weight_grad", calls)

    Gr, H, S, src, rev = _operands(322, 77)
    amax_G, amax_HS = _bounds(Gr, H, S)
    args = (Gr.to(DEV), H.to(DEV), S.to(DEV), src.to(DEV), rev.to(DEV))
    dW, db = K.weight_grad(*args, act=relu, amax_G=amax_G, amax_HS=amax_HS)
    dW0, db0 = K.weight_grad(*args, act=relu)
    assert calls == ["nt_dmpnn_weight_grad"] * 2, calls
    assert torch.equal(dW, dW0) and torch.equal(db, db0)

    del calls[:]
    Gr, H, S, src, rev = _operands(324, 77)
    amax_G, amax_HS = _bounds(Gr, H, S)
    flat = torch.zeros(77 * 324 + 1, device=DEV)
    Gv = flat[1:].view(77, 324)  # contiguous, 4 bytes off the 16-byte grid
    Gv.copy_(Gr)
    assert Gv.is_contiguous() and Gv.data_ptr() % 16 != 0
    args = (Gv, H.to(DEV), S.to(DEV), src.to(DEV), rev.to(DEV))
    dW, db = K.weight_grad(*args, act=relu, amax_G=amax_G, amax_HS=amax_HS)
    dW0, db0 = K.weight_grad(*args, act=relu)
    assert calls == ["nt_dmpnn_weight_grad"] * 2, calls
    assert torch.equal(dW, dW0) and torch.equal(db, db0)

    del calls[:]
    Gr, H, S, src, rev = _operands(300, 77)
    amax_G, amax_HS = _bounds(Gr, H, S)
    args = (Gr.to(DEV), H.to(DEV), S.to(DEV), src.to(DEV), rev.to(DEV))
    dW, db = K.weight_grad(*args, act=relu, amax_G=amax_G, amax_HS=amax_HS)
    dW2, db2 = K.weight_grad(*args, act=relu, amax_G=amax_G, amax_HS=amax_HS)
    assert calls == ["nt_dmpnn_weight_grad_fk"] * 2, calls
    assert torch.equal(dW, dW2) and torch.equal(db, db2)
    A = S.double()[src] - torch.relu(H.double())[rev]
    assert_parity(dW, Gr.double().t() @ A, FP32_NORM_TOL, "dW h=300")


# ------------------------------------------------------------------ block route and gradients
def _spy(monkeypatch, K, name, log):
    real = getattr(K, name)

    def wrapped(*a, **k):
        log.append((a, k))
        return real(*a, **k)

    monkeypatch.setattr(K, name, wrapped)


def _block_grads(h, depth, kind, n, dropout=0.0, seed=None):
    """fp64 truth and a device() closure of one fp32 block + Sum readout (the recipe of
    tests/test_gpu_bf16_wgrad_wide.py; with dropout the truth gets the block's own masks, recovered by
    running nt_dropout_residual on ones)."""
    from notorch_amd.nn import ChempropBlock, Sum
    from notorch_amd.nn.gnn import _engine

    K = _K()
    G = _graph(kind, n, seed=3)
    E = G.num_edges
    torch.manual_seed(0)
    Xv, Xe = torch.randn(G.num_nodes, h), torch.randn(E, h)
    torch.manual_seed(1)
    opts = dict(dropout=dropout) if dropout else {}
    blk = ChempropBlock(h, depth=depth, act=nn.SiLU, **opts).to(DEV).train()

    kw = {}
    if dropout:
        torch.manual_seed(seed)
        drawn = _engine.draw_dropout_seed()
        ones = torch.ones(E, h, device=DEV)
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

    def device():
        for p in blk.parameters():
            p.grad = None
        if dropout:
            torch.manual_seed(seed)  # the block draws the same seed
        Xv_d, Xe_d = Xv.to(DEV).requires_grad_(True), Xe.to(DEV).requires_grad_(True)
        out = blk(G.update(node_feats=Xv_d, edge_feats=Xe_d).to(DEV))
        (Sum()(out).pow(2).sum() + (out.edge_feats * torch.linspace(-1, 1, h, device=DEV)).sum()).backward()
        layers = blk._chemprop_layers()
        return ([Xv_d.grad, Xe_d.grad] + [l.linear.weight.grad for l in layers]
                + [l.linear.bias.grad for l in layers])

    return G, truth, device


def _check_grads(got, truth, depth, what):
    names = ["dXv", "dXe"] + [f"dW[{l}]" for l in range(depth)] + [f"db[{l}]" for l in range(depth)]
    for name, a, t in zip(names, got, truth):
        print(f"{what} {name}: normalised max error {norm_err(a, t):.3e}")
        assert_parity(a, t, 1e-5, f"{what} {name}")


@pytest.mark.parametrize("h", [384, 512])
def test_block_grads_fk_wide_wgrad_route(h, monkeypatch):
    """The backward of an fp32 block above hidden 320 hands the bounds it has (max|G|, the forward's amax
    row) to K.weight_grad, which runs nt_dmpnn_weight_grad_fk; no message tensor.  NT_WGRAD=kernel6 keeps
    the bf16x6 kernel (no bounds).  Both within 1e-5 of the fp64 oracle autograd."""
    K = _K()
    depth = 2
    monkeypatch.delenv("NT_WGRAD", raising=False)
    monkeypatch.setenv("NT_BWD", "kernel")
    G, truth, device = _block_grads(h, depth, "zinc", 16)
    wg, msg, entry = [], [], []
    _spy(monkeypatch, K, "weight_grad", wg)
    _spy(monkeypatch, K, "dmpnn_message", msg)
    _spy_entry(monkeypatch, "nt_dmpnn_weight_grad_fk", entry)

    got = device()
    assert len(wg) == depth and not msg, (len(wg), len(msg))
    assert all(k.get("amax_G") is not None and k.get("amax_HS") is not None for _, k in wg)
    assert all(a[0].dtype == torch.float32 and a[0].shape == (G.num_edges, h) for a, _ in wg)
    assert len(entry) == depth
    _check_grads(got, truth, depth, f"h={h} kernel")

    del wg[:], msg[:], entry[:]
    monkeypatch.setenv("NT_WGRAD", "kernel6")
    got = device()
    assert len(wg) == depth and not msg and not entry, (len(wg), len(msg), len(entry))
    assert all(k.get("amax_G") is None and k.get("amax_HS") is None for _, k in wg)
    _check_grads(got, truth, depth, f"h={h} kernel6")


# ------------------------------------------------------------------ dropout
def test_block_dropout_h384_wgrad(monkeypatch):
    """h = 384, p = 0.25 in training mode: the backward hands the dropout-scaled gradient
    (nt_dropout_residual's output) and a max|G| bound taken afresh from it to K.weight_grad; gradients
    against the fp64 oracle fed the block's own masks."""
    K = _K()
    h, depth, p = 384, 2, 0.25
    monkeypatch.delenv("NT_WGRAD", raising=False)
    monkeypatch.setenv("NT_BWD", "kernel")
    G, truth, device = _block_grads(h, depth, "qm9", 24, dropout=p, seed=99)
    wg, scaled, entry = [], [], []
    _spy(monkeypatch, K, "weight_grad", wg)
    _spy_entry(monkeypatch, "nt_dmpnn_weight_grad_fk", entry)
    real = K.dropout_residual

    def dropout_residual(*a, **k):
        out = real(*a, **k)
        scaled.append(out)  # kept alive: a later tensor cannot reuse its storage
        return out

    monkeypatch.setattr(K, "dropout_residual", dropout_residual)
    got = device()
    assert len(wg) == depth and len(entry) == depth
    ptrs = {t.data_ptr() for t in scaled}
    assert all(a[0].data_ptr() in ptrs and a[0].shape == (G.num_edges, h) for a, _ in wg)
    for a, k in wg:  # the bound is the scaled gradient's own maximum
        assert k["amax_G"].item() == a[0].abs().max().item()
    _check_grads(got, truth, depth, "dropout h=384")
