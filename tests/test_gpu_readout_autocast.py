"""Gated / SDPAttention under torch.autocast(dtype=bfloat16): bf16 node_feats (what a block returns there)
with fp32 keys (Gated.a.weight / a.bias, SDPAttention's Q) on nt_node_scores_mixed / nt_softmax_pool +
nt_softmax_pool_backward_mixed, which round each key element to bf16 where they load it.

The yardstick is code that exists without the feature: the same module moved .to(bfloat16) (or
Q.to(bfloat16)), run outside autocast on the bf16-storage kernels.  Outputs and dX must equal it bit
for bit; the fp32 keys' gradients stay fp32 and equal the yardstick's after rounding.  Accuracy is the
project's bf16 criterion (normalised max error <= 2e-2, tests/test_gpu_readout.py::test_readouts_bf16)
against the fp32 oracle on the rounded inputs.

Hidden sizes: 8 (16-byte pieces), 36 and 300 (h % 8 == 4: by element), 520 (the wave's column loop runs
twice).  Batches: 16 QM9-like molecules; the same with the nodes shuffled (batch_node_index not sorted:
mol_perm is used); the same plus a molecule of one node.
"""
import copy
import functools

import pytest
import torch

from helpers import assert_parity
from oracle import dmpnn_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
BF16_TOL = 2e-2  # tests/test_gpu_readout.py::test_readouts_bf16
KINDS = ("qm9", "unsorted", "single")
HS = (8, 36, 300, 520)


def _autocast(**kw):
    return torch.autocast(device_type="cuda", dtype=BF16, **kw)


@functools.lru_cache(maxsize=None)
def _graph(kind):
    """A CPU BatchedGraph; only its node side (batch_node_index, len) matters to a readout."""
    from notorch_amd.data.models.graph import BatchedGraph
    from notorch_amd.data.synth import make_batch

    G = make_batch("qm9", 16, seed=11).collate("nodes")
    bni, B, V = G.batch_node_index, len(G), G.num_nodes
    if kind == "qm9":
        return G
    if kind == "unsorted":  # new node i is old node pi[i]
        pi = torch.randperm(V, generator=torch.Generator().manual_seed(5))
        inv = torch.empty_like(pi)
        inv[pi] = torch.arange(V)
        G2 = BatchedGraph(G.node_feats[pi].contiguous(), G.edge_feats, inv[G.edge_index], G.rev_index,
                          batch_node_index=bni[pi].contiguous(), batch_edge_index=G.batch_edge_index, size=B)
        assert not bool((G2.batch_node_index[1:] >= G2.batch_node_index[:-1]).all())
        return G2
    assert kind == "single"  # one more molecule: a single atom, no bond
    G2 = BatchedGraph(torch.cat([G.node_feats, G.node_feats[:1]]), G.edge_feats, G.edge_index, G.rev_index,
                      batch_node_index=torch.cat([bni, torch.tensor([B])]), batch_edge_index=G.batch_edge_index,
                      size=B + 1)
    assert int((G2.batch_node_index == B).sum()) == 1
    return G2


@functools.lru_cache(maxsize=None)
def _inputs(kind, h):
    """(X bf16, fp32 Gated on the CPU, fp32 Q, fp32 loss weights), none of the keys bf16-representable."""
    from notorch_amd.nn import Gated

    G = _graph(kind)
    torch.manual_seed(100 + h)
    X = torch.randn(G.num_nodes, h).to(BF16)
    ro = Gated(h)
    Q = torch.randn(len(G), h)
    for k in (ro.a.weight, ro.a.bias, Q):  # rounding changes them: one rounding is told from none
        assert not torch.equal(k.detach(), k.detach().to(BF16).float())
    return X, ro, Q, torch.linspace(-1, 1, h)


def _on_device(kind, X, grad=False):
    Xd = X.to(DEV).requires_grad_(grad)
    return _graph(kind).update(node_feats=Xd).to(DEV), Xd  # update() copies: the cached CPU graph stays


def _loss(out, w):
    o = out.float()
    return o.pow(2).sum() + (o * w.to(o.device)).sum()


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("kind", KINDS)
def test_forward_equals_bf16_storage(kind, h, monkeypatch):
    from notorch_amd import kernels as K
    from notorch_amd.nn import SDPAttention
    from notorch_amd.nn.gnn import _engine

    X, ro, Q, _ = _inputs(kind, h)
    G = _graph(kind)
    B, bni = len(G), G.batch_node_index
    yard = copy.deepcopy(ro).to(DEV, BF16)
    ro = copy.deepcopy(ro).to(DEV)
    Gd, _ = _on_device(kind, X)
    if kind == "unsorted":
        assert _engine.mol_layout(Gd)[1] is not None
    calls = []
    real = getattr(K, "node_scores_mixed", None)  # without the feature the readout below raises TypeError
    monkeypatch.setattr(K, "node_scores_mixed", lambda *a, **k: calls.append(1) or real(*a, **k), raising=False)
    sdpa = SDPAttention(h)
    with torch.no_grad():
        with _autocast():
            got = ro(Gd)
            got_q = sdpa(Gd, Q=Q.to(DEV))
        assert calls == [1, 1]
        want = yard(Gd)
        want_q = sdpa(Gd, Q=Q.to(DEV, BF16))
    assert calls == [1, 1]  # the yardstick ran the plain kernels
    assert all(p.dtype == torch.float32 for p in ro.parameters())
    assert got.dtype == BF16 and got_q.dtype == BF16 and got.shape == (B, h)
    assert torch.equal(got, want), "Gated"
    assert torch.equal(got_q, want_q), "SDPAttention"
    Xf = X.float()
    ref = dmpnn_ref.readout_gated(Xf, bni, B, ro.a.weight.detach().cpu().to(BF16).float(),
                                  ro.a.bias.detach().cpu().to(BF16).float())
    assert_parity(got.float(), ref, BF16_TOL, "Gated against the fp32 oracle")
    ref_q = dmpnn_ref.readout_sdpa(Xf, bni, B, Q.to(BF16).float(), h ** 0.5)
    assert_parity(got_q.float(), ref_q, BF16_TOL, "SDPAttention against the fp32 oracle")


# ------------------------------------------------------------------ backward
def _twice(loss, leaves):
    """Gradients of two backward passes over the same graph."""
    runs = []
    for _ in range(2):
        for t in leaves:
            t.grad = None
        loss.backward(retain_graph=True)
        runs.append([t.grad.clone() for t in leaves])
    return runs


@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("kind", KINDS)
def test_backward_equals_bf16_storage(kind, h, monkeypatch):
    from notorch_amd import kernels as K
    from notorch_amd.nn import SDPAttention

    X, ro, Q, w = _inputs(kind, h)
    calls = []
    real = K.softmax_pool_backward_mixed
    monkeypatch.setattr(K, "softmax_pool_backward_mixed", lambda *a, **k: calls.append(1) or real(*a, **k))
    # Gated
    yard = copy.deepcopy(ro).to(DEV, BF16)
    ro = copy.deepcopy(ro).to(DEV)
    Gd, Xd = _on_device(kind, X, grad=True)
    with _autocast():
        out = ro(Gd)
    got, again = _twice(_loss(out, w), [Xd, ro.a.weight, ro.a.bias])
    assert calls == [1, 1]
    Gy, Xy = _on_device(kind, X, grad=True)
    _loss(yard(Gy), w).backward()
    assert calls == [1, 1]
    ref = [Xy.grad, yard.a.weight.grad, yard.a.bias.grad]
    assert got[0].dtype == BF16 and torch.equal(got[0], ref[0]), "Gated dX"
    for nm, g, r in zip(("da", "db"), got[1:], ref[1:]):
        assert g.dtype == torch.float32 and torch.isfinite(g).all(), nm
        assert r.dtype == BF16 and torch.equal(g.to(BF16), r), f"Gated {nm}: differs after rounding"
    assert bool((got[1] != got[1].bfloat16().float()).any()), "da is a widened bf16 value: the fp32 sum was not kept"
    for nm, g, a in zip(("dX", "da", "db"), got, again):
        assert torch.equal(g, a), f"Gated {nm}: not deterministic"
    # SDPAttention, X and Q both trained
    del calls[:]
    sdpa = SDPAttention(h)
    Gd, Xd = _on_device(kind, X, grad=True)
    Qd = Q.to(DEV).requires_grad_(True)
    with _autocast():
        out = sdpa(Gd, Q=Qd)
    got, again = _twice(_loss(out, w), [Xd, Qd])
    assert calls == [1, 1]
    Gy, Xy = _on_device(kind, X, grad=True)
    Qy = Q.to(DEV, BF16).requires_grad_(True)
    _loss(sdpa(Gy, Q=Qy), w).backward()
    assert got[0].dtype == BF16 and torch.equal(got[0], Xy.grad), "SDPA dX"
    assert got[1].dtype == torch.float32 and torch.isfinite(got[1]).all()
    assert Qy.grad.dtype == BF16 and torch.equal(got[1].to(BF16), Qy.grad), "SDPA dQ: differs after rounding"
    assert bool((got[1] != got[1].bfloat16().float()).any()), "dQ is a widened bf16 value"
    for nm, g, a in zip(("dX", "dQ"), got, again):
        assert torch.equal(g, a), f"SDPA {nm}: not deterministic"


def test_frozen_features_still_train_the_keys():
    """X without grad (a frozen encoder): the fp32 keys still get their fp32 gradients on the mixed route."""
    from notorch_amd.nn import SDPAttention

    X, ro, Q, w = _inputs("qm9", 36)
    ro = copy.deepcopy(ro).to(DEV)
    Gd, _ = _on_device("qm9", X)
    Qd = Q.to(DEV).requires_grad_(True)
    with _autocast():
        loss = _loss(ro(Gd), w) + _loss(SDPAttention(36)(Gd, Q=Qd), w)
    loss.backward()
    for g in (ro.a.weight.grad, ro.a.bias.grad, Qd.grad):
        assert g is not None and g.dtype == torch.float32 and torch.isfinite(g).all()


# ------------------------------------------------------------------ unchanged behaviour
def test_the_mixed_pair_is_still_rejected_outside_bf16_autocast():
    from notorch_amd.nn import SDPAttention

    h = 36
    X, ro, Q, _ = _inputs("qm9", h)
    ro = copy.deepcopy(ro).to(DEV)
    Gd, _ = _on_device("qm9", X)
    Qd = Q.to(DEV)
    sdpa = SDPAttention(h)
    msg = "float32 but the other operands are torch.bfloat16"
    with torch.no_grad():
        for run in (lambda: ro(Gd), lambda: sdpa(Gd, Q=Qd)):
            with pytest.raises(TypeError, match=msg):
                run()
            with torch.autocast(device_type="cuda", dtype=torch.float16), pytest.raises(TypeError, match=msg):
                run()
            with _autocast(), torch.autocast(device_type="cuda", enabled=False), pytest.raises(TypeError, match=msg):
                run()
            with _autocast(enabled=False), pytest.raises(TypeError, match=msg):
                run()
        # fp32 features with bf16 keys: not this feature, inside autocast or not
        Gf, _ = _on_device("qm9", X.float())
        ro16 = copy.deepcopy(ro).to(BF16)
        for run in (lambda: ro16(Gf), lambda: sdpa(Gf, Q=Qd.to(BF16))):
            with pytest.raises(TypeError, match="bfloat16 but the other operands are torch.float32"):
                run()
            with _autocast(), pytest.raises(TypeError, match="bfloat16 but the other operands are torch.float32"):
                run()


@pytest.mark.parametrize("h", [8, 300])
def test_operands_of_one_dtype_run_as_outside_autocast(h, monkeypatch):
    from notorch_amd import kernels as K
    from notorch_amd.nn import SDPAttention

    def _no_mixed(*a, **k):
        raise AssertionError("operands of one dtype must stay on the plain kernels")

    monkeypatch.setattr(K, "node_scores_mixed", _no_mixed)
    monkeypatch.setattr(K, "softmax_pool_backward_mixed", _no_mixed)
    X, ro, Q, w = _inputs("qm9", h)
    sdpa = SDPAttention(h)
    for dt in (torch.float32, BF16):
        mod = copy.deepcopy(ro).to(DEV, dt)
        res = []
        for auto in (False, True):
            Gd, Xd = _on_device("qm9", X.to(dt), grad=True)
            Qd = Q.to(DEV, dt).requires_grad_(True)
            mod.zero_grad(set_to_none=True)
            with _autocast(enabled=auto):
                o, oq = mod(Gd), sdpa(Gd, Q=Qd)
            (_loss(o, w) + _loss(oq, w)).backward()
            res.append([o, oq, Xd.grad, Qd.grad, mod.a.weight.grad.clone(), mod.a.bias.grad.clone()])
        for nm, a, b in zip(("Gated", "SDPA", "dX", "dQ", "da", "db"), *res):
            assert a.dtype == dt and b.dtype == dt, nm
            assert torch.equal(a, b), f"{dt} {nm}: autocast changed the result"


# ------------------------------------------------------------------ the whole model
def test_model_trains_under_autocast(monkeypatch):
    """EmbeddedChempropBlock -> Gated -> MLP, every parameter fp32, one training step inside bf16 autocast
    (what Lightning's precision="bf16-mixed" runs): the readout takes the mixed route, every parameter
    gets an fp32, finite gradient, and the loss is within 2e-2 (relative) of the fp32 oracle on the
    bf16-rounded tables and weights."""
    from notorch_amd import kernels as K
    from notorch_amd.nn import MLP, ChempropBlock, EmbeddedChempropBlock, Gated, GraphEmbedding

    h = 64
    Gc = _graph("qm9")
    B = len(Gc)
    torch.manual_seed(21)
    enc = EmbeddedChempropBlock(GraphEmbedding(hidden_dim=h), ChempropBlock(h, depth=2))
    ro, head = Gated(h), MLP(h, 1)
    y = torch.randn(B, 1)
    # the fp32 oracle on the rounded parameters (CPU)
    r = lambda t: t.detach().to(BF16).float()  # noqa: E731
    Xv = r(enc.embedding.node.weight)[Gc.node_feats].sum(1)
    Xe = r(enc.embedding.edge.weight)[Gc.edge_feats].sum(1)
    Ws, bs = dmpnn_ref.block_params(enc.block)
    node, _ = dmpnn_ref.chemprop_block(Xv, Xe, Gc.edge_index, Gc.rev_index, [r(W) for W in Ws],
                                       [None if b is None else r(b) for b in bs])
    pooled = dmpnn_ref.readout_gated(node, Gc.batch_node_index, B, r(ro.a.weight), r(ro.a.bias))
    head_r = copy.deepcopy(head)
    with torch.no_grad():
        for p in head_r.parameters():
            p.copy_(r(p))
        want = (head_r(pooled) - y).pow(2).mean().item()

    calls = {"fwd": 0, "bwd": 0}
    real_f, real_b = K.node_scores_mixed, K.softmax_pool_backward_mixed

    def spy_f(*a, **k):
        calls["fwd"] += 1
        return real_f(*a, **k)

    def spy_b(*a, **k):
        calls["bwd"] += 1
        return real_b(*a, **k)

    monkeypatch.setattr(K, "node_scores_mixed", spy_f)
    monkeypatch.setattr(K, "softmax_pool_backward_mixed", spy_b)
    enc, ro, head = enc.to(DEV).train(), ro.to(DEV).train(), head.to(DEV).train()
    params = [p for m in (enc, ro, head) for p in m.parameters()]
    opt = torch.optim.SGD(params, lr=1e-3)
    Gd = Gc.update().to(DEV)
    with _autocast():
        out = enc(Gd)
        assert out.node_feats.dtype == BF16
        pooled_d = ro(out)
        assert pooled_d.dtype == BF16
        loss = (head(pooled_d).float() - y.to(DEV)).pow(2).mean()
    loss.backward()
    opt.step()
    assert calls == {"fwd": 1, "bwd": 1}
    for p in params:
        assert p.dtype == torch.float32
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all()
    got = loss.item()
    rel = abs(got - want) / abs(want)
    print(f"model loss under autocast {got:.6f} | fp32 oracle on rounded parameters {want:.6f} | relative {rel:.3e}")
    assert rel <= 2e-2, f"loss {got} vs oracle {want}: relative {rel:.3e}"
