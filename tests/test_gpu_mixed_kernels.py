"""The mixed-precision boundary kernels (csrc/mixed.hip) bit for bit against what exists today:

* nt_dmpnn_pack_weights_mixed: the images of W and W^T and the bias copies equal
  pack_weights(W.to(bf16)), pack_weights(W.t().contiguous().to(bf16)) and b.to(bf16) byte for byte;
* nt_dmpnn_init_mixed: H0 = (Xv[src] + Xe).to(bf16) of the fp32 sum (one rounding), S the bits of
  segment_reduce over that H0;
* nt_dmpnn_init_embed_mixed: embed_bag (fp32) twice + nt_dmpnn_init_mixed.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

import topology

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
ACTS = {"ReLU": nn.ReLU(), "SiLU": nn.SiLU()}


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu()


# ------------------------------------------------------------------ pack
@pytest.mark.parametrize("nlayers", [1, 3, 16])
@pytest.mark.parametrize("h", [8, 36, 64, 528])  # partial k steps / column tiles; above 512 off a multiple of 32
def test_pack_bits(h, nlayers):
    from notorch_amd import kernels as K

    g = torch.Generator().manual_seed(100 * h + nlayers)
    Ws = [torch.randn(h, h, generator=g).to(DEV) for _ in range(nlayers)]
    bs = [torch.randn(h, generator=g).to(DEV) for _ in range(nlayers)]
    if nlayers == 3:  # one tensor given twice (a shared layer), one layer without a bias
        Ws[2], bs[2] = Ws[0], bs[0]
        bs[1] = None
    imgs, imgsT, b16 = K.pack_weights_mixed(Ws, bs, with_t=True)
    assert len(imgs) == len(imgsT) == len(b16) == nlayers
    for l, (W, b) in enumerate(zip(Ws, bs)):
        assert torch.equal(_bytes(imgs[l]), _bytes(K.pack_weights(W.to(BF16)))), f"image {l}"
        assert torch.equal(_bytes(imgsT[l]), _bytes(K.pack_weights(W.t().contiguous().to(BF16)))), f"image^T {l}"
        if b is None:
            assert b16[l] is None
        else:
            assert b16[l].dtype == BF16 and torch.equal(b16[l].cpu(), b.to(BF16).cpu()), f"bias {l}"
    # without the transposes and without biases: the same images
    only, none, nob = K.pack_weights_mixed(Ws)
    assert none is None and nob == [None] * nlayers
    for l in range(nlayers):
        assert torch.equal(_bytes(only[l]), _bytes(imgs[l]))
    # a bf16 source: the bytes of pack_weights
    W16 = [W.to(BF16) for W in Ws]
    i16, i16T, c16 = K.pack_weights_mixed(W16, [None if b is None else b.to(BF16) for b in bs], with_t=True)
    for l in range(nlayers):
        assert torch.equal(_bytes(i16[l]), _bytes(K.pack_weights(W16[l])))
        assert torch.equal(_bytes(i16T[l]), _bytes(K.pack_weights(W16[l].t().contiguous())))
        assert bs[l] is None or torch.equal(c16[l].cpu(), bs[l].to(BF16).cpu())


def test_pack_rejects_bad_arguments():
    from notorch_amd import kernels as K

    W = torch.zeros(16, 16, device=DEV)
    with pytest.raises(ValueError, match="at most 16"):
        K.pack_weights_mixed([W] * 17)
    with pytest.raises(ValueError, match="h <= 512"):
        K.pack_weights_mixed([torch.zeros(516, 516, device=DEV)])
    with pytest.raises(TypeError):
        K.pack_weights_mixed([W, W.to(BF16)])
    with pytest.raises(TypeError):
        K.pack_weights_mixed([W.double()])
    with pytest.raises(ValueError, match="contiguous"):
        K.pack_weights_mixed([torch.zeros(16, 32, device=DEV)[:, ::2]])


# ------------------------------------------------------------------ init
def _graphs():
    """(name, V, src, dst) of a small qm9 batch, a directed graph with in-degree-0 nodes, no edges."""
    from notorch_amd.data.synth import make_batch

    G = make_batch("qm9", 6, seed=4).collate("nodes")
    T = topology.block_graph("dir")
    assert (T.in_degree() == 0).any() and T.in_degree().max() > 8
    return [("qm9", G.num_nodes, G.edge_index[0], G.edge_index[1]),
            ("directed", T.V, T.edge_index[0], T.edge_index[1]),
            ("empty", 5, torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.int64))]


GRAPHS = None


def _cached_graphs():
    global GRAPHS
    if GRAPHS is None:
        GRAPHS = _graphs()
    return GRAPHS


@pytest.mark.parametrize("act", ["ReLU", "SiLU"])
@pytest.mark.parametrize("reduce", ["sum", "mean", "max", "min"])
@pytest.mark.parametrize("h", [64, 36, 8])  # 16-B pieces (two 16-B fp32 loads each), the scalar path, one piece
def test_init_bits(h, reduce, act):
    from notorch_amd import kernels as K

    code = K.act_code(ACTS[act])
    for name, V, src, dst in _cached_graphs():
        E = src.numel()
        g = torch.Generator().manual_seed(h + E)
        Xv, Xe = torch.randn(V, h, generator=g), torch.randn(E, h, generator=g)
        want = (Xv[src] + Xe).to(BF16)  # the fp32 sum, rounded once
        if E:  # the inputs are general: a cast followed by the bf16 add is a different number
            assert not torch.equal(want, (Xv.to(BF16)[src] + Xe.to(BF16)))
        if E:
            seg_ptr, perm = K.csr_build(dst.to(DEV), V)
        else:
            seg_ptr = torch.zeros(V + 1, dtype=torch.int32, device=DEV)
            perm = torch.empty(0, dtype=torch.int32, device=DEV)
        H0, S = K.dmpnn_init_mixed(Xv.to(DEV), Xe.to(DEV), src.to(DEV), seg_ptr, perm, act=code, reduce=reduce)
        assert H0.dtype == BF16 and S.dtype == BF16 and H0.shape == (E, h) and S.shape == (V, h)
        assert torch.equal(H0.cpu(), want), f"{name}: H0"
        S_ref = K.segment_reduce(want.to(DEV), seg_ptr, perm if E else None, V, reduce=reduce, act=code)
        assert torch.equal(S.cpu(), S_ref.cpu()), f"{name}: S"
        only, none = K.dmpnn_init_mixed(Xv.to(DEV), Xe.to(DEV), src.to(DEV))
        assert none is None and torch.equal(only.cpu(), want), f"{name}: init-only H0"


@pytest.mark.parametrize("kv,ke", [(7, 2), (3, 1)])
@pytest.mark.parametrize("h,reduce,act", [(64, "sum", "ReLU"), (36, "mean", "SiLU"), (8, "max", "ReLU"),
                                          (64, "min", "SiLU")])
def test_init_embed_bits(h, reduce, act, kv, ke):
    from notorch_amd import kernels as K

    code = K.act_code(ACTS[act])
    nv, ne = 42, 13
    for name, V, src, dst in _cached_graphs():
        E = src.numel()
        rng = np.random.default_rng(h + E + kv)
        vt = torch.from_numpy(rng.integers(0, nv, size=(V, kv))).to(DEV)
        et = torch.from_numpy(rng.integers(0, ne, size=(E, ke))).to(DEV)
        g = torch.Generator().manual_seed(h + kv)
        Tv, Te = torch.randn(nv, h, generator=g).to(DEV), torch.randn(ne, h, generator=g).to(DEV)
        if E:
            seg_ptr, perm = K.csr_build(dst.to(DEV), V)
        else:
            seg_ptr = torch.zeros(V + 1, dtype=torch.int32, device=DEV)
            perm = torch.empty(0, dtype=torch.int32, device=DEV)
        srcd = src.to(DEV)
        Xv, Xe = K.embed_bag(Tv, vt), K.embed_bag(Te, et)
        H_ref, S_ref = K.dmpnn_init_mixed(Xv, Xe, srcd, seg_ptr, perm, act=code, reduce=reduce)
        H0, S = K.dmpnn_init_embed_mixed(Tv, vt, Te, et, srcd, seg_ptr, perm, act=code, reduce=reduce)
        assert H0.dtype == BF16 and S.dtype == BF16
        assert torch.equal(H0.cpu(), H_ref.cpu()), f"{name}: H0"
        assert torch.equal(S.cpu(), S_ref.cpu()), f"{name}: S"
        only, none = K.dmpnn_init_embed_mixed(Tv, vt, Te, et, srcd)
        assert none is None and torch.equal(only.cpu(), H_ref.cpu()), f"{name}: init-only H0"
