"""The attention readouts (Gated / SDPAttention: nt_node_scores, nt_softmax_pool, nt_softmax_pool_backward
and the key-rounding copies of mixed.hip) at their seams, against fp64.

References.  The fp64 oracle (oracle/dmpnn_ref.py readout_gated / readout_sdpa / scatter_softmax) and, for
the binding-level backward, the closed form in fp64 on the same inputs (``_closed_form``):
alpha = softmax_g(s), ds = alpha (<dout_g, X_v> - <dout_g, out_g>), dX = alpha dout_g + ds key,
P_g = sum ds X.  ``test_closed_form_is_the_oracle_gradient`` (CPU) first holds the closed form to fp64
autograd through the oracle.  fp32 results are held to the project contract (assert_parity, 1e-5
normalised max error).

A. ``test_pool_supplied_scores*``: the pool alone, the scores passed in (fp32) so that the reference starts
   from the same scores: empty molecules in the middle / first and last, a 3000-node serial walk, scores
   in +-1 and +-200 (an unshifted exp overflows), tied maxima, a masked (-inf) node.  Each layout runs
   sorted (perm = None) and with the nodes shuffled (csr_build's perm).  The shuffle keeps the order of
   the nodes inside every molecule (csr_build is stable, the kernels walk ascending CSR positions), so
   every sum runs over the same values in the same order and the two runs are asserted bit-equal after
   un-permuting, besides both being within tolerance of the reference.
B. ``test_column_seams*``: hidden sizes around the lanes' column trips (fp32 256 columns per trip in 16-byte
   pieces and 64 by element, bf16 512) and buffers that are contiguous but not 16-byte aligned (the
   by-element fallback).  The two paths map lanes to columns differently (a lane of the 16-byte path sums N
   neighbouring columns per trip, a lane of the fallback strides by 64), so every wave-reduced dot product
   (the scores, c_g, hence ds, dX and P) is summed in another order: those are held to the reference
   tolerance only.  The pool forward sums each output column over the nodes in ascending order on both
   paths, so with the same scores its misaligned output is asserted bit-equal to the aligned one.
   bf16 storage here: the fp32 outputs (scores, ds, P) are fp32 arithmetic on exactly representable
   products and stay on the 1e-5 contract (the backward takes c_g from the pooled row before its rounding
   to bf16, not from the stored ``out``); the bf16 outputs (out, dX) are one rounding of an fp32 value,
   2^-9 relative, held to 2^-8 normalised.
C. ``test_grid_stride*``: the smallest shapes whose grid-stride loops take a second (and third) trip.
D. ``test_modules*``: Gated / SDPAttention under autograd on unsorted indices, empty molecules, long
   molecules; a query with more rows than the batch has molecules (dQ rows past the batch are zero), fp32
   and on the mixed (bf16 autocast) route.
E. ``test_bf16_storage_against_fp64``: bf16 storage against fp64 on the bf16-rounded inputs, no further than
   BF16_FACTOR x the oracle evaluated with torch ops in bf16 on the same device (tests/test_gpu_bf16.py) on
   the normalised max and the relative L2 error, and under the 2e-2 ceiling of the bf16 readout tests.
   Measured on an MI355X, device | torch bf16, each normalised max error / relative L2 (torch's scatter
   uses atomics: its figures move by a few percent between runs):

       h = 36   Gated out  2.46e-3 / 1.66e-3 | 1.01e-2 / 5.81e-3     SDPA out  1.97e-3 / 1.59e-3 | 8.75e-3 / 6.11e-3
                Gated dX   3.81e-3 / 2.40e-3 | 1.85e-2 / 1.32e-2     SDPA dX   3.16e-3 / 2.15e-3 | 1.53e-2 / 1.36e-2
                Gated da   1.53e-3 / 1.23e-3 | 8.91e-3 / 6.51e-3     SDPA dQ   2.09e-3 / 1.83e-3 | 1.45e-2 / 1.44e-2
                Gated db   6.8e-8 | 1.8e-4   (|error| / max|da|)
       h = 520  Gated out  2.39e-3 / 1.66e-3 | 1.29e-2 / 5.90e-3     SDPA out  3.47e-3 / 1.65e-3 | 1.10e-2 / 6.13e-3
                Gated dX   2.46e-3 / 1.92e-3 | 1.25e-2 / 2.04e-2     SDPA dX   2.13e-3 / 1.74e-3 | 1.70e-2 / 1.73e-2
                Gated da   1.85e-3 / 1.61e-3 | 1.77e-2 / 1.83e-2     SDPA dQ   3.33e-3 / 1.70e-3 | 2.53e-2 / 1.79e-2
                Gated db   4.2e-8 | 2.4e-5   (|error| / max|da|)

   db before the statistics kernel took c_g from the unrounded pooled row (it read the stored bf16 ``out``,
   which left sum_v ds_v = <dout_g, pooled_g - out_g> in every molecule): 2.5e-5 at h = 36 and 2.5e-4 at
   h = 520, the latter 5.6 x torch's 4.5e-5 of that run.
"""
import functools

import pytest
import torch

from helpers import assert_parity, norm_err
from oracle import dmpnn_ref

gpu = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
BF16_FACTOR = 2.0  # tests/test_gpu_bf16.py
BF16_CEIL = 2e-2  # tests/test_gpu_readout.py::test_readouts_bf16
BF16_ROUND = 2.0 ** -8  # one rounding to bf16 (2^-9 relative) of an fp32 value, with room for the fp32 error


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _seg_of(lens):
    lens = torch.as_tensor(lens, dtype=torch.int64)
    return torch.repeat_interleave(torch.arange(lens.numel()), lens)


def _seg_ptr(seg, B):
    ptr = torch.zeros(B + 1, dtype=torch.int64)
    ptr[1:] = torch.bincount(seg, minlength=B).cumsum(0)
    return ptr.to(torch.int32)


def _closed_form(X, s, seg, B, dout, key_rows):
    """fp64: (out, dX, ds, P) of the softmax pool of X (n x h) under the scores s (n) of molecules seg (n)
    for dout (B x h); key_rows (n x h or broadcastable) is ds_v's factor in dX_v: a for Gated,
    Q[seg] / sqrt_key for SDPAttention."""
    X, s, dout = X.double(), s.double(), dout.double()
    alpha = dmpnn_ref.scatter_softmax(s, seg, B)
    out = dmpnn_ref.scatter(alpha.unsqueeze(1) * X, seg, B, "sum")
    ds = alpha * ((dout[seg] * X).sum(1) - (dout * out).sum(1)[seg])
    dX = alpha.unsqueeze(1) * dout[seg] + ds.unsqueeze(1) * key_rows.double()
    P = dmpnn_ref.scatter(ds.unsqueeze(1) * X, seg, B, "sum")
    return out, dX, ds, P


def _key_rows(key, seg, sdpa, sqrt_key):
    return key.double()[seg] / sqrt_key if sdpa else key.double().reshape(1, -1)


def _ref_scores(X, key, bias, seg, sdpa, sqrt_key):
    if sdpa:
        return (key.double()[seg] * X.double()).sum(1) / sqrt_key
    s = X.double() @ key.double().reshape(-1)
    return s if bias is None else s + bias.double()


# ---------------------------------------------------------------------------------------------- CPU
def test_closed_form_is_the_oracle_gradient():
    """The closed form against fp64 autograd through the oracle: a finite case with unsorted indices, an
    empty molecule, a single-node molecule and a spread of scores."""
    g = torch.Generator().manual_seed(0)
    lens, h = [4, 0, 1, 7, 3], 6
    B = len(lens)
    seg = _seg_of(lens)[torch.randperm(sum(lens), generator=g)]
    X = 3 * torch.randn(sum(lens), h, generator=g, dtype=torch.float64)
    dout = torch.randn(B, h, generator=g, dtype=torch.float64)
    # Gated
    a = torch.randn(1, h, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(1, generator=g, dtype=torch.float64).requires_grad_(True)
    Xr = X.clone().requires_grad_(True)
    out = dmpnn_ref.readout_gated(Xr, seg, B, a, b)
    (out * dout).sum().backward()
    s = _ref_scores(X, a.detach(), b.detach(), seg, False, 1.0)
    o, dX, ds, P = _closed_form(X, s, seg, B, dout, _key_rows(a.detach(), seg, False, 1.0))
    assert s.max() - s.min() > 5
    for what, got, ref in (("out", o, out), ("dX", dX, Xr.grad), ("da", P.sum(0).reshape(1, h), a.grad)):
        assert_parity(got, ref.detach(), 1e-10, f"Gated {what}")
    assert abs(ds.sum().item() - b.grad.item()) <= 1e-10 * a.grad.abs().max().item()
    # the score gradient itself, through scatter_softmax
    sr = s.clone().requires_grad_(True)
    alpha = dmpnn_ref.scatter_softmax(sr, seg, B).unsqueeze(1)
    (dmpnn_ref.scatter(alpha * X, seg, B, "sum") * dout).sum().backward()
    assert_parity(ds, sr.grad, 1e-10, "ds")
    # SDPAttention, a query with more rows than molecules
    sk = h ** 0.5
    Q = torch.randn(B + 2, h, generator=g, dtype=torch.float64).requires_grad_(True)
    Xr = X.clone().requires_grad_(True)
    out = dmpnn_ref.readout_sdpa(Xr, seg, B, Q, sk)
    (out * dout).sum().backward()
    s = _ref_scores(X, Q.detach(), None, seg, True, sk)
    o, dX, ds, P = _closed_form(X, s, seg, B, dout, _key_rows(Q.detach(), seg, True, sk))
    for what, got, ref in (("out", o, out), ("dX", dX, Xr.grad), ("dQ", P / sk, Q.grad[:B])):
        assert_parity(got, ref.detach(), 1e-10, f"SDPA {what}")
    assert not Q.grad[B:].any()
    assert not o[1].any() and not P[1].any()  # the empty molecule


# ---------------------------------------------------------------------------------------------- A
LENS_MID = (1, 0, 3, 64, 65, 3000, 0, 2)  # empties in the middle, a long serial walk
LENS_ENDS = (0, 1, 3, 64, 65, 3000, 2, 0)  # empties first and last


@functools.lru_cache(maxsize=None)
def _pool_case(lens, h, span, sdpa, special=None):
    """CPU inputs (fp32) and the fp64 closed form of one supplied-scores case; computed once."""
    B, n = len(lens), sum(lens)
    g = torch.Generator().manual_seed(1000 * h + int(span) + 7 * sdpa + len(special or ""))
    seg = _seg_of(lens)
    X = torch.randn(n, h, generator=g)
    s = (torch.rand(n, generator=g) * 2 - 1) * span
    dout = torch.randn(B, h, generator=g)
    key = torch.randn(B, h, generator=g) if sdpa else torch.randn(h, generator=g) / h ** 0.5
    sqrt_key = h ** 0.5 if sdpa else 1.0
    ptr = _seg_ptr(seg, B)
    marked = None
    if special == "ties":  # three tied maxima in the 65-node molecule, two in the 3-node one
        g65, g3 = lens.index(65), lens.index(3)
        s[ptr[g65] + torch.tensor([0, 31, 64])] = s[seg == g65].max() + 0.5
        s[ptr[g3] + torch.tensor([0, 2])] = s[seg == g3].max()
    elif special == "masked":  # one node of the 64-node molecule is masked out
        marked = int(ptr[lens.index(64)]) + 17
        s[marked] = float("-inf")
    ref = _closed_form(X, s, seg, B, dout, _key_rows(key, seg, sdpa, sqrt_key))
    return dict(B=B, n=n, seg=seg, ptr=ptr, X=X, s=s, dout=dout, key=key, sqrt_key=sqrt_key, ref=ref,
                marked=marked)


def _shuffle(seg, seed):
    """(seg of the shuffled nodes, src): the j-th node of the sorted layout sits at position src[j] of the
    shuffled one.  The molecules are interleaved at random and the nodes of one molecule keep their
    order, so the stable CSR of the shuffled indices lists them as the sorted layout does."""
    new_seg = seg[torch.randperm(seg.numel(), generator=torch.Generator().manual_seed(seed))]
    return new_seg, torch.argsort(new_seg, stable=True)


def _pool_on_device(c, sdpa, shuffled):
    """(out, dX, ds, P) of K.softmax_pool / K.softmax_pool_backward, node rows in the sorted layout's order."""
    from notorch_amd import kernels as K

    B, X, s, seg = c["B"], c["X"], c["s"], c["seg"]
    src = None
    if shuffled:
        seg, src = _shuffle(c["seg"], seed=c["n"])
        assert not bool((seg[1:] >= seg[:-1]).all())
        X, s = torch.empty_like(X), torch.empty_like(s)
        X[src], s[src] = c["X"], c["s"]
        segd = seg.to(DEV)
        ptr, perm = K.csr_build(segd, B)
        assert torch.equal(ptr.cpu(), c["ptr"]) and torch.equal(perm.cpu().long(), src)
    else:
        segd, ptr, perm = seg.to(DEV), c["ptr"].to(DEV), None
    Xd, sd, dout, key = X.to(DEV), s.to(DEV), c["dout"].to(DEV), c["key"].to(DEV)
    out = K.softmax_pool(Xd, sd, ptr, perm, B)
    dX, ds, P = K.softmax_pool_backward(Xd, sd, ptr, perm, segd, B, out, dout,
                                        a=None if sdpa else key, Q=key if sdpa else None, sqrt_key=c["sqrt_key"])
    out, dX, ds, P = out.cpu(), dX.cpu(), ds.cpu(), P.cpu()
    if shuffled:
        dX, ds = dX[src], ds[src]
    return out, dX, ds, P


def _check_pool_case(c, sdpa):
    B, seg, X = c["B"], c["seg"], c["X"]
    lens = torch.bincount(seg, minlength=B)
    runs = {}
    for shuffled in (False, True):
        got = runs[shuffled] = _pool_on_device(c, sdpa, shuffled)
        tag = "shuffled" if shuffled else "sorted"
        for what, a, r in zip(("out", "dX", "ds", "P"), got, c["ref"]):
            assert torch.isfinite(a).all(), f"{tag} {what}: not finite"
            assert_parity(a, r, 1e-5, f"{tag} {what}")
        out, dX, ds, P = got
        for g in (lens == 0).nonzero().flatten().tolist():  # empty molecule: zeros, not NaN
            assert not out[g].any() and not P[g].any(), f"{tag}: empty molecule {g}"
        for g in (lens == 1).nonzero().flatten().tolist():  # single node: alpha is exactly 1
            v = int(c["ptr"][g])
            assert torch.equal(out[g], X[v]), f"{tag}: single-node molecule {g}"
            assert ds[v].item() == 0.0, f"{tag}: single-node ds"
    for what, a, b in zip(("out", "dX", "ds", "P"), runs[False], runs[True]):
        assert torch.equal(a, b), f"{what}: sorted and shuffled runs differ in bits"
    return runs[False]


@gpu
@pytest.mark.parametrize("sdpa", [False, True], ids=["gated", "sdpa"])
@pytest.mark.parametrize("span", [1.0, 200.0])
@pytest.mark.parametrize("h", [8, 300])
@pytest.mark.parametrize("lens", [LENS_MID, LENS_ENDS], ids=["empties-mid", "empties-ends"])
def test_pool_supplied_scores(lens, h, span, sdpa):
    _check_pool_case(_pool_case(lens, h, span, sdpa), sdpa)


@gpu
@pytest.mark.parametrize("h", [8, 300])
def test_pool_supplied_scores_tied_maxima(h):
    c = _pool_case(LENS_MID, h, 200.0, False, "ties")
    _check_pool_case(c, False)
    g65 = LENS_MID.index(65)
    tied = c["ptr"][g65] + torch.tensor([0, 31, 64])
    in_g = c["s"][c["seg"] == g65]
    assert (c["s"][tied] == in_g.max()).all() and int((in_g == in_g.max()).sum()) == 3  # the case is what it says


@gpu
@pytest.mark.parametrize("h", [8, 300])
@pytest.mark.parametrize("span", [1.0, 200.0])
def test_pool_supplied_scores_masked_node(h, span):
    """A node with score -inf: everything finite, its alpha, ds and dX row exactly 0."""
    from notorch_amd import kernels as K

    c = _pool_case(LENS_MID, h, span, True, "masked")
    out, dX, ds, P = _check_pool_case(c, True)
    v = c["marked"]
    assert ds[v].item() == 0.0 and not dX[v].any()
    # alpha itself: pool the indicator of the masked node (column 0) beside a column of ones (sum of alpha)
    g = int(c["seg"][v])
    probe = torch.zeros(c["n"], 4)
    probe[v, 0] = 1.0
    probe[c["seg"] == g, 1] = 1.0
    a = K.softmax_pool(probe.to(DEV), c["s"].to(DEV), c["ptr"].to(DEV), None, c["B"]).cpu()
    assert a[g, 0].item() == 0.0 and abs(a[g, 1].item() - 1.0) <= 1e-5


# ---------------------------------------------------------------------------------------------- B
@functools.lru_cache(maxsize=None)
def _qm9_seg(n_mols, seed):
    from notorch_amd.data.synth import make_batch

    G = make_batch("qm9", n_mols, seed=seed).collate("nodes")
    seg = G.batch_node_index.clone()
    assert bool((seg[1:] >= seg[:-1]).all())
    return seg, len(G)


def _offset_view(t):
    """t's values in a contiguous view one element into a flat device buffer: not 16-byte aligned."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _seam_inputs(seg, B, h, dtype, sdpa, seed):
    g = torch.Generator().manual_seed(seed)
    n = seg.numel()
    X = torch.randn(n, h, generator=g).to(dtype)
    dout = torch.randn(B, h, generator=g).to(dtype)
    if sdpa:
        key, bias, sqrt_key = torch.randn(B, h, generator=g).to(dtype), None, h ** 0.5
    else:
        key, bias, sqrt_key = (torch.randn(h, generator=g) / h ** 0.5).to(dtype), torch.randn(1, generator=g).to(dtype), 1.0
    return X, dout, key, bias, sqrt_key


def _scores_pool_backward(X, dout, key, bias, sqrt_key, seg, ptr, B, sdpa, scores=None):
    """Device (s, out, dX, ds, P) through the three bindings; the pool runs on ``scores`` if given."""
    from notorch_amd import kernels as K

    if sdpa:
        s = K.node_scores(X, Q=key, node_seg=seg, sqrt_key=sqrt_key)
    else:
        s = K.node_scores(X, a=key, a_bias=bias)
    sp = s if scores is None else scores
    out = K.softmax_pool(X, sp, ptr, None, B)
    dX, ds, P = K.softmax_pool_backward(X, sp, ptr, None, seg, B, out, dout, a=None if sdpa else key,
                                        Q=key if sdpa else None, sqrt_key=sqrt_key)
    return s, out, dX, ds, P


def _check_seams(cpu, got, seg, B, sdpa, what, scores=None):
    """Device results against fp64 on the same inputs; the pool's reference starts from the scores the pool
    was given.  fp32: 1e-5 everywhere.  bf16: see the module docstring (B)."""
    X, dout, key, bias, sqrt_key = cpu
    s, out, dX, ds, P = got
    bf = X.dtype == BF16
    assert s.dtype == torch.float32 and ds.dtype == torch.float32 and P.dtype == torch.float32
    assert out.dtype == X.dtype and dX.dtype == X.dtype
    assert_parity(s, _ref_scores(X, key, bias, seg, sdpa, sqrt_key), 1e-5, f"{what} scores")
    sp = (s if scores is None else scores).cpu()
    r_out, r_dX, r_ds, r_P = _closed_form(X, sp, seg, B, dout, _key_rows(key, seg, sdpa, sqrt_key))
    assert_parity(out, r_out, BF16_ROUND if bf else 1e-5, f"{what} out")
    assert_parity(dX, r_dX, BF16_ROUND if bf else 1e-5, f"{what} dX")
    assert_parity(ds, r_ds, 1e-5, f"{what} ds")
    assert_parity(P, r_P, 1e-5, f"{what} P")


SEAM_HS = [(torch.float32, h) for h in (1, 4, 63, 65, 129, 252, 256, 260, 516)] + \
          [(BF16, h) for h in (8, 36, 132, 504, 512, 520, 1032)]


@gpu
@pytest.mark.parametrize("sdpa", [False, True], ids=["gated", "sdpa"])
@pytest.mark.parametrize("dtype,h", SEAM_HS, ids=[f"{'bf16' if d == BF16 else 'fp32'}-{h}" for d, h in SEAM_HS])
def test_column_seams(dtype, h, sdpa):
    seg, B = _qm9_seg(16, 21)
    cpu = _seam_inputs(seg, B, h, dtype, sdpa, seed=h + sdpa)
    segd, ptr = seg.to(DEV), _seg_ptr(seg, B).to(DEV)
    X, dout, key, bias, sqrt_key = (t.to(DEV) if torch.is_tensor(t) else t for t in cpu)
    got = _scores_pool_backward(X, dout, key, bias, sqrt_key, segd, ptr, B, sdpa)
    _check_seams(cpu, got, seg, B, sdpa, f"h={h}")


@gpu
@pytest.mark.parametrize("sdpa", [False, True], ids=["gated", "sdpa"])
@pytest.mark.parametrize("dtype,h", [(torch.float32, 300), (BF16, 520)], ids=["fp32-300", "bf16-520"])
def test_column_seams_misaligned(dtype, h, sdpa):
    """X, the key and dout one element off 16-byte alignment: the by-element fallback at a hidden size that
    otherwise runs in 16-byte pieces.  Bit-equal to the aligned run where the order of every sum is the
    same (the pool forward on the same scores); reference tolerance for the rest (module docstring, B)."""
    seg, B = _qm9_seg(16, 21)
    cpu = _seam_inputs(seg, B, h, dtype, sdpa, seed=h + sdpa)
    segd, ptr = seg.to(DEV), _seg_ptr(seg, B).to(DEV)
    X, dout, key, bias, sqrt_key = (t.to(DEV) if torch.is_tensor(t) else t for t in cpu)
    assert all(t.data_ptr() % 16 == 0 for t in (X, dout, key))
    al = _scores_pool_backward(X, dout, key, bias, sqrt_key, segd, ptr, B, sdpa)
    _check_seams(cpu, al, seg, B, sdpa, f"aligned h={h}")
    Xm, dm, km = _offset_view(X), _offset_view(dout), _offset_view(key)
    mis = _scores_pool_backward(Xm, dm, km, bias, sqrt_key, segd, ptr, B, sdpa, scores=al[0])
    _check_seams(cpu, mis, seg, B, sdpa, f"misaligned h={h}", scores=al[0])
    assert torch.equal(mis[1], al[1]), "pool forward: misaligned and aligned runs differ in bits"


# ---------------------------------------------------------------------------------------------- C
def _grid_case(lens, h, seed):
    """Scores on the device (both keys), then the pool forward and backward on those scores, fp32."""
    B, n = len(lens), int(sum(lens))
    seg = _seg_of(lens)
    segd, ptr = seg.to(DEV), _seg_ptr(seg, B).to(DEV)
    for sdpa in (False, True):
        cpu = _seam_inputs(seg, B, h, torch.float32, sdpa, seed=seed + sdpa)
        X, dout, key, bias, sqrt_key = (t.to(DEV) if torch.is_tensor(t) else t for t in cpu)
        got = _scores_pool_backward(X, dout, key, bias, sqrt_key, segd, ptr, B, sdpa)
        _check_seams(cpu, got, seg, B, sdpa, f"n={n} B={B} h={h} {'sdpa' if sdpa else 'gated'}")


@gpu
def test_grid_stride_nodes_and_stats():
    """65,537 nodes in 32,769 molecules of 1-3 nodes, h = 8: the per-node score and backward kernels (one
    wave per node, 32,768 waves) reach their third trip, the per-molecule statistics kernel its second."""
    lens = [1, 2, 3] * 10923
    lens[2] = 2
    assert len(lens) == 32769 and sum(lens) == 65537
    _grid_case(lens, 8, seed=31)


@gpu
@pytest.mark.parametrize("B,h", [(8193, 1024), (8225, 255)], ids=["pieces-1024", "by-element-255"])
def test_grid_stride_pool_lanes(B, h):
    """The pool and weighted-pool kernels (one lane per molecule and column piece, 8192 x 256 lanes) take
    a second trip: 8,193 x 1024 / 4 and 8,225 x 255 lanes."""
    lens = ([1, 2] * (B // 2 + 1))[:B]
    assert B * (h // 4 if h % 4 == 0 else h) > 8192 * 256
    _grid_case(lens, h, seed=37)


# ---------------------------------------------------------------------------------------------- D
@functools.lru_cache(maxsize=None)
def _module_graph(kind):
    from notorch_amd.data.models.graph import BatchedGraph
    from notorch_amd.data.synth import make_batch

    if kind == "polymer":
        return make_batch("polymer", 2, seed=7).collate("nodes")
    G = make_batch("qm9", 8, seed=2).collate("nodes")
    if kind == "unsorted":  # tests/test_gpu_parity.py::test_readout_unsorted_batch_index
        p = torch.randperm(G.num_nodes, generator=torch.Generator().manual_seed(3))
        bni, size = G.batch_node_index[p].contiguous(), 8
        assert not bool((bni[1:] >= bni[:-1]).all())
    else:  # molecule 3 and the last molecule are empty
        assert kind == "empties"
        bni, size = G.batch_node_index + (G.batch_node_index >= 3).long(), 10
        assert torch.bincount(bni, minlength=size)[[3, 9]].tolist() == [0, 0]
    return BatchedGraph(G.node_feats, G.edge_feats, G.edge_index, G.rev_index, batch_node_index=bni,
                        batch_edge_index=G.batch_edge_index, size=size)


def _loss(out, w):
    o = out.float() if out.dtype == BF16 else out
    return o.pow(2).sum() + (o * w.to(device=o.device, dtype=o.dtype)).sum()


def _fp64_module_refs(G, X, gated, Q, w):
    """fp64 oracle autograd: (Gated out, dX, da, db), (SDPA out, dX, dQ) on the given (CPU) values."""
    bni, B, h = G.batch_node_index, len(G), X.shape[1]
    w = w.double()
    a, b = gated.a.weight.detach().double().requires_grad_(True), gated.a.bias.detach().double().requires_grad_(True)
    Xr = X.double().requires_grad_(True)
    out = dmpnn_ref.readout_gated(Xr, bni, B, a, b)
    _loss(out, w).backward()
    ref_g = (out.detach(), Xr.grad, a.grad, b.grad)
    Xr, Qr = X.double().requires_grad_(True), Q.double().requires_grad_(True)
    out = dmpnn_ref.readout_sdpa(Xr, bni, B, Qr, h ** 0.5)
    _loss(out, w).backward()
    return ref_g, (out.detach(), Xr.grad, Qr.grad)


@gpu
@pytest.mark.parametrize("h", [36, 13])
@pytest.mark.parametrize("kind", ["unsorted", "empties", "polymer"])
def test_modules_against_fp64_autograd(kind, h):
    from notorch_amd.nn import Gated, SDPAttention
    from notorch_amd.nn.gnn import _engine

    G = _module_graph(kind)
    B = len(G)
    torch.manual_seed(40 + h)
    X = torch.randn(G.num_nodes, h)
    Q = torch.randn(B, h)
    w = torch.linspace(-1, 1, h)
    ro = Gated(h)
    ref_g, ref_q = _fp64_module_refs(G, X, ro, Q, w)
    ro = ro.to(DEV)
    Xd = X.to(DEV).requires_grad_(True)
    Gd = G.update(node_feats=Xd).to(DEV)
    assert len(Gd) == B
    if kind == "unsorted":
        assert _engine.mol_layout(Gd)[1] is not None
    o = ro(Gd)
    _loss(o, w).backward()
    assert o.shape == (B, h)
    assert_parity(o, ref_g[0], 1e-5, "Gated")
    assert_parity(Xd.grad, ref_g[1], 1e-5, "Gated dX")
    assert_parity(ro.a.weight.grad, ref_g[2], 1e-5, "Gated da")
    # db: tests/test_gpu_readout.py::test_attention_kernel_backward's rule
    assert (ro.a.bias.grad.double().cpu() - ref_g[3]).abs().max().item() <= 1e-5 * ref_g[2].abs().max().item(), "Gated db"
    Xd = X.to(DEV).requires_grad_(True)
    Qd = Q.to(DEV).requires_grad_(True)
    o = SDPAttention(h)(G.update(node_feats=Xd).to(DEV), Q=Qd)
    _loss(o, w).backward()
    assert_parity(o, ref_q[0], 1e-5, "SDPA")
    assert_parity(Xd.grad, ref_q[1], 1e-5, "SDPA dX")
    assert_parity(Qd.grad, ref_q[2], 1e-5, "SDPA dQ")
    if kind == "empties":
        assert not o[3].any() and not o[9].any() and not Qd.grad[3].any() and not Qd.grad[9].any()


@gpu
@pytest.mark.parametrize("route", ["fp32", "mixed"])
def test_modules_query_longer_than_the_batch(route):
    """A query table with more rows than the batch has molecules (a short last batch): the forward is that of
    Q[:B], backward() runs, dQ[:B] is the oracle's and dQ[B:] is exactly 0.  ``mixed``: bf16 node rows, an
    fp32 Q, bf16 autocast; there dQ[:B] must also be the bits of the B-row query's gradient."""
    import contextlib

    from notorch_amd.nn import SDPAttention

    mixed = route == "mixed"
    G = _module_graph("unsorted")
    B, h = len(G), 36
    torch.manual_seed(50)
    X = torch.randn(G.num_nodes, h)
    Q = torch.randn(B + 3, h)
    w = torch.linspace(-1, 1, h)
    if mixed:
        X = X.to(BF16)
    cast = (lambda: torch.autocast(device_type="cuda", dtype=BF16)) if mixed else contextlib.nullcontext
    Qk = Q.to(BF16) if mixed else Q  # the key as the kernels read it
    Xr, Qr = X.double().requires_grad_(True), Qk.double().requires_grad_(True)
    ref = dmpnn_ref.readout_sdpa(Xr, G.batch_node_index, B, Qr, h ** 0.5)
    _loss(ref, w.double()).backward()
    assert not Qr.grad[B:].any()

    sdpa = SDPAttention(h)
    Xs = X.to(DEV).requires_grad_(True)
    Qs = Q[:B].clone().to(DEV).requires_grad_(True)
    with cast():
        short = sdpa(G.update(node_feats=Xs).to(DEV), Q=Qs)
    _loss(short, w).backward()

    Xd = X.to(DEV).requires_grad_(True)
    Qd = Q.to(DEV).requires_grad_(True)
    with cast():
        out = sdpa(G.update(node_feats=Xd).to(DEV), Q=Qd)
    assert out.shape == (B, h) and torch.equal(out, short)
    _loss(out, w).backward()
    assert Qd.grad.shape == Q.shape and Qd.grad.dtype == torch.float32
    assert not Qd.grad[B:].any(), "dQ rows past the batch must be exactly 0"
    assert torch.equal(Qd.grad[:B], Qs.grad) and torch.equal(Xd.grad, Xs.grad)
    tol = BF16_CEIL if mixed else 1e-5
    assert_parity(out, ref.detach(), tol, "SDPA")
    assert_parity(Qd.grad[:B], Qr.grad[:B], tol, "dQ[:B]")
    assert_parity(Xd.grad, Xr.grad, tol, "dX")


# ---------------------------------------------------------------------------------------------- E
def _bf16_rule(what, dev, torch_bf16, truth):
    e_dev, e_t = norm_err(dev, truth), norm_err(torch_bf16, truth)
    l_dev, l_t = _rel_l2(dev, truth), _rel_l2(torch_bf16, truth)
    print(f"{what}: device vs fp64 max {e_dev:.3e} L2 {l_dev:.3e}; torch bf16 vs fp64 max {e_t:.3e} L2 {l_t:.3e}")
    return [
        (e_dev <= BF16_FACTOR * e_t, f"{what}: max err {e_dev:.3e} > {BF16_FACTOR} x torch bf16 {e_t:.3e}"),
        (l_dev <= BF16_FACTOR * l_t, f"{what}: L2 err {l_dev:.3e} > {BF16_FACTOR} x torch bf16 {l_t:.3e}"),
        (e_dev <= BF16_CEIL, f"{what}: max err {e_dev:.3e} > {BF16_CEIL}"),
        (l_dev <= BF16_CEIL, f"{what}: L2 err {l_dev:.3e} > {BF16_CEIL}"),
    ]


@gpu
@pytest.mark.parametrize("h", [36, 520])
def test_bf16_storage_against_fp64(h):
    """bf16 storage (h = 36 by element, h = 520 in 16-byte pieces with a second column trip) against fp64 on
    the bf16-rounded inputs: Gated out / dX / da / db and SDPAttention out / dX / dQ, each no further than
    BF16_FACTOR x the oracle run with torch ops in bf16 on the device, and under 2e-2.  db is an
    ill-conditioned sum (0 in exact arithmetic for every molecule): its absolute error is scaled by max|da|."""
    from notorch_amd.nn import Gated, SDPAttention

    G = _qm9_graph64()
    B = len(G)
    torch.manual_seed(60 + h)
    X = torch.randn(G.num_nodes, h).to(BF16)
    Q = torch.randn(B, h).to(BF16)
    w = torch.linspace(-1, 1, h)
    ro = Gated(h).to(BF16)
    truth_g, truth_q = _fp64_module_refs(G, X, ro, Q, w)
    # the oracle with torch ops in bf16 on the device
    bni = G.batch_node_index.to(DEV)
    a, b = (t.detach().clone().to(DEV).requires_grad_(True) for t in (ro.a.weight, ro.a.bias))
    Xt = X.to(DEV).requires_grad_(True)
    o = dmpnn_ref.readout_gated(Xt, bni, B, a, b)
    assert o.dtype == BF16
    _loss(o, w).backward()
    torch_g = (o.detach(), Xt.grad, a.grad, b.grad)
    Xt, Qt = X.to(DEV).requires_grad_(True), Q.to(DEV).requires_grad_(True)
    o = dmpnn_ref.readout_sdpa(Xt, bni, B, Qt, h ** 0.5)
    assert o.dtype == BF16
    _loss(o, w).backward()
    torch_q = (o.detach(), Xt.grad, Qt.grad)
    # the kernels
    ro = ro.to(DEV)
    Xd = X.to(DEV).requires_grad_(True)
    o = ro(G.update(node_feats=Xd).to(DEV))
    assert o.dtype == BF16
    _loss(o, w).backward()
    dev_g = (o.detach(), Xd.grad, ro.a.weight.grad, ro.a.bias.grad)
    Xd, Qd = X.to(DEV).requires_grad_(True), Q.to(DEV).requires_grad_(True)
    o = SDPAttention(h)(G.update(node_feats=Xd).to(DEV), Q=Qd)
    _loss(o, w).backward()
    dev_q = (o.detach(), Xd.grad, Qd.grad)
    checks = []
    for nm, d, t, r in zip(("Gated out", "Gated dX", "Gated da"), dev_g, torch_g, truth_g):
        assert d.dtype == BF16
        checks += _bf16_rule(f"h={h} {nm}", d, t, r)
    for nm, d, t, r in zip(("SDPA out", "SDPA dX", "SDPA dQ"), dev_q, torch_q, truth_q):
        assert d.dtype == BF16
        checks += _bf16_rule(f"h={h} {nm}", d, t, r)
    scale = truth_g[2].abs().max().item()
    db_dev = (dev_g[3].double().cpu() - truth_g[3]).abs().max().item() / scale
    db_t = (torch_g[3].double().cpu() - truth_g[3]).abs().max().item() / scale
    print(f"h={h} Gated db: |device - fp64| / max|da| {db_dev:.3e}; torch bf16 {db_t:.3e}")
    checks += [(db_dev <= BF16_FACTOR * db_t, f"db: {db_dev:.3e} > {BF16_FACTOR} x torch bf16 {db_t:.3e}"),
               (db_dev <= BF16_CEIL, f"db: {db_dev:.3e} > {BF16_CEIL}")]
    failed = [msg for ok, msg in checks if not ok]
    assert not failed, "; ".join(failed)


@functools.lru_cache(maxsize=None)
def _qm9_graph64():
    from notorch_amd.data.synth import make_batch

    return make_batch("qm9", 64, seed=9).collate("nodes")
