"""CPU references for the segment-reduce and backward-gather kernel tests (test_gpu_segment_edges.py,
test_gpu_backward_edges.py), in plain torch / numpy from the formulas in the headers of
csrc/segment.hip and csrc/backward.hip (chemprop.py:28-43, :86 and agg.py:23-47 semantics).  Nothing
here calls notorch_amd.kernels; the helpers are checked on their own in test_segment_ref.py.

Every function takes ``dtype``: torch.float64 is the truth, torch.float32 the same expression in fp32
(the error floor ``err32`` of the 4 x err32 bounds, and the exact target where a kernel claims the CPU
order bit for bit).
"""
import numpy as np
import torch
import torch.nn as nn

ACTS = {
    "Identity": nn.Identity(),
    "ReLU": nn.ReLU(),
    "LeakyReLU": nn.LeakyReLU(0.1),
    "ELU": nn.ELU(1.3),
    "GELU": nn.GELU(),
    "SiLU": nn.SiLU(),
    "Tanh": nn.Tanh(),
    "Sigmoid": nn.Sigmoid(),
}


# ------------------------------------------------------------------ CSRs
def index_from_counts(counts, shuffle_seed=None) -> torch.Tensor:
    """int64 segment index per row with counts[s] rows in segment s: sorted (rows stored segment by
    segment, the perm = None layout) or shuffled by ``shuffle_seed``."""
    counts = torch.as_tensor(counts, dtype=torch.int64)
    idx = torch.repeat_interleave(torch.arange(len(counts)), counts)
    if shuffle_seed is not None:
        idx = idx[torch.randperm(len(idx), generator=torch.Generator().manual_seed(shuffle_seed))]
    return idx.contiguous()


def csr(idx: torch.Tensor, nseg: int):
    """(seg_ptr int64[nseg + 1], perm int64[n]) of the stable CSR of idx (rows of a segment ascending)."""
    perm = torch.from_numpy(np.argsort(idx.numpy(), kind="stable"))
    seg_ptr = torch.zeros(nseg + 1, dtype=torch.int64)
    seg_ptr[1:] = torch.cumsum(torch.bincount(idx, minlength=nseg), 0)
    return seg_ptr, perm


# ------------------------------------------------------------------ segment reduce
def segment_reduce_ref(X, seg_ptr, perm, reduce, act=None, dtype=torch.float64):
    """out[s] = R_{j in [seg_ptr[s], seg_ptr[s+1])} act(X[perm[j]]), visited in ascending j, one
    accumulator per (segment, column): acc += y for sum / mean, strict > / < replacement for max / min.
    Empty segments give 0; mean divides by max(n, 1).  perm = None: row j itself."""
    Y = X.to(dtype)
    if act is not None:
        Y = act(Y)
    seg_ptr = seg_ptr.to(torch.int64)
    n = seg_ptr[1:] - seg_ptr[:-1]
    nseg = n.numel()
    acc = torch.zeros(nseg, Y.shape[1], dtype=dtype)
    for k in range(int(n.max()) if nseg else 0):  # position k of every segment that has one
        live = torch.nonzero(n > k).flatten()
        pos = seg_ptr[live] + k
        y = Y[pos if perm is None else perm[pos].to(torch.int64)]
        if reduce in ("sum", "mean"):
            acc[live] = acc[live] + y
        elif k == 0:
            acc[live] = y
        else:
            a = acc[live]
            acc[live] = torch.where(y > a if reduce == "max" else y < a, y, a)
    if reduce == "mean":
        acc = acc / n.clamp(min=1).to(dtype)[:, None]
    return acc


def segment_arg_ref(Y, seg_ptr, perm, reduce) -> torch.Tensor:
    """int32 nseg x h: the first row in CSR order holding each column's max / min of Y (strict > / <),
    -1 for empty segments.  A plain loop over segments and their rows."""
    Y = Y.numpy()
    seg_ptr = seg_ptr.numpy()
    nseg, h = len(seg_ptr) - 1, Y.shape[1]
    arg = np.full((nseg, h), -1, dtype=np.int32)
    for s in range(nseg):
        best = None
        for j in range(seg_ptr[s], seg_ptr[s + 1]):
            r = j if perm is None else int(perm[j])
            y = Y[r]
            if best is None:
                best = y.copy()
                arg[s, :] = r
                continue
            better = y > best if reduce == "max" else y < best
            best[better] = y[better]
            arg[s, better] = r
    return torch.from_numpy(arg)


# ------------------------------------------------------------------ backward gathers
def act_grad_ref(H, act, dtype=torch.float64):
    """act'(H) by autograd in ``dtype`` (no derivative formula of our own)."""
    x = H.detach().to(dtype).clone().requires_grad_(True)
    act(x).sum().backward()
    return x.grad


def counts(idx, nseg, dtype=torch.float64):
    """max(rows of segment s, 1): the mean's divisor."""
    return torch.bincount(idx, minlength=nseg).clamp(min=1).to(dtype)


def message_ref(H, S, src, rev, act, dtype=torch.float64):
    """A[e] = S[src e] - act(H[rev e])."""
    return S.to(dtype)[src] - act(H.to(dtype))[rev]


def _rev_scatter(dA, rev, dtype):
    return torch.zeros(dA.shape, dtype=dtype).index_add_(0, rev, dA.to(dtype))


def edge_backward_ref(G, H, dA, dS, dst, rev, act, reduce="sum", dtype=torch.float64):
    """(G or 0) + act'(H[e]) * (dS[dst e] / c_{dst e} - sum_{e': rev e' = e} dA[e']); c = in-degree
    (at least 1) for mean, 1 for sum.  G = None: no residual term."""
    dm = dS.to(dtype)
    if reduce == "mean":
        dm = dm / counts(dst, dS.shape[0], dtype)[:, None]
    out = act_grad_ref(H, act, dtype) * (dm[dst] - _rev_scatter(dA, rev, dtype))
    return out if G is None else G.to(dtype) + out


def edge_backward_arg_ref(G, H, dA, dS, arg, dst, rev, act, dtype=torch.float64):
    """as edge_backward_ref with dS[dst e] reaching row e only where arg[dst e, column] == e."""
    e = torch.arange(H.shape[0])[:, None]
    dm = torch.where(arg.to(torch.int64)[dst] == e, dS.to(dtype)[dst], torch.zeros((), dtype=dtype))
    out = act_grad_ref(H, act, dtype) * (dm - _rev_scatter(dA, rev, dtype))
    return out if G is None else G.to(dtype) + out


def gather_rows_ref(X, idx, base=None, mean_idx_counts=None, dtype=torch.float64):
    """out[i] = (base[i] or 0) + X[idx i] / c_{idx i}; mean_idx_counts = counts(...) or None (c = 1)."""
    x = X.to(dtype)
    if mean_idx_counts is not None:
        x = x / mean_idx_counts.to(dtype)[:, None]
    out = x[idx]
    return out if base is None else base.to(dtype) + out


def gather_rows_arg_ref(X, idx, arg, base=None, dtype=torch.float64):
    """out[i] = (base[i] or 0) + (arg[idx i] == i ? X[idx i] : 0)."""
    i = torch.arange(idx.numel())[:, None]
    out = torch.where(arg.to(torch.int64)[idx] == i, X.to(dtype)[idx], torch.zeros((), dtype=dtype))
    return out if base is None else base.to(dtype) + out
