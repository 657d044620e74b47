"""Tensor-level wrappers over the C-ABI (``include/notorch_amd.h``).

Each wrapper validates device / dtype / shape / contiguity up front (raising ``TypeError`` /
``ValueError`` the way the reference's ATen ops would raise for bad inputs), allocates outputs with
``torch.empty`` on the tensor's device (PyTorch's caching allocator owns all memory) and launches on
``torch.cuda.current_stream()``.  Nothing here computes on the host: a CPU tensor is an error.
"""
from __future__ import annotations

import ctypes

import torch
from torch import Tensor

from notorch_amd import _lib
from notorch_amd._lib import NT_BF16, NT_F32, REDUCE_CODES, check

__all__ = [
    "csr_build",
    "dmpnn_init",
    "segment_reduce",
    "dmpnn_aggregate",
    "chunk_plan",
    "pack_weights",
    "dmpnn_update",
    "tile_plan",
    "tile_stride",
    "fused_tile_rows",
    "absmax",
    "dmpnn_row_table",
    "fused_supported",
    "dmpnn_update_fused",
    "act_code",
    "reduce_code",
    "dmpnn_message",
    "dmpnn_edge_backward",
    "gather_rows",
    "embed_bag",
    "dmpnn_init_embed",
    "embed_edge_records",
    "embed_bag_backward",
    "node_scores",
    "softmax_pool",
    "dense_matmul",
    "weight_grad",
    "segment_arg",
    "dmpnn_edge_backward_arg",
    "gather_rows_arg",
    "pack_weights_mixed",
    "dmpnn_init_mixed",
    "dmpnn_init_embed_mixed",
    "node_scores_mixed",
    "softmax_pool_backward_mixed",
    "rnc_max_n",
    "rnc_rank",
    "rnc_long_max_n",
    "rnc_rank_long",
    "task_loss",
    "task_loss_single_max",
    "rank_metric",
    "rank_metric_long",
    "rank_metric_long_max_n",
    "rank_metric_max_n",
]


def _ptr(t: Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _run(dev: torch.device, fn, *args) -> None:
    """Call a C-ABI entry point with ``dev`` as the current HIP device (the library queries the
    current device for its CU count and kernel attributes; the launch goes to dev's stream)."""
    if dev.index is not None and dev.index != torch.cuda.current_device():
        with torch.cuda.device(dev):
            check(fn(*args))
    else:
        check(fn(*args))


def _require_device(*ts: Tensor | None) -> torch.device:
    dev = None
    for t in ts:
        if t is None:
            continue
        if t.device.type != "cuda":
            raise RuntimeError(
                "notorch_amd kernels run on ROCm devices only; got a tensor on "
                f"'{t.device}'. Move the graph with G.to('cuda') first."
            )
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"tensors on different devices: {dev} vs {t.device}")
    assert dev is not None
    return dev


def _require_f32(name: str, t: Tensor) -> None:
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 on the fp32 kernel path, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


_DTYPE_CODES = {torch.float32: NT_F32, torch.bfloat16: NT_BF16}


def _require_feat(name: str, t: Tensor, dtype: torch.dtype | None = None) -> int:
    """Feature tensor on the kernel path: fp32 or bf16 (all operands of one call share it), contiguous.
    Returns the C-ABI dtype code."""
    if t.dtype not in _DTYPE_CODES:
        raise TypeError(f"{name} must be float32 or bfloat16, got {t.dtype}")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} is {t.dtype} but the other operands are {dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return _DTYPE_CODES[t.dtype]


def _row_pitch(name: str, t: Tensor, dtype: torch.dtype | None = None) -> int:
    """Row pitch (elements) of a 2-D feature tensor that is contiguous or a row-padded view
    (X[:, :h] of an [n, ld] fp32 buffer: unit column stride, 16-byte row pitch)."""
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D")
    if t.is_contiguous():
        _require_feat(name, t, dtype)
        return t.shape[1]
    if t.dtype != torch.float32 or t.stride(1) != 1 or t.stride(0) < t.shape[1] or t.stride(0) % 4:
        raise ValueError(f"{name} must be contiguous (or an fp32 row-padded view with a pitch % 4 == 0)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} is {t.dtype} but the other operands are {dtype}")
    return t.stride(0)


def padded_rows(n: int, h: int, pitch: int, dtype: torch.dtype, device) -> Tensor:
    """An n x h tensor whose rows sit ``pitch`` elements apart (a view of an n x pitch buffer)."""
    if pitch == h:
        return torch.empty(n, h, dtype=dtype, device=device)
    return torch.empty(max(n, 1), pitch, dtype=dtype, device=device)[:n, :h]


def _require_i64(name: str, t: Tensor) -> None:
    if t.dtype != torch.int64:
        raise TypeError(f"{name} must be int64 (reference index dtype), got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def reduce_code(reduce: str) -> int:
    try:
        return REDUCE_CODES[reduce]
    except KeyError:
        raise ValueError(f"unsupported reduce '{reduce}', expected one of {list(REDUCE_CODES)}")


def act_code(act: torch.nn.Module) -> tuple[int, float]:
    """Map an activation module instance to the kernel's (code, alpha)."""
    nn = torch.nn
    if isinstance(act, nn.ReLU):
        return _lib.NT_ACT_RELU, 0.0
    if isinstance(act, nn.Identity):
        return _lib.NT_ACT_IDENTITY, 0.0
    if isinstance(act, nn.LeakyReLU):
        return _lib.NT_ACT_LEAKY_RELU, float(act.negative_slope)
    if isinstance(act, nn.ELU):
        return _lib.NT_ACT_ELU, float(act.alpha)
    if isinstance(act, nn.GELU):
        if act.approximate != "none":
            raise NotImplementedError("GELU(approximate='tanh') is not implemented in the kernels")
        return _lib.NT_ACT_GELU, 0.0
    if isinstance(act, nn.SiLU):
        return _lib.NT_ACT_SILU, 0.0
    if isinstance(act, nn.Tanh):
        return _lib.NT_ACT_TANH, 0.0
    if isinstance(act, nn.Sigmoid):
        return _lib.NT_ACT_SIGMOID, 0.0
    raise NotImplementedError(
        f"activation {type(act).__name__} has no kernel implementation "
        "(supported: ReLU, Identity, LeakyReLU, ELU, GELU, SiLU, Tanh, Sigmoid)"
    )


def csr_build(idx: Tensor, nseg: int, *, check_bounds: bool = True) -> tuple[Tensor, Tensor]:
    """Stable CSR of an int64 index vector: (seg_ptr[nseg+1] int32, perm[n] int32).

    ``check_bounds`` synchronises once to raise ``IndexError`` for out-of-range indices, like the
    reference's scatter would; the kernel itself never reads or writes out of bounds.
    """
    dev = _require_device(idx)
    _require_i64("idx", idx)
    if idx.dim() != 1:
        raise ValueError("idx must be 1-D")
    n = idx.numel()
    if nseg < 0:
        raise ValueError("nseg must be >= 0")
    lib = _lib.load()
    seg_ptr = torch.empty(nseg + 1, dtype=torch.int32, device=dev)
    perm = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
    ws_bytes = lib.nt_csr_workspace_bytes(n, nseg)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _run(dev, lib.nt_csr_build,
         _ptr(idx), n, nseg, _ptr(seg_ptr), _ptr(perm), _ptr(ws), ws_bytes, _ptr(err), _stream(dev))
    if check_bounds and n > 0 and int(err.item()) != 0:
        raise IndexError(f"index out of range for a scatter into {nseg} rows")
    return seg_ptr, perm


def dmpnn_init(
    Xv: Tensor,
    Xe: Tensor,
    src: Tensor,
    seg_ptr: Tensor | None = None,
    perm: Tensor | None = None,
    *,
    act: tuple[int, float] = (_lib.NT_ACT_RELU, 0.0),
    reduce: str = "sum",
    amax: Tensor | None = None,
    pitch: int | None = None,
    skip_degree: int = 0,
) -> tuple[Tensor, Tensor | None]:
    """H0 = Xv[src] + Xe, optionally fused with S = scatter(act(H0), dst) (needs the dst CSR).
    skip_degree (fp32, with S, h >= 128): nodes with more in-edges are left out (their H0 rows and S
    row are then dmpnn_init_chunked's with chunk_ids = their chunks).
    amax (fp32, 2 zero-filled device floats): raised to max|H0|, max|S| (layer 0's amax_in).
    pitch (fp32, h % 4 == 0, h >= 128 with the aggregation): H0 and S as row-padded views whose rows
    sit ``pitch`` floats apart (nt_dmpnn_init's ld_out)."""
    dev = _require_device(Xv, Xe, src, seg_ptr, perm, amax)
    _require_amax(amax, Xv.dtype)
    code = _require_feat("node_feats", Xv)
    _require_feat("edge_feats", Xe, Xv.dtype)
    _require_i64("src", src)
    if Xv.dim() != 2 or Xe.dim() != 2 or Xv.shape[1] != Xe.shape[1]:
        raise RuntimeError(
            f"node_feats {tuple(Xv.shape)} and edge_feats {tuple(Xe.shape)} must be V x h and E x h"
        )
    V, h = Xv.shape
    E = Xe.shape[0]
    if src.numel() != E:
        raise ValueError("src must have one entry per edge")
    ld = h if pitch is None else int(pitch)
    H0 = padded_rows(E, h, ld, Xv.dtype, dev)
    S = None
    if seg_ptr is not None:
        S = padded_rows(V, h, ld, Xv.dtype, dev)
    lib = _lib.load()
    _run(dev, lib.nt_dmpnn_init,
         _ptr(Xv), _ptr(Xe), _ptr(src), _ptr(seg_ptr), _ptr(perm), V, E, h, act[0], act[1],
         reduce_code(reduce), code, _ptr(H0), _ptr(S), _ptr(amax), 0 if ld == h else ld, int(skip_degree),
         _stream(dev))
    return H0, S


def _require_amax(amax: Tensor | None, dtype: torch.dtype, n: int = 2) -> None:
    if amax is None:
        return
    if dtype != torch.float32:
        raise ValueError("amax is fp32 only")
    if amax.dtype != torch.float32 or amax.numel() < n or not amax.is_contiguous():
        raise ValueError(f"amax must be a contiguous float32 device tensor of {n} elements")


def absmax(X: Tensor, out: Tensor | None = None) -> Tensor:
    """max |X| (fp32) into out[0] (a 1-element float32 device tensor, zero-filled if not given)."""
    dev = _require_device(X, out)
    _require_f32("X", X)
    if not X.is_contiguous():
        raise ValueError("absmax: X must be contiguous")
    if out is None:
        out = torch.zeros(1, dtype=torch.float32, device=dev)
    _run(dev, _lib.load().nt_absmax, _ptr(X), X.numel(), NT_F32, _ptr(out), _stream(dev))
    return out


def segment_reduce(
    X: Tensor,
    seg_ptr: Tensor,
    perm: Tensor | None,
    nseg: int,
    *,
    reduce: str = "sum",
    act: tuple[int, float] = (_lib.NT_ACT_IDENTITY, 0.0),
    out: Tensor | None = None,
) -> Tensor:
    """out[s] = reduce over rows X[perm[j]] (j in segment s) of act(row); empty segment -> 0."""
    dev = _require_device(X, seg_ptr, perm)
    code = _require_feat("X", X)
    if out is not None:
        _require_feat("out", out, X.dtype)
    if X.dim() != 2:
        raise ValueError("X must be 2-D")
    if seg_ptr.dtype != torch.int32 or seg_ptr.numel() != nseg + 1:
        raise ValueError("seg_ptr must be int32 of length nseg + 1")
    h = X.shape[1]
    if out is None:
        out = torch.empty(nseg, h, dtype=X.dtype, device=dev)
    if X.shape[0] == 0:  # no rows (an edge-free batch): every segment is empty -> 0 (torch_scatter)
        return out.zero_()
    lib = _lib.load()
    _run(dev, lib.nt_segment_reduce,
         _ptr(X), _ptr(seg_ptr), _ptr(perm), nseg, h, reduce_code(reduce), act[0], act[1], code,
         _ptr(out), _stream(dev))
    return out


def dmpnn_aggregate(H: Tensor, row_ptr: Tensor, perm: Tensor, V: int, *, reduce: str = "sum") -> Tensor:
    """S[v] = reduce over v's in-edges of relu(H[e]) (chemprop.py:36-39) through nt_dmpnn_aggregate
    (the dst CSR of nt_csr_build: row_ptr int32[V+1], perm int32[E])."""
    dev = _require_device(H, row_ptr, perm)
    code = _require_feat("H", H)
    if H.dim() != 2:
        raise ValueError("H must be 2-D")
    if row_ptr.dtype != torch.int32 or row_ptr.numel() != V + 1 or not row_ptr.is_contiguous():
        raise ValueError("row_ptr must be contiguous int32 of length V + 1")
    if perm.dtype != torch.int32 or perm.numel() != H.shape[0] or not perm.is_contiguous():
        raise ValueError("perm must be contiguous int32 with one entry per row of H")
    S = torch.empty(V, H.shape[1], dtype=H.dtype, device=dev)
    if H.shape[0] == 0:
        return S.zero_()
    _run(dev, _lib.load().nt_dmpnn_aggregate,
         _ptr(H), _ptr(row_ptr), _ptr(perm), V, H.shape[1], reduce_code(reduce), code, _ptr(S), _stream(dev))
    return S


CHUNK_ROWS = 32  # rows per chunk of the load-balanced segment reduce


def chunk_plan(seg_ptr: Tensor, chunk: int = CHUNK_ROWS) -> tuple:
    """(chunk_pos[nchunks+1], nchunks, chunk_ptr[nseg+1], chunk_seg[nchunks], comb_seg[ncomb]) for
    nt_segment_reduce_chunked: every segment cut into chunks of at most ``chunk`` CSR positions;
    chunk_seg[k] = the segment of chunk k when it is that segment's only chunk (pass 1 stores its
    result directly), else -1; comb_seg = the segments with != 1 chunk (pass 2's list).  Device ops;
    one host sync (the two counts)."""
    _require_device(seg_ptr)
    dev = seg_ptr.device
    sp = seg_ptr.to(torch.int64)
    n = sp[1:] - sp[:-1]
    nch = (n + chunk - 1) // chunk
    chunk_ptr64 = torch.zeros(n.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(nch, 0, out=chunk_ptr64[1:])
    multi = nch != 1
    nchunks, ncomb = (int(x) for x in torch.stack([chunk_ptr64[-1], multi.sum()]).tolist())
    seg_of = torch.repeat_interleave(torch.arange(n.numel(), device=dev), nch, output_size=nchunks)
    k_in_seg = torch.arange(nchunks, device=dev) - chunk_ptr64[seg_of]
    chunk_pos = torch.empty(nchunks + 1, dtype=torch.int32, device=dev)
    chunk_pos[:nchunks] = (sp[seg_of] + k_in_seg * chunk).to(torch.int32)
    chunk_pos[nchunks] = seg_ptr[-1]
    chunk_seg = torch.where(multi[seg_of], -1, seg_of).to(torch.int32)
    comb_seg = torch.nonzero(multi).flatten().to(torch.int32)
    assert comb_seg.numel() == ncomb
    return chunk_pos, nchunks, chunk_ptr64.to(torch.int32), chunk_seg, comb_seg


def _chunk_args(plan, nseg: int):
    """ctypes arguments (chunk_pos, nchunks, chunk_ptr, chunk_seg, comb_seg, ncomb) of a chunk plan."""
    if len(plan) != 5:
        raise ValueError("plan must be chunk_plan(seg_ptr): (chunk_pos, nchunks, chunk_ptr, chunk_seg, comb_seg)")
    chunk_pos, nchunks, chunk_ptr, chunk_seg, comb_seg = plan
    for name, t in (("chunk_pos", chunk_pos), ("chunk_ptr", chunk_ptr), ("chunk_seg", chunk_seg),
                    ("comb_seg", comb_seg)):
        if t.dtype != torch.int32:
            raise TypeError(f"{name} must be int32")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if (chunk_pos.numel() != nchunks + 1 or chunk_ptr.numel() != nseg + 1 or chunk_seg.numel() != nchunks
            or comb_seg.numel() > nseg):
        raise ValueError("plan must be chunk_plan(seg_ptr) of this CSR")
    return _ptr(chunk_pos), nchunks, _ptr(chunk_ptr), _ptr(chunk_seg), _ptr(comb_seg), comb_seg.numel()


def segment_reduce_chunked(
    X: Tensor,
    seg_ptr: Tensor,
    perm: Tensor | None,
    nseg: int,
    plan: tuple[Tensor, int, Tensor],
    *,
    reduce: str = "sum",
    act: tuple[int, float] = (_lib.NT_ACT_IDENTITY, 0.0),
    out: Tensor | None = None,
    amax: Tensor | None = None,
) -> Tensor:
    """segment_reduce load-balanced over chunks (plan = chunk_plan(seg_ptr)) for skewed segments;
    fp32: amax (1 zero-filled device float, optional) is raised to max|out|."""
    dev = _require_device(X, seg_ptr, perm, amax)
    code = _require_feat("X", X)
    if seg_ptr.dtype != torch.int32 or seg_ptr.numel() != nseg + 1:
        raise ValueError("seg_ptr must be int32 of length nseg + 1")
    cargs = _chunk_args(plan, nseg)
    nchunks = plan[1]
    h = X.shape[1]
    if out is None:
        out = torch.empty(nseg, h, dtype=X.dtype, device=dev)
    else:
        _require_feat("out", out, X.dtype)
    partial = torch.empty(max(nchunks, 1), h, dtype=torch.float32, device=dev)
    _run(dev, _lib.load().nt_segment_reduce_chunked,
         _ptr(X), _ptr(perm), *cargs, _ptr(seg_ptr), nseg, h,
         reduce_code(reduce), act[0], act[1], code, _ptr(partial), _ptr(out), _ptr(amax), _stream(dev))
    return out


def dmpnn_init_chunked(
    Xv: Tensor,
    Xe: Tensor,
    src: Tensor,
    seg_ptr: Tensor,
    perm: Tensor,
    plan: tuple[Tensor, int, Tensor],
    *,
    act: tuple[int, float] = (_lib.NT_ACT_IDENTITY, 0.0),
    reduce: str = "sum",
    amax: Tensor | None = None,
    pitch: int | None = None,
    H0: Tensor | None = None,
    S: Tensor | None = None,
    chunk_ids: Tensor | None = None,
) -> tuple[Tensor, Tensor]:
    """(H0, S) = dmpnn_init with layer 0's aggregation over the chunk plan of a hub graph (fp32,
    plan = chunk_plan(seg_ptr)): H0 written once, S combined from per-chunk partials.  amax (2
    zero-filled device floats, optional) raised to max|H0|, max|S|.  pitch: H0 and S as row-padded
    views (as dmpnn_init's)."""
    nchunks = plan[1]
    dev = _require_device(Xv, Xe, src, seg_ptr, perm, plan[0], plan[2], amax)
    if Xv.dtype != torch.float32 or Xe.dtype != torch.float32:
        raise ValueError("dmpnn_init_chunked is fp32 only")
    _require_amax(amax, Xv.dtype)
    _require_i64("src", src)
    for name, t in (("seg_ptr", seg_ptr), ("perm", perm)):
        if t.dtype != torch.int32:
            raise TypeError(f"{name} must be int32")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    V, h = Xv.shape
    E = Xe.shape[0]
    if Xe.shape[1] != h or src.numel() != E or perm.numel() != E or seg_ptr.numel() != V + 1:
        raise ValueError("shape mismatch between Xv, Xe, src and the dst CSR")
    cargs = _chunk_args(plan, V)
    ld = h if pitch is None else int(pitch)
    if H0 is None:
        H0 = padded_rows(E, h, ld, torch.float32, dev)
    if S is None:
        S = padded_rows(V, h, ld, torch.float32, dev)
    if H0.shape != (E, h) or S.shape != (V, h) or _row_pitch("H0", H0) != ld or _row_pitch("S", S) != ld:
        raise ValueError("H0 / S must be E x h / V x h with the given row pitch")
    if chunk_ids is not None and (chunk_ids.dtype != torch.int32 or not chunk_ids.is_contiguous()
                                  or chunk_ids.numel() > nchunks):
        raise ValueError("chunk_ids must be contiguous int32 chunk indices of the plan")
    partial = torch.empty(max(nchunks, 1), h, dtype=torch.float32, device=dev)
    _run(dev, _lib.load().nt_dmpnn_init_chunked,
         _ptr(Xv.contiguous()), _ptr(Xe.contiguous()), _ptr(src), _ptr(perm), *cargs, _ptr(seg_ptr), V, E, h, act[0], act[1], reduce_code(reduce), _DTYPE_CODES[torch.float32],
         _ptr(partial), _ptr(H0), _ptr(S), _ptr(amax), 0 if ld == h else ld, _ptr(chunk_ids),
         0 if chunk_ids is None else chunk_ids.numel(), _stream(dev))
    return H0, S


def packed_weight_numel(h: int, dtype: torch.dtype = torch.float32) -> int:
    """Size (in 4-byte words) of one layer's packed weight image for feature dtype ``dtype``."""
    return _lib.load().nt_dmpnn_packed_weight_bytes(h, _DTYPE_CODES[dtype]) // 4


def pack_weights(W: Tensor, *, fk_only: bool = False) -> Tensor:
    """Pack one nn.Linear weight [h, h] (or a stack [L, h, h]) into the MFMA fragment image of its
    dtype (fp32: the two-part fp16 image of the fp32 layer kernel, or for h % 4 != 0 the fp32 fragment image;
    bf16: one bf16 fragment image, h <= 512 or h % 8 == 0 up to 8192).  The image is an opaque
    float32-typed buffer.  fk_only (fp32): only the part nt_dmpnn_update_fused / dense_matmul read
    (nt_dmpnn_pack_weight_fk)."""
    dev = _require_device(W)
    code = _require_feat("weight", W)
    if W.dim() == 2:
        W3 = W.unsqueeze(0)
    else:
        W3 = W
    L, h, h2 = W3.shape
    if h != h2:
        raise ValueError(f"ChempropLayer weight must be square, got {tuple(W.shape)}")
    Wp = torch.empty(L, packed_weight_numel(h, W.dtype), dtype=torch.float32, device=dev)
    lib = _lib.load()
    if fk_only and W.dtype == torch.float32:
        W3 = W3.contiguous()
        _run(dev, lib.nt_dmpnn_pack_weight_fk, _ptr(W3), L, h, _ptr(Wp), _stream(dev))
    else:
        _run(dev, lib.nt_dmpnn_pack_weight, _ptr(W3), L, h, code, _ptr(Wp), _stream(dev))
    return Wp[0] if W.dim() == 2 else Wp


def pack_weights_fk_multi(Ws: Sequence[Tensor], with_t: bool = False) -> tuple[list[Tensor], list[Tensor] | None]:
    """fp32: the fk images (nt_dmpnn_pack_weight_fk's part of pack_weights) of up to 16 separate h x h
    weights and, with ``with_t``, of their transposes (the backward's dA image), in one launch pair
    (nt_dmpnn_pack_weights_fk).  Bytes equal pack_weights(W, fk_only=True) and
    pack_weights(W.t().contiguous(), fk_only=True)."""
    if not Ws:
        return [], ([] if with_t else None)
    dev = _require_device(*Ws)
    h = Ws[0].shape[0]
    for W in Ws:
        _require_f32("weight", W)
        if W.shape != (h, h) or not W.is_contiguous():
            raise ValueError("pack_weights_fk_multi: contiguous h x h weights of one hidden size")
    if len(Ws) > 16:
        raise ValueError("pack_weights_fk_multi: at most 16 weights per call")
    n = packed_weight_numel(h, torch.float32)
    imgs = [torch.empty(n, dtype=torch.float32, device=dev) for _ in Ws]
    imgsT = [torch.empty(n, dtype=torch.float32, device=dev) for _ in Ws] if with_t else None
    arr = ctypes.c_void_p * len(Ws)
    _run(dev, _lib.load().nt_dmpnn_pack_weights_fk, arr(*[W.data_ptr() for W in Ws]), len(Ws), h,
         arr(*[t.data_ptr() for t in imgs]), None if imgsT is None else arr(*[t.data_ptr() for t in imgsT]),
         _stream(dev))
    return imgs, imgsT


# ------------------------------------------------------------------------------------ mixed precision
def bf16_h_supported(h: int) -> bool:
    """Hidden sizes of the bf16 storage path (NT_BF16_H_RULE): h <= 512, or h % 8 == 0 up to 8192."""
    return h >= 1 and (h <= 512 or (h % 8 == 0 and h <= 8192))


def pack_weights_mixed(Ws: Sequence[Tensor], biases: Sequence[Tensor | None] | None = None,
                       with_t: bool = False) -> tuple[list[Tensor], list[Tensor] | None, list[Tensor | None]]:
    """The bf16 fragment images of up to 16 separate h x h weights of one dtype (fp32 master weights, or
    bf16), with ``with_t`` of their transposes (the backward's dA image), and the bf16 copies of the
    given biases (same dtype as the weights; None entries stay None), in one launch
    (nt_dmpnn_pack_weights_mixed).  Bytes equal pack_weights(W.to(bfloat16)),
    pack_weights(W.t().contiguous().to(bfloat16)) and b.to(bfloat16).
    Returns (images, transpose images or None, bf16 biases)."""
    if not Ws:
        return [], ([] if with_t else None), []
    if biases is None:
        biases = [None] * len(Ws)
    dev = _require_device(*Ws, *biases)
    h = Ws[0].shape[0]
    dtype = Ws[0].dtype
    code = _require_feat("weight", Ws[0])
    if len(Ws) > 16:
        raise ValueError("pack_weights_mixed: at most 16 weights per call")
    if len(biases) != len(Ws):
        raise ValueError("pack_weights_mixed: one bias (or None) per weight")
    if not bf16_h_supported(h):
        raise ValueError(f"pack_weights_mixed: the bf16 path needs h <= 512, or h % 8 == 0 and h <= 8192; got {h}")
    for W in Ws:
        _require_feat("weight", W, dtype)
        if W.shape != (h, h):
            raise ValueError("pack_weights_mixed: h x h weights of one hidden size")
    for b in biases:
        if b is not None:
            _require_feat("bias", b, dtype)
            if b.shape != (h,):
                raise ValueError("pack_weights_mixed: a bias has h elements")
    n = packed_weight_numel(h, torch.bfloat16)
    imgs = [torch.empty(n, dtype=torch.float32, device=dev) for _ in Ws]
    imgsT = [torch.empty(n, dtype=torch.float32, device=dev) for _ in Ws] if with_t else None
    b16 = [None if b is None else torch.empty(h, dtype=torch.bfloat16, device=dev) for b in biases]
    arr = ctypes.c_void_p * len(Ws)
    any_b = any(b is not None for b in biases)
    _run(dev, _lib.load().nt_dmpnn_pack_weights_mixed, arr(*[W.data_ptr() for W in Ws]), len(Ws), h, code,
         arr(*[t.data_ptr() for t in imgs]), None if imgsT is None else arr(*[t.data_ptr() for t in imgsT]),
         arr(*[_ptr(b) for b in biases]) if any_b else None, arr(*[_ptr(t) for t in b16]) if any_b else None,
         _stream(dev))
    return imgs, imgsT, b16


def _require_dst_csr(seg_ptr: Tensor | None, perm: Tensor | None, V: int, E: int) -> None:
    if (seg_ptr is None) != (perm is None):
        raise ValueError("the dst CSR needs both seg_ptr and perm")
    if seg_ptr is None:
        return
    if seg_ptr.dtype != torch.int32 or seg_ptr.numel() != V + 1 or not seg_ptr.is_contiguous():
        raise ValueError("seg_ptr must be contiguous int32 of length V + 1")
    if perm.dtype != torch.int32 or perm.numel() != E or not perm.is_contiguous():
        raise ValueError("perm must be contiguous int32 with one entry per edge")


def dmpnn_init_mixed(
    Xv: Tensor,
    Xe: Tensor,
    src: Tensor,
    seg_ptr: Tensor | None = None,
    perm: Tensor | None = None,
    *,
    act: tuple[int, float] = (_lib.NT_ACT_RELU, 0.0),
    reduce: str = "sum",
) -> tuple[Tensor, Tensor | None]:
    """dmpnn_init from fp32 Xv / Xe to bf16 outputs (nt_dmpnn_init_mixed): H0 = bf16(Xv[src] + Xe), added
    in fp32 and rounded once, optionally fused with S = scatter(act(H0), dst) (needs the dst CSR;
    the bits of segment_reduce over that H0).  Rows of whole 16-byte pieces (h % 8 == 0) or 8-byte pieces
    (h % 4 == 0) of 16-byte aligned tensors (the allocator's alignment) move as vectors, other rows by
    element."""
    dev = _require_device(Xv, Xe, src, seg_ptr, perm)
    _require_f32("node_feats", Xv)
    _require_f32("edge_feats", Xe)
    _require_i64("src", src)
    if Xv.dim() != 2 or Xe.dim() != 2 or Xv.shape[1] != Xe.shape[1]:
        raise RuntimeError(
            f"node_feats {tuple(Xv.shape)} and edge_feats {tuple(Xe.shape)} must be V x h and E x h"
        )
    V, h = Xv.shape
    E = Xe.shape[0]
    if src.numel() != E:
        raise ValueError("src must have one entry per edge")
    if not bf16_h_supported(h):
        raise ValueError(f"dmpnn_init_mixed: the bf16 path needs h <= 512, or h % 8 == 0 and h <= 8192; got {h}")
    _require_dst_csr(seg_ptr, perm, V, E)
    H0 = torch.empty(E, h, dtype=torch.bfloat16, device=dev)
    S = None if seg_ptr is None else torch.empty(V, h, dtype=torch.bfloat16, device=dev)
    _run(dev, _lib.load().nt_dmpnn_init_mixed,
         _ptr(Xv), _ptr(Xe), _ptr(src), _ptr(seg_ptr), _ptr(perm), V, E, h, act[0], act[1],
         reduce_code(reduce), _ptr(H0), _ptr(S), _stream(dev))
    return H0, S


def dmpnn_init_embed_mixed(
    node_table: Tensor,
    node_types: Tensor,
    edge_table: Tensor,
    edge_types: Tensor,
    src: Tensor,
    seg_ptr: Tensor | None = None,
    perm: Tensor | None = None,
    *,
    act: tuple[int, float] = (_lib.NT_ACT_RELU, 0.0),
    reduce: str = "sum",
    validate: bool = True,
) -> tuple[Tensor, Tensor | None]:
    """dmpnn_init_embed from fp32 tables to bf16 outputs (nt_dmpnn_init_embed_mixed): the bits of
    embed_bag (fp32) twice followed by dmpnn_init_mixed, with Xv / Xe never written."""
    dev = _require_device(node_table, node_types, edge_table, edge_types, src, seg_ptr, perm)
    _require_f32("node_table", node_table)
    _require_f32("edge_table", edge_table)
    if node_table.dim() != 2 or edge_table.dim() != 2 or node_table.shape[1] != edge_table.shape[1]:
        raise RuntimeError("node and edge embedding tables must share the hidden dimension")
    if validate:
        _check_types("node_types", node_types, node_table.shape[0])
        _check_types("edge_types", edge_types, edge_table.shape[0])
    else:
        _require_i64("node_types", node_types)
        _require_i64("edge_types", edge_types)
        if node_types.dim() != 2 or edge_types.dim() != 2:
            raise ValueError("type indices must be n x k")
    _require_i64("src", src)
    V, kv = node_types.shape
    E, ke = edge_types.shape
    h = node_table.shape[1]
    if src.numel() != E:
        raise ValueError("src must have one entry per edge")
    if not bf16_h_supported(h):
        raise ValueError(f"dmpnn_init_embed_mixed: the bf16 path needs h <= 512, or h % 8 == 0 and h <= 8192; got {h}")
    _require_dst_csr(seg_ptr, perm, V, E)
    H0 = torch.empty(E, h, dtype=torch.bfloat16, device=dev)
    S = None if seg_ptr is None else torch.empty(V, h, dtype=torch.bfloat16, device=dev)
    _run(dev, _lib.load().nt_dmpnn_init_embed_mixed,
         _ptr(node_table), node_table.shape[0], _ptr(node_types), kv, _ptr(edge_table),
         edge_table.shape[0], _ptr(edge_types), ke, _ptr(src), _ptr(seg_ptr), _ptr(perm), V, E, h,
         act[0], act[1], reduce_code(reduce), _ptr(H0), _ptr(S), _stream(dev))
    return H0, S


def dmpnn_update(
    H: Tensor,
    S: Tensor,
    src: Tensor,
    rev: Tensor,
    Wp: Tensor,
    bias: Tensor | None,
    *,
    residual: bool = True,
    act: tuple[int, float] = (_lib.NT_ACT_RELU, 0.0),
    out: Tensor | None = None,
) -> Tensor:
    """H_out = (residual ? H : 0) + (S[src] - act(H[rev])) @ W^T + b   (one fused launch)."""
    dev = _require_device(H, S, src, rev, Wp, bias, out)
    code = _require_feat("H", H)
    _require_feat("S", S, H.dtype)
    _require_i64("src", src)
    _require_i64("rev_index", rev)
    E, h = H.shape
    V = S.shape[0]
    if S.shape[1] != h or src.numel() != E or rev.numel() != E:
        raise ValueError("shape mismatch between H, S, src and rev_index")
    if Wp.numel() != packed_weight_numel(h, H.dtype):
        raise ValueError(f"Wp is not a packed {H.dtype} weight image for this hidden size")
    if bias is not None:
        _require_feat("bias", bias, H.dtype)
        if bias.numel() != h:
            raise ValueError("bias must have h entries")
    if out is None:
        out = torch.empty_like(H)
    else:
        _require_feat("out", out, H.dtype)
    lib = _lib.load()
    # fp32 split scales: a 2-float device workspace owned by the caller (ABI 6), allocated on the
    # current stream by the caching allocator, so its reuse is stream-ordered
    ws = torch.empty(2, dtype=torch.float32, device=dev) if code == NT_F32 and h % 4 == 0 else None
    _run(dev, lib.nt_dmpnn_update,
         _ptr(H), _ptr(S), _ptr(src), _ptr(rev), _ptr(Wp), _ptr(bias), V, E, h, int(residual),
         act[0], act[1], code, _ptr(ws), _ptr(out), _stream(dev))
    return out


def fused_supported(V: int, E: int, h: int, dtype: torch.dtype = torch.float32) -> bool:
    """Shapes nt_dmpnn_update_fused accepts: the fp32 fk kernel (h % 4 == 0, h <= 8192) or the bf16
    tile kernel (h % 8 == 0, h <= 8192, above 512 its column-pass variant; or h % 4 == 0, h <= 512, on
    8-byte row pieces, which nt_dmpnn_update_fused_dropout does not take)."""
    if dtype == torch.bfloat16:
        return ((h % 8 == 0 and 8 <= h <= 8192) or (h % 4 == 0 and 4 <= h <= 512)) and E < 2**31
    return (dtype == torch.float32 and h % 4 == 0 and 4 <= h <= 8192 and E * h // 4 < 2**31
            and V * h // 4 < 2**31 and E < 2**31 and V < 2**31)


PLAN_NCU = 256  # CUs the balanced tile plans are cut for (MI355X; host and device plans agree)
# slots the 64-row plans are balanced over.  Their kernels run two workgroups per CU, but balancing
# for 512 workgroups (~51-row tiles) measured slower than for the 256 CUs (~61 rows, whose tile count
# leaves some workgroups one tile short): config 2 layer 118-119 vs 107-110 us, config 3 233-235 vs
# 228 us, training 1.545 vs 1.478-1.495 ms (tools/r6_slots.sh, profiles/r6/slots_ab.txt)
PLAN_SLOTS64 = PLAN_NCU


def fused_tile_rows(h: int, dtype: torch.dtype, act: tuple[int, float] = (_lib.NT_ACT_RELU, 0.0),
                    reduce: str = "sum", agg_act: tuple[int, float] = (_lib.NT_ACT_RELU, 0.0)) -> int:
    """Row capacity of a nt_dmpnn_update_fused tile for this layer (128 or 64)."""
    code = NT_BF16 if dtype == torch.bfloat16 else NT_F32
    return int(_lib.load().nt_dmpnn_fused_tile_rows(h, code, act[0], reduce_code(reduce), agg_act[0]))


def tile_stride(E: int, max_in_degree: int, rows: int, ncu: int = PLAN_NCU) -> int:
    """Stride of the tile plan with tiles of at most `rows` rows, balanced over ncu CUs."""
    return int(_lib.load().nt_dmpnn_tile_stride(E, max_in_degree, rows, ncu))


def tile_plan(dst_ptr: Tensor, E: int, max_in_degree: int, rows: int = 64,
              ncu: int = 0, hub_degree: int = 0) -> tuple[Tensor, int, Tensor]:
    """(tile_ptr[ntiles+1], ntiles, dst_sorted[E]) for nt_dmpnn_update_fused: node-aligned tiles of
    at most `rows` rows (max_in_degree <= 32), balanced to whole rounds of ncu tiles (ncu = 0: the
    largest tiles; the engine's 128-row plans use PLAN_NCU).  hub_degree > 0: nodes with more
    in-edges are hubs, cut at the stride (nt_dmpnn_tile_plan_hubs; max_in_degree is then the largest
    non-hub in-degree).  The plan's largest tile is checked against `rows` here, where the plan is
    built (one device->host read per plan; the engine builds one per graph layout): the layer kernels
    clamp a larger tile and keep no status word, so a wrong max_in_degree must fail at this call."""
    dev = _require_device(dst_ptr)
    if dst_ptr.dtype != torch.int32:
        raise TypeError("dst_ptr must be int32")
    V = dst_ptr.numel() - 1
    lib = _lib.load()
    stride = tile_stride(E, max_in_degree, rows, ncu) if E > 0 else 1
    if E > 0 and stride <= 0:
        raise ValueError(f"max in-degree {max_in_degree} exceeds the tile rows {rows}")
    ntiles = int(lib.nt_dmpnn_tile_count(E, stride))
    tile_ptr = torch.empty(ntiles + 1, dtype=torch.int32, device=dev)
    dsts = torch.empty(max(E, 1), dtype=torch.int32, device=dev)[:E]
    if hub_degree > 0:
        _run(dev, lib.nt_dmpnn_tile_plan_hubs,
             _ptr(dst_ptr), V, E, stride, int(hub_degree), _ptr(tile_ptr), ntiles, _ptr(dsts), _stream(dev))
    else:
        _run(dev, lib.nt_dmpnn_tile_plan,
             _ptr(dst_ptr), V, E, stride, _ptr(tile_ptr), ntiles, _ptr(dsts), _stream(dev))
    if ntiles > 0:
        mx = int((tile_ptr[1:] - tile_ptr[:-1]).max())
        if mx > rows:
            raise ValueError(f"tile plan holds a tile of {mx} rows > {rows}: max_in_degree={max_in_degree} is "
                             "below the graph's largest (non-hub) in-degree")
    return tile_ptr, ntiles, dsts


def hub_runs(row_table: Tensor, dst_ptr: Tensor, dst_sorted: Tensor, tile_ptr: Tensor, hub_degree: int,
             run_rows: int) -> tuple[Tensor, int, Tensor, Tensor]:
    """A row table whose hub rows (nodes with more than hub_degree in-edges) are sub-runs for the fused
    layer's hub partials: runs of one hub's consecutive positions within a tile (tile_ptr), cut every
    run_rows rows (<= the launch's max_in_degree, so the kernel's segmented scan covers them), entry
    w = -((slot << 2) | start | end << 1) - 1.  Returns (table, nslots, hubs, slot_ptr) for
    dmpnn_update_fused(S_part=...) and hub_combine.  Device ops; one sync (the slot count)."""
    dev = _require_device(row_table, dst_ptr, dst_sorted, tile_ptr)
    E, V = row_table.shape[0], dst_ptr.numel() - 1
    run_rows = max(1, int(run_rows))
    dp = dst_ptr.long()
    deg = dp[1:] - dp[:-1]
    is_hub = deg > hub_degree
    d = dst_sorted.long()
    pos = torch.arange(E, device=dev)
    hub_row = is_hub[d]
    ts = torch.zeros(E + 1, dtype=torch.bool, device=dev)
    ts[tile_ptr.long()] = True
    run_start = hub_row & ((pos == dp[d]) | ts[:E])
    run_end = hub_row & ((pos + 1 == dp[d + 1]) | ts[1:])
    # offset of each row in its run (the run's start position by a running max), cut every run_rows
    rs = torch.cummax(torch.where(run_start, pos, torch.zeros_like(pos)), 0).values
    off = pos - rs
    sub_start = hub_row & (off % run_rows == 0)
    sub_end = hub_row & ((off % run_rows == run_rows - 1) | run_end)
    slot = torch.cumsum(sub_start.long(), 0) - 1
    hubs = torch.nonzero(is_hub).flatten()
    nslots = int(sub_start.sum()) if E else 0
    w = -(((slot << 2) | sub_start.long() | (sub_end.long() << 1))) - 1
    out = row_table.clone()
    out[:, 3] = torch.where(hub_row, w, row_table[:, 3].long()).to(torch.int32)
    # slot_ptr[v] = sub-runs starting before node v's first position (the hubs' slot CSR)
    before = torch.zeros(E + 1, dtype=torch.long, device=dev)
    torch.cumsum(sub_start.long(), 0, out=before[1:])
    slot_ptr = before[dp].to(torch.int32)
    return out, nslots, hubs.to(torch.int32), slot_ptr


def hub_combine(partial: Tensor, hubs: Tensor, slot_ptr: Tensor, seg_ptr: Tensor, out: Tensor, *,
                reduce: str = "sum", amax: Tensor | None = None) -> Tensor:
    """out[v] = reduce over the partial rows [slot_ptr[v], slot_ptr[v + 1]) for v in hubs
    (nt_dmpnn_hub_combine); out may be a row-padded view."""
    dev = _require_device(partial, hubs, slot_ptr, seg_ptr, out, amax)
    if partial.dtype != torch.float32 or out.dtype != torch.float32 or not partial.is_contiguous():
        raise TypeError("hub_combine: contiguous fp32 partial rows, fp32 out")
    V = seg_ptr.numel() - 1
    if slot_ptr.numel() != V + 1 or out.shape[0] != V:
        raise ValueError("slot_ptr must have V + 1 entries and out V rows")
    ld = _row_pitch("out", out)
    h = out.shape[1]
    _run(dev, _lib.load().nt_dmpnn_hub_combine, _ptr(partial), _ptr(hubs), _ptr(slot_ptr), hubs.numel(),
         _ptr(seg_ptr), V, h, reduce_code(reduce), NT_F32, _ptr(amax), _ptr(out), 0 if ld == h else ld, _stream(dev))
    return out


def mark_hub_rows(row_table: Tensor, dst_ptr: Tensor, hub_degree: int) -> Tensor:
    """In place: the row-table entries of nodes with more than hub_degree in-edges lose their
    "last in-edge" flag (nt_dmpnn_mark_hub_rows), so the fused layer leaves their S_out rows to
    hub_aggregate."""
    dev = _require_device(row_table, dst_ptr)
    if dst_ptr.dtype != torch.int32:
        raise TypeError("dst_ptr must be int32")
    _run(dev, _lib.load().nt_dmpnn_mark_hub_rows, _ptr(row_table), row_table.shape[0], _ptr(dst_ptr),
         dst_ptr.numel() - 1, int(hub_degree), _stream(dev))
    return row_table


def hub_aggregate(X: Tensor, perm: Tensor, seg_ptr: Tensor, hubs: Tensor, out: Tensor, *, reduce: str = "sum",
                  act: tuple[int, float] = (_lib.NT_ACT_IDENTITY, 0.0), amax: Tensor | None = None) -> Tensor:
    """out[v] = reduce over the in-edges p of v of act(X[perm[p]]) for the nodes v in ``hubs`` (int32),
    other rows of ``out`` untouched; amax (1 float, may be None) raised to max|out[hubs]|.  X and out
    may be row-padded views of one common pitch."""
    dev = _require_device(X, perm, seg_ptr, hubs, out, amax)
    if X.dtype != torch.float32 or out.dtype != torch.float32:
        raise TypeError("hub_aggregate is fp32 only")
    ld = _row_pitch("X", X)
    if _row_pitch("out", out) != ld:
        raise ValueError("X and out must share one row pitch")
    if hubs.dtype != torch.int32 or seg_ptr.dtype != torch.int32 or perm.dtype != torch.int32:
        raise TypeError("hubs, seg_ptr and perm must be int32")
    if out.shape[1] != X.shape[1] or out.shape[0] != seg_ptr.numel() - 1:
        raise ValueError("out must be nseg x h")
    _run(dev, _lib.load().nt_dmpnn_hub_aggregate, _ptr(X), _ptr(perm), _ptr(seg_ptr), _ptr(hubs), hubs.numel(),
         X.shape[1], reduce_code(reduce), act[0], act[1], NT_F32, _ptr(amax), _ptr(out),
         0 if ld == X.shape[1] else ld, _stream(dev))
    return out


def dmpnn_update_fused(
    H: Tensor,
    S: Tensor,
    src: Tensor,
    rev: Tensor,
    Wp: Tensor,
    bias: Tensor | None,
    *,
    residual: bool = True,
    act: tuple[int, float] = (_lib.NT_ACT_RELU, 0.0),
    plan: tuple[Tensor, int, Tensor] | None = None,
    tile_rows: int = 64,
    max_in_degree: int = 32,
    perm: Tensor | None = None,
    reduce: str = "sum",
    agg_act: tuple[int, float] = (_lib.NT_ACT_RELU, 0.0),
    zero_fill: bool = False,
    amax_in: Tensor | None = None,
    amax_out: Tensor | None = None,
    row_table: Tensor | None = None,
    out: Tensor | None = None,
    S_out: Tensor | None = None,
    pitch_out: int | None = None,
    S_part: Tensor | None = None,
    n_nodes: int | None = None,
    dropout: tuple[float, int, int] | None = None,
) -> tuple[Tensor, Tensor | None]:
    """H_out = (residual ? H : 0) + (S[src] - act(H[rev])) @ W^T + b and, with a tile plan (tiles of at
    most ``tile_rows`` rows), S_out = scatter(agg_act(H_out), dst, reduce) in the same persistent launch.

    ``dropout`` = (p, seed, offset) (with a plan only; nt_dmpnn_update_fused_dropout): the update passes
    the mask of dropout_residual(p, seed, offset) before the residual is added,
    H_out = (residual ? H : 0) + keep * ((S[src] - act(H[rev])) @ W^T + b) / (1 - p), in the layer
    kernel's epilogue; S_out and amax_out are those of the values after dropout.  bf16: plans of at
    most 64 rows.

    fp32: H and S may be row-padded views with one common pitch (see dmpnn_init's ``pitch``); H_out /
    S_out are allocated with rows ``pitch_out`` floats apart (default: dense), or given with one pitch.

    fp32: ``amax_in`` = (max|H|, max|S|) on the device (computed here with nt_absmax when not given);
    ``amax_out`` (2 zero-filled floats) receives max|H_out|, max|S_out| for the next layer.
    ``row_table`` (with a plan): nt_dmpnn_row_table of (perm, dst_sorted, src, rev), built here
    when not given (cache it per graph).
    ``zero_fill`` must be True when some node has no in-edge (its S_out row is then 0).
    ``S_part`` (fp32, slots x h): the hub partial rows when the row table marks hub sub-runs
    (hub_runs); hub_combine then finishes the hubs' S_out rows.
    ``n_nodes``: the aggregation's segment count, i.e. the rows S_out must hold (default: S's rows;
    the backward's fused dA passes S = G with E rows and S_out with the graph's V)."""
    dev = _require_device(H, S, src, rev, Wp, bias, out, S_out, perm, amax_in, amax_out)
    if dropout is not None:
        p, seed, offset = float(dropout[0]), int(dropout[1]), int(dropout[2])
        if not 0.0 <= p <= 1.0:
            raise ValueError("dropout probability must be in [0, 1]")
        if offset < 0:
            raise ValueError("dropout offset must be >= 0")
        if plan is None:
            raise ValueError("dropout in the layer kernel needs a tile plan")
        if H.dtype == torch.bfloat16 and tile_rows > 64:
            raise ValueError("bf16 dropout in the layer kernel takes plans of at most 64 rows")
    ld_in = _row_pitch("H", H)
    code = _DTYPE_CODES[H.dtype]
    if _row_pitch("S", S, H.dtype) != ld_in:
        raise ValueError("H and S must share one row pitch")
    _require_i64("src", src)
    _require_i64("rev_index", rev)
    _require_amax(amax_in, H.dtype)
    _require_amax(amax_out, H.dtype)
    E, h = H.shape
    V = S.shape[0]
    if S.shape[1] != h or src.numel() != E or rev.numel() != E:
        raise ValueError("shape mismatch between H, S, src and rev_index")
    if Wp.numel() != packed_weight_numel(h, H.dtype):
        raise ValueError(f"Wp is not a packed {H.dtype} weight image for this hidden size")
    if bias is not None:
        _require_feat("bias", bias, H.dtype)
        if bias.numel() != h:
            raise ValueError("bias must have h entries")
    if out is None:
        out = padded_rows(E, h, h if pitch_out is None else int(pitch_out), H.dtype, dev)
    ld_out = _row_pitch("out", out, H.dtype)
    tile_ptr = dsts = None
    ntiles = 0
    if plan is not None:
        tile_ptr, ntiles, dsts = plan
        if perm is None or perm.dtype != torch.int32 or perm.numel() != E:
            raise ValueError("fused aggregation needs the int32 dst CSR permutation")
        if dsts is None or dsts.dtype != torch.int32 or dsts.numel() != E:
            raise ValueError("the plan's dst_sorted must be int32 with E entries")
        n_out = V if n_nodes is None else int(n_nodes)
        if S_part is not None and (S_part.dtype != torch.float32 or not S_part.is_contiguous()
                                   or S_part.dim() != 2 or S_part.shape[1] != h or S_part.shape[0] < 1):
            raise ValueError("S_part must be a contiguous fp32 (slots x h) tensor")
        if S_out is None:
            S_out = padded_rows(n_out, h, ld_out, H.dtype, dev)
            if zero_fill:
                S_out.zero_()
        else:
            if _row_pitch("S_out", S_out, H.dtype) != ld_out:
                raise ValueError("out and S_out must share one row pitch")
            if S_out.shape[0] < n_out or S_out.shape[1] != h:
                raise ValueError(f"S_out must hold n_nodes={n_out} rows of h={h}")
            if zero_fill:
                S_out.zero_()
    else:
        perm = None
        S_out = None
        if S_part is not None:
            raise ValueError("S_part needs a tile plan")
    if plan is not None and row_table is None and E > 0:
        row_table = dmpnn_row_table(perm, dsts, src, rev, V)
    if H.dtype == torch.float32 and amax_in is None and E > 0:
        amax_in = torch.zeros(2, dtype=torch.float32, device=dev)
        absmax(H.contiguous(), amax_in[0:1])
        absmax(S.contiguous(), amax_in[1:2])
    lib = _lib.load()
    args = (_ptr(H), _ptr(S), _ptr(src), _ptr(rev), _ptr(Wp), _ptr(bias), V, E, h, int(residual),
            act[0], act[1], _ptr(tile_ptr), ntiles, int(tile_rows), int(max_in_degree), _ptr(perm), _ptr(dsts),
            _ptr(row_table), reduce_code(reduce), agg_act[0], agg_act[1], code, _ptr(amax_in), _ptr(amax_out),
            _ptr(out), _ptr(S_out), _ptr(S_part), 0 if ld_in == h else ld_in, 0 if ld_out == h else ld_out)
    if dropout is not None:
        _run(dev, lib.nt_dmpnn_update_fused_dropout, *args, p, seed & (2**64 - 1), offset, _stream(dev))
    else:
        _run(dev, lib.nt_dmpnn_update_fused, *args, _stream(dev))
    return out, S_out


def dmpnn_row_table(perm: Tensor, dst_sorted: Tensor, src: Tensor, rev: Tensor, V: int) -> Tensor:
    """E x 4 int32: {edge, src, rev, (node << 2) | start | end << 1} per dst-sorted position (the fp32
    layer kernel's one-load view of a fused plan's rows)."""
    dev = _require_device(perm, dst_sorted, src, rev)
    _require_i64("src", src)
    _require_i64("rev_index", rev)
    E = perm.numel()
    out = torch.empty(max(E, 1), 4, dtype=torch.int32, device=dev)[:E]
    _run(dev, _lib.load().nt_dmpnn_row_table, _ptr(perm), _ptr(dst_sorted), _ptr(src), _ptr(rev), V, E, _ptr(out),
         _stream(dev))
    return out


def dense_matmul(X: Tensor, Wp: Tensor, out: Tensor | None = None, *, kernel: str = "fk",
                 amax: Tensor | None = None) -> Tensor:
    """X @ W^T for the packed image Wp of W: the layer GEMM alone.  With Wp = pack_weights(W.t()) it is
    the backward's dA = G @ W.  fp32 (h % 4 == 0, any h <= 8192): the fp16x3 layer kernel in dense
    mode.  kernel picks how it gets its split scale: "fk" passes amax_in (amax: 2 device floats whose
    [1] >= max|X|, else nt_absmax first); "pk" (the name of a kernel that no longer exists) passes no
    amax_in, so the entry point measures max|X| itself into a workspace allocated here.  bf16
    (h <= 512, or h % 8 == 0 up to 8192): the bf16 layer kernel
    without gathers (fp32 accumulate, one rounding)."""
    dev = _require_device(X, Wp, out, amax)
    code = _require_feat("X", X)
    M, h = X.shape
    if Wp.numel() != packed_weight_numel(h, X.dtype):
        raise ValueError(f"Wp is not a packed {X.dtype} weight image for this hidden size")
    if out is None:
        out = torch.empty_like(X)
    if code == NT_BF16:
        if h > 512 and (h % 8 or h > 8192):
            raise ValueError("dense_matmul: bf16 needs h <= 512, or h % 8 == 0 and h <= 8192")
        _run(dev, _lib.load().nt_dmpnn_dense_matmul, _ptr(X), M, h, _ptr(Wp), NT_BF16, None, None, _ptr(out),
             _stream(dev))
        return out
    if kernel == "fk":
        if amax is None:
            amax = torch.zeros(2, dtype=torch.float32, device=dev)
            absmax(X, amax[1:2])
        else:
            _require_amax(amax, X.dtype)
    elif kernel != "pk":
        raise ValueError("kernel must be 'fk' or 'pk'")
    # kernel = "pk" passes no amax: the entry point writes max|X| into this caller-owned workspace (ABI 6)
    ws = torch.empty(2, dtype=torch.float32, device=dev) if amax is None else None
    _run(dev, _lib.load().nt_dmpnn_dense_matmul, _ptr(X), M, h, _ptr(Wp), NT_F32, _ptr(amax), _ptr(ws), _ptr(out),
         _stream(dev))
    return out


def weight_grad(G: Tensor, H: Tensor | None, S: Tensor, src: Tensor | None, rev: Tensor | None, *,
                act: tuple[int, float] = (_lib.NT_ACT_RELU, 0.0), bias: bool = True,
                amax_G: Tensor | None = None, amax_HS: Tensor | None = None) -> tuple[Tensor, Tensor | None]:
    """(dW, db) = (G^T A, sum_e G[e]) with A[e] = S[src e] - act(H[rev e]) formed on the fly
    (src = rev = None: A = S).  Split-K, deterministic.  fp32: with amax_G (1 device float >= max|G|)
    and amax_HS (2 floats >= max|H|, max|S|), src / rev given, and h <= 320 or h % 4 == 0 up to 8192
    with 16-byte aligned G, H and S (above 320 on the kernel that tiles dW in both dimensions), the
    two-part fp16 kernel (nt_dmpnn_weight_grad_fk); every other call the bf16x6 kernel.  bf16 (src /
    rev given; an even h <= 512, or h % 8 == 0 up to 8192 on the kernel that tiles dW in both
    dimensions): A rounded to bf16 as the forward's message, one bf16 MFMA per tile; dW and db come
    back in fp32."""
    dev = _require_device(G, H, S, src, rev, amax_G, amax_HS)
    code = _require_feat("G", G)
    _require_feat("S", S, G.dtype)
    if code == NT_BF16:
        hb = G.shape[1]
        if src is None or not ((hb <= 512 and hb % 2 == 0) or (hb % 8 == 0 and hb <= 8192)):
            raise ValueError("weight_grad: bf16 needs src / rev_index, and an even h <= 512 or h % 8 == 0 "
                             "and h <= 8192")
    E, h = G.shape
    if (src is None) != (rev is None):
        raise ValueError("weight_grad: pass both src and rev_index or neither")
    if src is not None:
        assert H is not None
        _require_feat("H", H, G.dtype)
        _require_i64("src", src)
        _require_i64("rev_index", rev)
        if H.shape != (E, h) or S.shape[1] != h or src.numel() != E or rev.numel() != E:
            raise ValueError("shape mismatch between G, H, S, src and rev_index")
    elif S.shape != (E, h):
        raise ValueError("weight_grad: S must be E x h when src is None")
    for n_, t in (("G", G), ("H", H), ("S", S)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"weight_grad: {n_} must be contiguous")
    if E == 0 and code == NT_BF16:
        # empty sums; empty index tensors have no address to hand to the entry point, which asks
        # bf16 callers for src and rev before it looks at E
        return (torch.zeros(h, h, dtype=torch.float32, device=dev),
                torch.zeros(h, dtype=torch.float32, device=dev) if bias else None)
    lib = _lib.load()
    # the workspace is sized by the plan of the launch device (its CU count): query under its guard
    if dev.index is not None and dev.index != torch.cuda.current_device():
        with torch.cuda.device(dev):
            nbytes = lib.nt_dmpnn_weight_grad_workspace(E, h)
    else:
        nbytes = lib.nt_dmpnn_weight_grad_workspace(E, h)
    if nbytes < 0:
        raise ValueError(f"weight_grad: bad sizes E={E} h={h}")
    ws = torch.empty((max(nbytes, 4) + 3) // 4, dtype=torch.float32, device=dev)
    dW = torch.empty(h, h, dtype=torch.float32, device=dev)
    db = torch.empty(h, dtype=torch.float32, device=dev) if bias else None
    fk = code == NT_F32 and amax_G is not None and amax_HS is not None and src is not None
    if fk and h > 320:  # the kernel that tiles dW in both dimensions: 16-B row pieces
        fk = h % 4 == 0 and h <= 8192 and all(t.data_ptr() % 16 == 0 for t in (G, H, S))
    if fk:
        _require_amax(amax_G, G.dtype, n=1)
        _require_amax(amax_HS, G.dtype)
        _run(dev, lib.nt_dmpnn_weight_grad_fk, _ptr(G), _ptr(H), _ptr(S), _ptr(src), _ptr(rev), S.shape[0], E,
             h, act[0], act[1], _ptr(amax_G), _ptr(amax_HS), NT_F32, _ptr(ws), ws.numel() * 4, _ptr(dW), _ptr(db),
             _stream(dev))
        return dW, db
    _run(dev, lib.nt_dmpnn_weight_grad, _ptr(G), _ptr(H), _ptr(S), _ptr(src), _ptr(rev), S.shape[0], E, h,
         act[0], act[1], code, _ptr(ws), ws.numel() * 4, _ptr(dW), _ptr(db), _stream(dev))
    return dW, db


def segment_arg(X: Tensor, seg_ptr: Tensor, perm: Tensor | None, nseg: int, reduce: str, *,
                act: tuple[int, float] = (_lib.NT_ACT_IDENTITY, 0.0)) -> Tensor:
    """int32 (nseg x h): the first row (ascending CSR order) of each segment holding the max / min
    of act(X) per column, -1 for empty segments (torch_scatter scatter_max / scatter_min's arg).
    fp32 or bf16 X."""
    dev = _require_device(X, seg_ptr, perm)
    code = _require_feat("X", X)
    if reduce not in ("max", "min"):
        raise ValueError("segment_arg: reduce must be 'max' or 'min'")
    h = X.shape[1]
    arg = torch.empty(nseg, h, dtype=torch.int32, device=dev)
    if X.shape[0] == 0:  # no rows: every segment is empty
        return arg.fill_(-1)
    _run(dev, _lib.load().nt_segment_arg, _ptr(X), _ptr(seg_ptr), _ptr(perm), nseg, h, reduce_code(reduce),
         act[0], act[1], code, _ptr(arg), _stream(dev))
    return arg


def dmpnn_edge_backward_arg(G: Tensor | None, H: Tensor, dA: Tensor, dS: Tensor, arg: Tensor, dst: Tensor,
                            rev_ptr: Tensor, rev_perm: Tensor, *, residual: bool = True,
                            act: tuple[int, float] = (_lib.NT_ACT_RELU, 0.0), amax: Tensor | None = None) -> Tensor:
    """dL/dH_l for a max / min aggregation (arg = segment_arg of act(H_l) over the dst CSR); amax (1
    zero-filled device float, optional, fp32 only) is raised to max|out|.  fp32 or bf16 storage."""
    dev = _require_device(G, H, dA, dS, arg, dst, rev_ptr, rev_perm, amax)
    code = _require_feat("H", H)
    for n_, t in (("dA", dA), ("dS", dS)) + ((("G", G),) if G is not None else ()):
        _require_feat(n_, t, H.dtype)
    if amax is not None and code != NT_F32:
        raise ValueError("amax is fp32 only")
    E, h = H.shape
    V = dS.shape[0]
    out = torch.empty_like(H)
    _run(dev, _lib.load().nt_dmpnn_edge_backward_arg, _ptr(G), _ptr(H), _ptr(dA), _ptr(dS), _ptr(arg),
         _ptr(dst), _ptr(rev_ptr), _ptr(rev_perm), V, E, h, int(residual), act[0], act[1], code,
         _ptr(out), _ptr(amax), _stream(dev))
    return out


def gather_rows_arg(X: Tensor, idx: Tensor, arg: Tensor, *, base: Tensor | None = None,
                    amax: Tensor | None = None) -> Tensor:
    """out[i] = base[i] + (arg[idx i] == i ? X[idx i] : 0) (max / min scatter backward); amax as
    dmpnn_edge_backward_arg.  fp32 or bf16."""
    dev = _require_device(X, idx, arg, base, amax)
    code = _require_feat("X", X)
    if base is not None:
        _require_feat("base", base, X.dtype)
    if amax is not None and code != NT_F32:
        raise ValueError("amax is fp32 only")
    n, h = idx.numel(), X.shape[1]
    out = torch.empty(n, h, dtype=X.dtype, device=dev)
    _run(dev, _lib.load().nt_gather_rows_arg, _ptr(base), _ptr(X), _ptr(idx), _ptr(arg), n, h, code,
         _ptr(out), _ptr(amax), _stream(dev))
    return out


# ------------------------------------------------------------------------------------ backward
def dmpnn_message(H: Tensor, S: Tensor, src: Tensor, rev: Tensor, *,
                  act: tuple[int, float] = (_lib.NT_ACT_RELU, 0.0), out: Tensor | None = None) -> Tensor:
    """A = S[src] - act(H[rev])  (the layer message, recomputed for the weight gradient)."""
    dev = _require_device(H, S, src, rev, out)
    code = _require_feat("H", H)
    _require_feat("S", S, H.dtype)
    _require_i64("src", src)
    _require_i64("rev_index", rev)
    E, h = H.shape
    V = S.shape[0]
    if S.shape[1] != h or src.numel() != E or rev.numel() != E:
        raise ValueError("shape mismatch between H, S, src and rev_index")
    if out is None:
        out = torch.empty_like(H)
    else:
        _require_feat("out", out, H.dtype)
    _run(dev, _lib.load().nt_dmpnn_message,
         _ptr(H), _ptr(S), _ptr(src), _ptr(rev), V, E, h, act[0], act[1], code, _ptr(out), _stream(dev))
    return out


def dmpnn_edge_backward(G: Tensor | None, H: Tensor, dA: Tensor, dS: Tensor, dst: Tensor,
                        rev_ptr: Tensor, rev_perm: Tensor, dst_ptr: Tensor | None, *,
                        residual: bool = True, act: tuple[int, float] = (_lib.NT_ACT_RELU, 0.0),
                        reduce: str = "sum", out: Tensor | None = None, amax: Tensor | None = None) -> Tensor:
    """dL/dH_l = (residual ? G : 0) + act'(H) * (dS[dst] / c - scatter(dA, rev))  (see header); fp32:
    amax (1 zero-filled device float, optional) is raised to max|out|."""
    dev = _require_device(G, H, dA, dS, dst, rev_ptr, rev_perm, dst_ptr, out, amax)
    code = _require_feat("H", H)
    for name, t in (("dA", dA), ("dS", dS)):
        _require_feat(name, t, H.dtype)
    if residual:
        if G is None:
            raise ValueError("residual backward needs G")
        _require_feat("G", G, H.dtype)
    _require_i64("dst", dst)
    E, h = H.shape
    V = dS.shape[0]
    if dA.shape != H.shape or dS.shape[1] != h or dst.numel() != E or rev_ptr.numel() != E + 1:
        raise ValueError("shape mismatch in dmpnn_edge_backward")
    if reduce == "mean" and dst_ptr is None:
        raise ValueError("mean reduce needs the dst CSR")
    if out is None:
        out = torch.empty_like(H)
    else:
        _require_feat("out", out, H.dtype)
    _run(dev, _lib.load().nt_dmpnn_edge_backward,
         _ptr(G if residual else None), _ptr(H), _ptr(dA), _ptr(dS), _ptr(dst), _ptr(rev_ptr),
         _ptr(rev_perm), _ptr(dst_ptr), V, E, h, int(residual), act[0], act[1], reduce_code(reduce),
         code, _ptr(out), _ptr(amax), _stream(dev))
    return out


def gather_rows(X: Tensor, idx: Tensor, *, base: Tensor | None = None, seg_ptr: Tensor | None = None,
                out: Tensor | None = None, amax: Tensor | None = None) -> Tensor:
    """out[i] = (base[i] if base is given) + X[idx[i]], divided by max(segment size of idx[i], 1)
    when ``seg_ptr`` is given (the backward of a mean scatter); fp32: amax as dmpnn_edge_backward."""
    dev = _require_device(X, idx, base, seg_ptr, out, amax)
    code = _require_feat("X", X)
    _require_i64("idx", idx)
    nseg, h = X.shape
    n = idx.numel()
    if base is not None:
        _require_feat("base", base, X.dtype)
        if base.shape != (n, h):
            raise ValueError("base must be n x h")
    if seg_ptr is not None and (seg_ptr.dtype != torch.int32 or seg_ptr.numel() != nseg + 1):
        raise ValueError("seg_ptr must be int32 of length nseg + 1")
    if out is None:
        out = torch.empty(n, h, dtype=X.dtype, device=dev)
    else:
        _require_feat("out", out, X.dtype)
    _run(dev, _lib.load().nt_gather_rows,
         _ptr(base), _ptr(X), _ptr(idx), _ptr(seg_ptr), n, nseg, h, code, _ptr(out), _ptr(amax), _stream(dev))
    return out


# ------------------------------------------------------------------------------------ embedding
def _check_types(name: str, idx: Tensor, num_types: int) -> None:
    _require_i64(name, idx)
    if idx.dim() != 2:
        raise ValueError(f"{name} must be n x k type indices")
    if idx.numel():
        mm = torch.stack([idx.min(), idx.max()]).cpu()
        if mm[0] < 0 or mm[1] >= num_types:
            raise IndexError(f"{name}: type index out of range for an embedding of {num_types} rows")


def embed_bag(table: Tensor, idx: Tensor, *, validate: bool = True, out: Tensor | None = None) -> Tensor:
    """nn.EmbeddingBag(mode="sum") of an n x k index matrix: out[i] = sum_j table[idx[i, j]]."""
    dev = _require_device(table, idx, out)
    code = _require_feat("table", table)
    ntypes, h = table.shape
    if validate:
        _check_types("idx", idx, ntypes)
    else:
        _require_i64("idx", idx)
    n, k = idx.shape
    if out is None:
        out = torch.empty(n, h, dtype=table.dtype, device=dev)
    _run(dev, _lib.load().nt_embed_bag,
         _ptr(table), ntypes, _ptr(idx), n, k, h, code, _ptr(out), _stream(dev))
    return out


def dmpnn_init_embed(
    node_table: Tensor,
    node_types: Tensor,
    edge_table: Tensor,
    edge_types: Tensor,
    src: Tensor,
    seg_ptr: Tensor | None = None,
    perm: Tensor | None = None,
    *,
    act: tuple[int, float] = (_lib.NT_ACT_RELU, 0.0),
    reduce: str = "sum",
    validate: bool = True,
    amax: Tensor | None = None,
    pitch: int | None = None,
    records: Tensor | None = None,
) -> tuple[Tensor, Tensor | None]:
    """H0 = Xv[src] + Xe with Xv = EmbeddingBag(node_table)(node_types), Xe likewise, never
    materialised; optionally fused with S = scatter(act(H0), dst) (needs the dst CSR).
    amax (fp32, 2 zero-filled device floats): raised to max|H0|, max|S|.
    records: embed_edge_records of this graph (fp32 with S, 7 + 2 type columns): the wave-per-node
    init over them (same bits)."""
    dev = _require_device(node_table, node_types, edge_table, edge_types, src, seg_ptr, perm, amax, records)
    _require_amax(amax, node_table.dtype)
    code = _require_feat("node_table", node_table)
    _require_feat("edge_table", edge_table, node_table.dtype)
    if node_table.shape[1] != edge_table.shape[1]:
        raise RuntimeError("node and edge embedding tables must share the hidden dimension")
    if validate:
        _check_types("node_types", node_types, node_table.shape[0])
        _check_types("edge_types", edge_types, edge_table.shape[0])
    _require_i64("src", src)
    V, kv = node_types.shape
    E, ke = edge_types.shape
    h = node_table.shape[1]
    if src.numel() != E:
        raise ValueError("src must have one entry per edge")
    if records is not None and (records.dtype != torch.int32 or records.shape != (E, 4) or not records.is_contiguous()):
        raise ValueError("records must be the (E, 4) int32 embed_edge_records of this graph")
    ld = h if pitch is None else int(pitch)  # row-padded H0 / S views (as dmpnn_init's pitch)
    H0 = padded_rows(E, h, ld, node_table.dtype, dev)
    S = None if seg_ptr is None else padded_rows(V, h, ld, node_table.dtype, dev)
    _run(dev, _lib.load().nt_dmpnn_init_embed,
         _ptr(node_table), node_table.shape[0], _ptr(node_types), kv, _ptr(edge_table),
         edge_table.shape[0], _ptr(edge_types), ke, _ptr(src), _ptr(seg_ptr), _ptr(perm), V, E, h,
         act[0], act[1], reduce_code(reduce), code, _ptr(H0), _ptr(S), _ptr(amax), 0 if ld == h else ld,
         _ptr(records), _stream(dev))
    return H0, S


def embed_edge_records(node_types: Tensor, num_node_types: int, edge_types: Tensor, num_edge_types: int,
                       src: Tensor, perm: Tensor) -> Tensor:
    """(E, 4) int32 type records of a graph for dmpnn_init_embed (nt_embed_edge_records): per position of
    the dst CSR permutation, the in-edge and its 7 node-type and 2 edge-type indices as bytes (255 =
    out of range).  Build once per graph."""
    dev = _require_device(node_types, edge_types, src, perm)
    _require_i64("node_types", node_types)
    _require_i64("edge_types", edge_types)
    _require_i64("src", src)
    if node_types.dim() != 2 or node_types.shape[1] != 7 or edge_types.dim() != 2 or edge_types.shape[1] != 2:
        raise ValueError("type records need 7 node-type and 2 edge-type columns")
    V, E = node_types.shape[0], edge_types.shape[0]
    if perm.dtype != torch.int32 or perm.numel() != E or src.numel() != E:
        raise ValueError("perm (int32) and src need one entry per edge")
    out = torch.empty(max(E, 1), 4, dtype=torch.int32, device=dev)[:E]
    _run(dev, _lib.load().nt_embed_edge_records, _ptr(node_types.contiguous()), int(num_node_types),
         _ptr(edge_types.contiguous()), int(num_edge_types), _ptr(src), _ptr(perm), V, E, _ptr(out), _stream(dev))
    return out


def embed_bag_backward(dX: Tensor, idx: Tensor, ntypes: int, seg_ptr: Tensor | None = None,
                       perm: Tensor | None = None, pitch: int | None = None,
                       out_dtype: torch.dtype | None = None) -> Tensor:
    """Table gradient of a sum-mode EmbeddingBag (nt_embed_bag_backward): dT[t] = sum of R[i] over every
    (i, j) with idx[i, j] == t, accumulated in fp32 and rounded once to out_dtype (default dX's).
    R[i] = dX[i], or with the CSR (seg_ptr int32[n + 1], perm int32 over dX's rows, from csr_build)
    R[i] = sum of dX[perm[p]] over segment i.  dX: fp32 or bf16 rows, contiguous or a row-padded view
    (pitch: its row pitch in elements when it is not the tensor's own stride).  A type no index names
    gets a zero row; indices outside [0, ntypes) contribute nothing (the forward validates them).
    Deterministic: per-workgroup LDS partial tables combined in a fixed order, no float atomics; tables
    past the LDS partial are taken in chunks of type rows by the same kernel."""
    dev = _require_device(dX, idx, seg_ptr, perm)
    if dX.dim() != 2:
        raise ValueError("dX must be 2-D")
    if dX.dtype not in _DTYPE_CODES:
        raise TypeError(f"dX must be float32 or bfloat16, got {dX.dtype}")
    n_dx, h = dX.shape
    if pitch is None:
        if dX.is_contiguous():
            pitch = h
        elif dX.stride(1) == 1 and dX.stride(0) >= h:
            pitch = dX.stride(0)
        else:
            raise ValueError("dX must be contiguous or a row-padded view (unit column stride)")
    pitch = int(pitch)
    if pitch < h or (n_dx > 1 and dX.stride(0) != pitch) or (n_dx > 0 and h > 1 and dX.stride(1) != 1):
        raise ValueError("pitch must be dX's row stride (>= h)")
    _require_i64("idx", idx)
    if idx.dim() != 2:
        raise ValueError("idx must be n x k type indices")
    n, k = idx.shape
    if ntypes < 0 or h <= 0:
        raise ValueError("ntypes must be >= 0 and h > 0")
    if (seg_ptr is None) != (perm is None):
        raise ValueError("the CSR needs both seg_ptr and perm")
    if seg_ptr is None:
        if n_dx != n:
            raise ValueError("without a CSR dX needs one row per row of idx")
    else:
        if seg_ptr.dtype != torch.int32 or seg_ptr.numel() != n + 1 or not seg_ptr.is_contiguous():
            raise ValueError("seg_ptr must be contiguous int32 of length n + 1")
        if perm.dtype != torch.int32 or perm.numel() != n_dx or not perm.is_contiguous():
            raise ValueError("perm must be contiguous int32 with one entry per row of dX")
    out_dtype = dX.dtype if out_dtype is None else out_dtype
    if out_dtype not in _DTYPE_CODES:
        raise TypeError(f"out_dtype must be float32 or bfloat16, got {out_dtype}")
    out = torch.empty(ntypes, h, dtype=out_dtype, device=dev)
    if ntypes == 0:
        return out
    lib = _lib.load()
    ws_bytes = lib.nt_embed_bag_backward_workspace(n, ntypes, h)
    if ws_bytes < 0:
        raise ValueError("bad sizes for embed_bag_backward")
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
    _run(dev, lib.nt_embed_bag_backward,
         _ptr(dX), pitch, n_dx, _ptr(idx), n, k, int(ntypes), h, _ptr(seg_ptr), _ptr(perm),
         _DTYPE_CODES[dX.dtype], _DTYPE_CODES[out_dtype], _ptr(out), _ptr(ws), ws_bytes, _stream(dev))
    return out


# ------------------------------------------------------------------------------------ attention readouts
def node_scores(X: Tensor, *, a: Tensor | None = None, a_bias: Tensor | None = None,
                Q: Tensor | None = None, node_seg: Tensor | None = None,
                sqrt_key: float = 1.0) -> Tensor:
    """Per-node readout scores (fp32): X @ a + a_bias (Gated) or (Q[node_seg] * X).sum(1) / sqrt_key
    (SDPAttention)."""
    dev = _require_device(X, a, a_bias, Q, node_seg)
    code = _require_feat("X", X)
    n, h = X.shape
    if (a is None) == (Q is None):
        raise ValueError("pass exactly one of a (Gated) and Q (SDPAttention)")
    if a is not None:
        _require_feat("a", a, X.dtype)
        if a.numel() != h:
            raise ValueError("a must have h entries")
        if a_bias is not None:
            _require_feat("a_bias", a_bias, X.dtype)
    else:
        _require_feat("Q", Q, X.dtype)
        if Q.dim() != 2 or Q.shape[1] != h:
            raise RuntimeError(f"Q must be b x {h}, got {tuple(Q.shape)}")
        if node_seg is None:
            raise ValueError("SDPAttention scores need batch_node_index")
        _require_i64("batch_node_index", node_seg)
    s = torch.empty(n, dtype=torch.float32, device=dev)
    _run(dev, _lib.load().nt_node_scores,
         _ptr(X), n, h, _ptr(a), _ptr(a_bias), _ptr(Q), _ptr(node_seg), float(sqrt_key), code,
         _ptr(s), _stream(dev))
    return s


def softmax_pool(X: Tensor, scores: Tensor, seg_ptr: Tensor, perm: Tensor | None, nseg: int) -> Tensor:
    """out[g] = sum over v in segment g of softmax_g(scores)[v] * X[v]."""
    dev = _require_device(X, scores, seg_ptr, perm)
    code = _require_feat("X", X)
    if scores.dtype != torch.float32 or scores.numel() != X.shape[0]:
        raise ValueError("scores must be fp32 with one entry per row of X")
    if seg_ptr.dtype != torch.int32 or seg_ptr.numel() != nseg + 1:
        raise ValueError("seg_ptr must be int32 of length nseg + 1")
    h = X.shape[1]
    out = torch.empty(nseg, h, dtype=X.dtype, device=dev)
    _run(dev, _lib.load().nt_softmax_pool,
         _ptr(X), _ptr(scores), _ptr(seg_ptr), _ptr(perm), nseg, h, code, _ptr(out), _stream(dev))
    return out


def softmax_pool_backward(X: Tensor, scores: Tensor, seg_ptr: Tensor, perm: Tensor | None, node_seg: Tensor,
                          nseg: int, out: Tensor, dout: Tensor, *, a: Tensor | None = None,
                          Q: Tensor | None = None, sqrt_key: float = 1.0) -> tuple[Tensor, Tensor, Tensor]:
    """Backward of node_scores + softmax_pool for dout (nseg x h): (dX, ds, P) with ds the fp32 score
    gradient and P[g] = sum_{v in g} ds[v] X[v] (fp32): Gated da = P.sum(0), db = ds.sum(); SDPA
    dQ = P / sqrt_key (nt_softmax_pool_backward)."""
    dev = _require_device(X, scores, seg_ptr, perm, node_seg, out, dout, a, Q)
    code = _require_feat("X", X)
    _require_feat("out", out, X.dtype)
    _require_feat("dout", dout, X.dtype)
    if (a is None) == (Q is None):
        raise ValueError("pass exactly one of a (Gated) and Q (SDPAttention)")
    _require_feat("a" if a is not None else "Q", a if a is not None else Q, X.dtype)
    _require_i64("batch_node_index", node_seg)
    if scores.dtype != torch.float32 or scores.numel() != X.shape[0]:
        raise ValueError("scores must be fp32 with one entry per row of X")
    n, h = X.shape
    dX = torch.empty_like(X)
    ds = torch.empty(n, dtype=torch.float32, device=dev)
    P = torch.empty(nseg, h, dtype=torch.float32, device=dev)
    stats = torch.empty(max(3 * nseg, 1), dtype=torch.float32, device=dev)
    _run(dev, _lib.load().nt_softmax_pool_backward,
         _ptr(X), _ptr(scores), _ptr(seg_ptr), _ptr(perm), _ptr(node_seg), nseg, n, h, _ptr(out), _ptr(dout),
         _ptr(a), _ptr(Q), float(sqrt_key), code, _ptr(stats), _ptr(dX), _ptr(ds), _ptr(P), _stream(dev))
    return dX, ds, P


def _require_f32_key(name: str, t: Tensor) -> None:
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 on the mixed readout path, got {t.dtype} "
                        "(operands of one dtype take node_scores / softmax_pool_backward)")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _require_mixed_readout(X: Tensor, a: Tensor | None, a_bias: Tensor | None, Q: Tensor | None,
                           node_seg: Tensor | None) -> None:
    """bf16 X (n x h, contiguous) with exactly one fp32 key: a (h entries, with an optional fp32 a_bias of
    one entry) or Q (b x h, with batch_node_index)."""
    if X.dtype != torch.bfloat16:
        raise TypeError(f"X must be bfloat16 on the mixed readout path, got {X.dtype}")
    if X.dim() != 2:
        raise ValueError("X must be n x h")
    if not X.is_contiguous():
        raise ValueError("X must be contiguous")
    h = X.shape[1]
    if (a is None) == (Q is None):
        raise ValueError("pass exactly one of a (Gated) and Q (SDPAttention)")
    if a is not None:
        _require_f32_key("a", a)
        if a.numel() != h:
            raise ValueError("a must have h entries")
        if a_bias is not None:
            _require_f32_key("a_bias", a_bias)
            if a_bias.numel() != 1:
                raise ValueError("a_bias must have one entry")
    else:
        _require_f32_key("Q", Q)
        if Q.dim() != 2 or Q.shape[1] != h:
            raise RuntimeError(f"Q must be b x {h}, got {tuple(Q.shape)}")
        if a_bias is not None:
            raise ValueError("a_bias goes with a (Gated)")
        if node_seg is None:
            raise ValueError("SDPAttention scores need batch_node_index")
    if node_seg is not None:
        _require_i64("batch_node_index", node_seg)
        if node_seg.numel() != X.shape[0]:
            raise ValueError("batch_node_index must have one entry per row of X")


def node_scores_mixed(X: Tensor, *, a: Tensor | None = None, a_bias: Tensor | None = None,
                      Q: Tensor | None = None, node_seg: Tensor | None = None,
                      sqrt_key: float = 1.0) -> Tensor:
    """node_scores for bf16 X and fp32 keys (nt_node_scores_mixed): every element of a / a_bias / Q is
    rounded to bf16 (to nearest even) where the kernel loads it, so the scores are the bits of
    node_scores on a.to(bfloat16) / Q.to(bfloat16) with no bf16 copy of the key written.  A bf16 key
    belongs to node_scores."""
    _require_mixed_readout(X, a, a_bias, Q, node_seg)
    dev = _require_device(X, a, a_bias, Q, node_seg)
    n, h = X.shape
    s = torch.empty(n, dtype=torch.float32, device=dev)
    _run(dev, _lib.load().nt_node_scores_mixed,
         _ptr(X), n, h, _ptr(a), _ptr(a_bias), _ptr(Q), _ptr(node_seg), float(sqrt_key), NT_BF16,
         _ptr(s), _stream(dev))
    return s


def softmax_pool_backward_mixed(X: Tensor, scores: Tensor, seg_ptr: Tensor, perm: Tensor | None,
                                node_seg: Tensor, nseg: int, out: Tensor, dout: Tensor, *,
                                a: Tensor | None = None, Q: Tensor | None = None,
                                sqrt_key: float = 1.0) -> tuple[Tensor, Tensor, Tensor]:
    """softmax_pool_backward for bf16 X / out / dout and an fp32 key (nt_softmax_pool_backward_mixed): the
    key is rounded to bf16 where the kernel loads it; (dX bf16, ds fp32, P fp32) are the bits of
    softmax_pool_backward on the rounded key.  The fp32 key's gradient is formed from ds and P by the
    caller and stays fp32."""
    _require_mixed_readout(X, a, None, Q, node_seg)
    for name, t in (("out", out), ("dout", dout)):
        if t.dtype != torch.bfloat16:
            raise TypeError(f"{name} must be bfloat16 on the mixed readout path, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if t.dim() != 2 or t.shape[0] != nseg or t.shape[1] != X.shape[1]:
            raise ValueError(f"{name} must be nseg x h")
    if scores.dtype != torch.float32 or scores.numel() != X.shape[0] or not scores.is_contiguous():
        raise ValueError("scores must be contiguous fp32 with one entry per row of X")
    if seg_ptr.dtype != torch.int32 or seg_ptr.numel() != nseg + 1:
        raise ValueError("seg_ptr must be int32 of length nseg + 1")
    dev = _require_device(X, scores, seg_ptr, perm, node_seg, out, dout, a, Q)
    n, h = X.shape
    dX = torch.empty_like(X)
    ds = torch.empty(n, dtype=torch.float32, device=dev)
    P = torch.empty(nseg, h, dtype=torch.float32, device=dev)
    stats = torch.empty(max(3 * nseg, 1), dtype=torch.float32, device=dev)
    _run(dev, _lib.load().nt_softmax_pool_backward_mixed,
         _ptr(X), _ptr(scores), _ptr(seg_ptr), _ptr(perm), _ptr(node_seg), nseg, n, h, _ptr(out), _ptr(dout),
         _ptr(a), _ptr(Q), float(sqrt_key), NT_BF16, _ptr(stats), _ptr(dX), _ptr(ds), _ptr(P), _stream(dev))
    return dX, ds, P


# ------------------------------------------------------------------------------------ dropout
def dropout_residual(Y: Tensor, p: float, seed: int, offset: int = 0, *, base: Tensor | None = None,
                     out: Tensor | None = None) -> Tensor:
    """out = (base or 0) + keep * Y / (1 - p), keep a counter-based hash of (seed, offset + i)
    (chemprop.py:26 Dropout + residual.py:28; see include/notorch_amd.h).  The same call on a
    gradient with base=None is the backward."""
    dev = _require_device(Y, base, out)
    code = _require_feat("Y", Y)
    if not Y.is_contiguous():
        raise ValueError("Y must be contiguous")
    if base is not None:
        _require_feat("base", base, Y.dtype)
        if base.shape != Y.shape or not base.is_contiguous():
            raise ValueError("base must be a contiguous tensor shaped like Y")
    if out is None:
        out = torch.empty_like(Y)
    else:
        _require_feat("out", out, Y.dtype)
        if out.shape != Y.shape or not out.is_contiguous():
            raise ValueError("out must be a contiguous tensor shaped like Y")
    _run(dev, _lib.load().nt_dropout_residual,
         _ptr(base), _ptr(Y), Y.numel(), float(p), int(seed) & (2**64 - 1), int(offset), code, _ptr(out),
         _stream(dev))
    return out


# ------------------------------------------------------------------------- Rank-N-Contrast loss
def rnc_max_n() -> int:
    """Largest n of rnc_rank (what one workgroup's LDS and threads hold; the library's constant)."""
    return int(_lib.load().nt_rnc_max_n())


def _rnc_rank(entry: str, sim: Tensor, dist: Tensor, temp: float, eps: float,
              need_grad: bool) -> tuple[Tensor, Tensor | None]:
    dev = _require_device(sim, dist)
    _require_f32("sim", sim)
    _require_f32("dist", dist)
    if sim.dim() != 2 or sim.shape[0] != sim.shape[1] or dist.shape != sim.shape:
        raise ValueError(f"sim and dist must be n x n, got {tuple(sim.shape)} and {tuple(dist.shape)}")
    n = sim.shape[0]
    row_nll = torch.empty(n, dtype=torch.float32, device=dev)
    dsim = torch.empty_like(sim) if need_grad else None
    _run(dev, getattr(_lib.load(), entry),
         _ptr(sim), _ptr(dist), n, float(temp), float(eps), _ptr(row_nll), _ptr(dsim), _stream(dev))
    return row_nll, dsim


def rnc_rank(sim: Tensor, dist: Tensor, temp: float, eps: float, need_grad: bool) -> tuple[Tensor, Tensor | None]:
    """The ranking part of RankNContrastLoss for n x n fp32 sim and dist (nt_rnc_rank): row_nll[i] =
    sum_{j != i} (log denom_ij - sim_ij / temp) and, with need_grad, dsim = d(mean loss) / d sim from
    the same launch (else None: no n x n buffer is allocated)."""
    return _rnc_rank("nt_rnc_rank", sim, dist, temp, eps, need_grad)


def rnc_long_max_n() -> int:
    """Largest n of rnc_rank_long (16 positions per thread in 128.25 KiB of LDS; the library's constant)."""
    return int(_lib.load().nt_rnc_long_max_n())


def rnc_rank_long(sim: Tensor, dist: Tensor, temp: float, eps: float,
                  need_grad: bool) -> tuple[Tensor, Tensor | None]:
    """rnc_rank for n up to rnc_long_max_n() (nt_rnc_rank_long): the same arguments and results, equal to
    rnc_rank's to fp32 rounding (the per-thread part of the sums has another, equally fixed, order)."""
    return _rnc_rank("nt_rnc_rank_long", sim, dist, temp, eps, need_grad)


# ------------------------------------------------------------------------- task losses and ranking metrics
def task_loss_single_max() -> int:
    """Largest b * t that task_loss takes in one launch of one workgroup (the library's constant)."""
    return int(_lib.load().nt_task_loss_single_max())


def _byte_mask(name: str, m: Tensor | None, shape: tuple) -> Tensor | None:
    """A b x t mask as the bytes nt_task_loss / nt_rank_metric read (torch.bool is one byte per element)."""
    if m is None:
        return None
    if m.dtype != torch.bool:
        raise TypeError(f"{name} must be a bool tensor, got {m.dtype}")
    if tuple(m.shape) != shape or not m.is_contiguous():
        raise ValueError(f"{name} must be a contiguous tensor of shape {shape}, got {tuple(m.shape)}")
    return m.view(torch.uint8)


def task_loss(preds: Tensor, targets: Tensor, kind: str, mask: Tensor | None = None,
              sample_weights: Tensor | None = None, lt_mask: Tensor | None = None, gt_mask: Tensor | None = None,
              v_kl: float = 0.0, eps: float = 0.0, need_grad: bool = False) -> tuple[Tensor, Tensor | None]:
    """The element loss ``kind`` (a key of _lib.LOSS_CODES), its masked weighted reduction and, with need_grad,
    dLoss/dpreds from the same launch (nt_task_loss): preds b x t [x c] fp32 or bf16, targets b x t fp32, mask /
    lt_mask / gt_mask b x t bool, sample_weights b fp32.  Returns (loss, a 0-d fp32 tensor; dpreds in the dtype
    of preds, or None: no gradient buffer is allocated)."""
    dev = _require_device(preds, targets, mask, sample_weights, lt_mask, gt_mask)
    code = _require_feat("preds", preds)
    _require_f32("targets", targets)
    if kind not in _lib.LOSS_CODES:
        raise ValueError(f"unknown loss kind {kind!r} (one of {sorted(_lib.LOSS_CODES)})")
    if targets.dim() != 2 or preds.dim() not in (2, 3) or tuple(preds.shape[:2]) != tuple(targets.shape):
        raise ValueError(f"preds must be b x t [x c] and targets b x t, got {tuple(preds.shape)} and "
                         f"{tuple(targets.shape)}")
    b, t = targets.shape
    c = preds.shape[2] if preds.dim() == 3 else 1
    shape = (b, t)
    masks = [_byte_mask(n, m, shape) for n, m in (("mask", mask), ("lt_mask", lt_mask), ("gt_mask", gt_mask))]
    if sample_weights is not None:
        _require_f32("sample_weights", sample_weights)
        if tuple(sample_weights.shape) != (b,):
            raise ValueError(f"sample_weights must have shape ({b},), got {tuple(sample_weights.shape)}")
    lib = _lib.load()
    loss = torch.full((), float("nan"), dtype=torch.float32, device=dev) if b * t == 0 else \
        torch.empty((), dtype=torch.float32, device=dev)
    dpreds = torch.empty_like(preds) if need_grad else None
    ws_bytes = int(lib.nt_task_loss_workspace(b, t))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes > 0 else None
    _run(dev, lib.nt_task_loss,
         _ptr(preds), code, _ptr(targets), _ptr(masks[0]), _ptr(sample_weights), _ptr(masks[1]), _ptr(masks[2]),
         b, t, c, _lib.LOSS_CODES[kind], float(v_kl), float(eps), _ptr(loss), _ptr(dpreds), _ptr(ws), ws_bytes,
         _stream(dev))
    return loss, dpreds


def rank_metric_max_n() -> int:
    """Largest n of rank_metric (what one workgroup's LDS and threads hold; the library's constant)."""
    return int(_lib.load().nt_rank_metric_max_n())


def rank_metric(scores: Tensor, targets: Tensor, mask: Tensor | None = None) -> Tensor:
    """AUROC, average precision, P and N of every column of n x t fp32 scores and targets (nt_rank_metric): a
    t x 4 fp32 tensor.  An entry counts as positive where int(target) == 1, negative where it is 0, and is ignored
    otherwise or where the n x t bool mask is False; AUROC and AP are NaN for a column without both classes."""
    dev = _require_device(scores, targets, mask)
    _require_f32("scores", scores)
    _require_f32("targets", targets)
    if scores.dim() != 2 or scores.shape != targets.shape:
        raise ValueError(f"scores and targets must be n x t, got {tuple(scores.shape)} and {tuple(targets.shape)}")
    n, t = scores.shape
    m = _byte_mask("mask", mask, (n, t))
    out = torch.empty(t, 4, dtype=torch.float32, device=dev)
    _run(dev, _lib.load().nt_rank_metric, _ptr(scores), _ptr(targets), _ptr(m), n, t, _ptr(out), _stream(dev))
    return out


def rank_metric_long_max_n() -> int:
    """Largest n of rank_metric_long (P and N return as fp32 counts, exact up to 2^24; the library's constant)."""
    return int(_lib.load().nt_rank_metric_long_max_n())


def rank_metric_long(scores: Tensor, targets: Tensor, mask: Tensor | None = None,
                     workspace: Tensor | None = None) -> Tensor:
    """rank_metric for any n up to rank_metric_long_max_n() (nt_rank_metric_long): sorted runs of 4096 rows,
    merge passes and a tiled scan over several workgroups per column.  ``workspace`` is a contiguous uint8
    device tensor of at least nt_rank_metric_long_workspace(n, t) bytes, 16-byte aligned (its contents do not
    matter); without one the call allocates it."""
    dev = _require_device(scores, targets, mask, workspace)
    _require_f32("scores", scores)
    _require_f32("targets", targets)
    if scores.dim() != 2 or scores.shape != targets.shape:
        raise ValueError(f"scores and targets must be n x t, got {tuple(scores.shape)} and {tuple(targets.shape)}")
    n, t = scores.shape
    m = _byte_mask("mask", mask, (n, t))
    lib = _lib.load()
    ws_bytes = int(lib.nt_rank_metric_long_workspace(n, t))
    if workspace is None:
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes > 0 else None
    elif workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise TypeError(f"workspace must be a contiguous uint8 tensor, got {workspace.dtype}")
    out = torch.empty(t, 4, dtype=torch.float32, device=dev)
    _run(dev, lib.nt_rank_metric_long, _ptr(scores), _ptr(targets), _ptr(m), n, t, _ptr(out), _ptr(workspace),
         0 if workspace is None else workspace.numel(), _stream(dev))
    return out
