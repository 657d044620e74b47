"""Device engine behind ChempropBlock / readouts: the fused layer loop, its dispatch and the autograd
wrappers.  Graph layouts and plans live in _layout.py, the packed-weight cache in _weights.py.

Forward (per call, all on ``torch.cuda.current_stream()``, inputs already resident).  Which launch a
block takes is decided by forward_route; on a graph with a fused plan:

    nt_dmpnn_init         H0 = Xv[src] + Xe  fused with  S = scatter(act(H0), dst)  chemprop.py:82-83,37-39
      (GraphEmbedding models: nt_dmpnn_init_embed from the type indices, over the graph's type records)
    for l in 0..d-1:
      nt_dmpnn_update_fused  H_{l+1} = H_l + W_l (S[src] - act(H_l)[rev]) + b_l      chemprop.py:40-41, residual.py:28
                             S = scatter(act(H_{l+1}), dst)   (last layer: node = scatter(H_d, dst),
                                                               chemprop.py:86)

d + 1 launches (+ one nt_dmpnn_pack_weights_fk launch pair per new set of weights).  Training-mode
dropout keeps that sequence: nt_dmpnn_update_fused_dropout applies layer l's mask (p, seed,
dropout_offset(l, E, h)) to the update in the layer kernel's epilogue, ahead of the residual add and
the aggregation.  Without a fused plan:

    nt_dmpnn_init; for l: nt_dmpnn_update, nt_segment_reduce; nt_segment_reduce (node)   2 + 2d launches
      (dropout: nt_dmpnn_update without its residual, then nt_dropout_residual adds it back)

bf16 features (BASELINE config 3) run the same d + 1 launch sequence on the bf16 kernels
(csrc/bf16.hip: the 64-edge-tile update fused with the next aggregation).  Activations without a
kernel code, or layers that differ in activation / dropout, run layer by layer
(block_forward_layerwise).

Under bf16 autocast (autocast_bf16; block_forward(..., bf16_compute=True)) an fp32 block runs that bf16
sequence on fp32 leaves: nt_dmpnn_init_mixed / nt_dmpnn_init_embed_mixed read the fp32 features or
tables (one rounding of the fp32 sum), one nt_dmpnn_pack_weights_mixed launch writes the bf16 images of
W, W^T (training) and the bf16 biases of every layer (pack_layer_weights_bf16), and block_backward
returns dW / db in the parameter's dtype (the weight-gradient kernel's fp32 result for an fp32 weight).

Backward (training): the forward keeps (H_l, S_l) of every layer; per layer,
last to first (csrc/backward.hip, csrc/wgrad.hip), on the kernels backward_route picks:

    dW_l = G^T A_l, db_l = colsum(G), A_l = S_l[src] - act(H_l)[rev] formed while staging
    dA = G W_l and dS = scatter_sum(dA, src)
    nt_dmpnn_edge_backward   G <- G + act'(H_l) * (dS[dst] / c - scatter_sum(dA, rev))  (rev CSR)
      (max / min: nt_segment_arg + nt_dmpnn_edge_backward_arg, fp32 and bf16: dS[dst] reaches only the arg)

then dXe = G, dXv = scatter_sum(G, src).
"""
from __future__ import annotations

import contextlib
import os
import threading
from typing import NamedTuple, Optional, Sequence

import torch
from torch import Tensor

from notorch_amd import _lib
from notorch_amd import kernels as K
from notorch_amd._lib import NT_ACT_IDENTITY
from notorch_amd.data.models.graph import DeviceLayout
# some of these only for the callers that reach them as _engine.<name>
from notorch_amd.nn.gnn._layout import (HUB_DEGREE, LONG_SEGMENT, MAX_FUSED_IN_DEGREE, _degree_range,  # noqa: F401
                                        _validate_indices, backward_layout, dA_plan, dst_chunks, dst_layout,
                                        embed_records, fused_max_in_degree, fused_plan, hub_chunk_ids, hub_info,
                                        hub_run_table, mol_chunks, mol_layout, row_table, zero_rows_needed)
from notorch_amd.nn.gnn._weights import pack_layer_weights, pack_layer_weights_bf16, packed_transpose

_IDENTITY = (NT_ACT_IDENTITY, 0.0)
_RELU = (_lib.NT_ACT_RELU, 0.0)
# The routes' knobs, read at call time; forward_route / backward_route say what each decides and why.
_FUSED_DA = os.environ.get("NT_FUSED_DA", "1") != "0"  # A/B: 0 keeps dense_matmul + segment_reduce
_WGRAD_DEFAULT = "kernel"  # NT_WGRAD: "kernel", "kernel6" or "library"
BF16_WGRAD_MAX_H = 2048  # bf16: the largest h on the weight-gradient kernel
FP32_WGRAD_FK_MAX_H = 4096  # fp32: the largest h on nt_dmpnn_weight_grad_fk
BF16_FUSED_DROPOUT_MAX_H = 512  # bf16: the largest h with dropout in the fused layer launch
BF16_FUSED_PIECE4 = True  # bf16 rows of whole 8-byte pieces (h % 8 == 4) in the fused layer launch
NW4_MAX_EDGES = int(os.environ.get("NT_NW4_MAX_EDGES", "131072"))  # fp32: the most edges on 64-row tiles


def _bf16_backward_kernels(V: int, E: int, h: int) -> bool:
    """bf16 shapes whose backward runs dA on the layer kernel's dense mode (the W^T images packed in the
    forward) and dW on the weight-gradient kernel: rows of whole 16-byte pieces.  Narrower than
    K.fused_supported: h % 8 == 4 keeps the library dA / dW (moving it changes gradient bits)."""
    return h % 8 == 0 and 8 <= h <= 8192 and E < 2**31


def _fused_enabled() -> bool:
    return os.environ.get("NT_FUSED", "1") != "0"


def _fused_dropout_enabled() -> bool:
    """NT_FUSED_DROPOUT=0 (A/B) keeps training-mode dropout out of the fused layer launch."""
    return os.environ.get("NT_FUSED_DROPOUT", "1") != "0"


class ForwardRoute(NamedTuple):
    plan: bool  # ask fused_plan for a tile plan and run one fused launch per layer over it
    rows: int  # that plan's tile rows (64 or 128)
    dropout: bool  # the fused launch applies the dropout mask (nt_dmpnn_update_fused_dropout)
    fallback: str  # no plan asked for or none available: "persistent" or "update", + a segment reduce


def forward_route(V: int, E: int, h: int, dtype: torch.dtype, act, reduce: str, drop=None) -> ForwardRoute:
    """Which launches the d layers of a block take (every layer the same; drop = (p, seed) or None).

    A plan is asked for when NT_FUSED is not 0 and K.fused_supported(V, E, h, dtype) holds, except:
      * bf16 with h % 8 == 4 (rows of whole 8-byte pieces, h <= 512, update_bf16_kernel<.., W = 4, ..>)
        when BF16_FUSED_PIECE4 is False.  Measured at h = 300 on config 2's batch against the parent
        commit's library (three alternating fresh-process runs): forward 0.256-0.257 ms
        against 1.020-1.021 (bf16 storage) and 0.274-0.277 against 1.046-1.055 (bf16 autocast), the
        parent's spread 0.001 / 0.009 ms; the training step 1.74-1.76 against 2.63-2.64 ms.
      * with dropout, when NT_FUSED_DROPOUT=0 (A/B), and in bf16 when h % 8 != 0 (those rows have no
        dropout instances) or h > BF16_FUSED_DROPOUT_MAX_H: fp32 and bf16 at h = 512 are measured
        faster; above it the column-pass kernel's dropout epilogue is tested at kernel
        level but not timed.
    rows is the layer kernel's tile capacity over every layer of the block (the last aggregates without
    the activation), with two overrides.  fp32 at h <= 320 on graphs of at most NW4_MAX_EDGES edges
    takes 64-row tiles walked by two 4-wave workgroups per CU (update_fk.hip, fk_nw4: one's epilogue
    overlaps the other's K loop) unless NT_FK_NW=8; larger graphs keep the 128-row walk.  Measured per
    launch (tools/r4_sweep.sh, tools/r4_nw4b.sh): 78k edges 115-117 vs 125 us; 155k 243 vs 244; 310k
    465 vs 462; 456k (polymer-16) 720 vs 691; 621k 904 vs 895.  bf16 dropout lives in the 64-row
    kernel's epilogue, whatever NT_BF16_KERNEL selects.

    fallback is what runs when no plan is asked for or fused_plan has none (in-degree > 32 in bf16):
    "persistent" (fp32 without dropout, where a plan was asked for: the persistent layer kernel without
    its aggregation) or "update" (nt_dmpnn_update; with dropout without its residual, then
    nt_dropout_residual), each followed by a separate segment reduce."""
    fp32 = dtype == torch.float32
    ok = _fused_enabled() and K.fused_supported(V, E, h, dtype) and (fp32 or h % 8 == 0 or BF16_FUSED_PIECE4)
    if drop is not None:
        ok = ok and _fused_dropout_enabled() and (fp32 or (h % 8 == 0 and h <= BF16_FUSED_DROPOUT_MAX_H))
    if not ok:
        return ForwardRoute(False, 64, False, "update")
    rows = min(K.fused_tile_rows(h, dtype, act, reduce, act), K.fused_tile_rows(h, dtype, act, reduce, _IDENTITY))
    if rows == 128 and fp32 and h <= 320 and E <= NW4_MAX_EDGES and os.environ.get("NT_FK_NW") != "8":
        rows = 64
    if drop is not None and not fp32:
        rows = 64
    return ForwardRoute(True, rows, drop is not None, "persistent" if fp32 and drop is None else "update")


class BackwardRoute(NamedTuple):
    dW: str  # "fk", "bf16x6", "bf16" or "library"
    dA: str  # "plan", "fk_dense", "bf16_dense" or "mm"


def backward_route(V: int, E: int, h: int, gdtype: torch.dtype) -> BackwardRoute:
    """Which kernels the layers of block_backward take for a gradient of dtype gdtype (an fp32 master
    weight under bf16 compute follows the bf16 gradient).  NT_WGRAD: "kernel" (default), "kernel6" or
    "library".

    dW, fp32: "fk" = nt_dmpnn_weight_grad_fk (the two-part fp16 split on the forward's bounds) for
    h <= 320, and on its variant that tiles dW in both dimensions for h % 4 == 0 up to
    FP32_WGRAD_FK_MAX_H (the entry accepts up to 8192; measured, DESIGN.md §4: 2.3 to 3.6 times faster
    than the bf16x6 kernel at 384, 512, 1024, 2048 and 4096, the training step 23 % to 40 % shorter;
    4096 is the largest size measured); else, and with NT_WGRAD=kernel6, "bf16x6" =
    nt_dmpnn_weight_grad.  Both form A = S[src] - act(H)[rev] while staging.
    dW, bf16: "bf16" = the bf16 weight-gradient kernel (A rounded to bf16 as the forward's message, fp32
    partials; above h = 512 its variant that tiles dW in both dimensions) at the shapes of
    _bf16_backward_kernels up to BF16_WGRAD_MAX_H (K.weight_grad accepts every h % 8 == 0 up to 8192;
    measured, DESIGN.md §4: the kernel wins at 640 and 1024, is 14 % behind the library route at 2048
    and 19 % at 4096).
    dW "library" (NT_WGRAD=library, and every other case): nt_dmpnn_message + the split-K GEMM.

    dA, fp32 where K.fused_supported holds: "plan" = dA and dS = sum_src dA in one fused launch of the
    layer kernel over dA_plan (where that has no plan, and with NT_FUSED_DA=0, "fk_dense" =
    nt_dmpnn_dense_matmul + segment reduce).  bf16 at the shapes of _bf16_backward_kernels: "bf16_dense" =
    the bf16 layer kernel without gathers, unless NT_WGRAD=library or NT_BF16_DA is not "kernel".
    Otherwise "mm": torch.mm + segment reduce."""
    wgrad = os.environ.get("NT_WGRAD", _WGRAD_DEFAULT)
    if gdtype == torch.float32:
        dW = "library"
        if wgrad in ("kernel", "kernel6"):
            fk = wgrad == "kernel" and (h <= 320 or (h % 4 == 0 and h <= FP32_WGRAD_FK_MAX_H))
            dW = "fk" if fk else "bf16x6"
        dense = K.fused_supported(V, E, h, gdtype)
        return BackwardRoute(dW, ("plan" if _FUSED_DA else "fk_dense") if dense else "mm")
    kernels = gdtype == torch.bfloat16 and wgrad != "library" and _bf16_backward_kernels(V, E, h)
    return BackwardRoute("bf16" if kernels and h <= BF16_WGRAD_MAX_H else "library",
                         "bf16_dense" if kernels and os.environ.get("NT_BF16_DA", "kernel") == "kernel" else "mm")


# Optional per-launch timer for the dominant kernel (bench.py sets it): a list that receives
# (start, end) torch.cuda.Event pairs recorded on the launch stream around every nt_dmpnn_update.
UPDATE_EVENTS: Optional[list] = None
# What the last layer-update launch ran (bench.py's roofline): kernel, numerics, padded MFMA shape.
LAST_UPDATE_INFO: dict = {}


def _note_update(kind: str, dtype: torch.dtype, h: int, rows: int = 0) -> None:
    """Record which layer kernel the forward ran (bench labels): the variant is the library's own
    report of its last launch (nt_last_kernel), so the label cannot drift from the dispatch."""
    kp, np_ = 32 * ((h + 31) // 32), 16 * ((h + 15) // 16)
    launched = _lib.load().nt_last_kernel().decode()
    short = launched.split(" ")[0].rstrip(":") or "update"
    if dtype == torch.bfloat16:
        info = dict(numerics="bf16 storage, bf16 MFMA, fp32 accumulate", products=1)
    elif short == "update_fk_kernel":
        info = dict(numerics="fp32 via scaled two-part fp16 split (3 fp16 MFMA products, fp32 accumulate)",
                    products=3)
    else:
        info = dict(numerics="exact fp32 MFMA", products=1)
    tail = {"fused": "aggregation of the next layer fused",
            "persistent": "no tile plan: hub graph, aggregation by the chunked segment reduce"}.get(kind, "unfused")
    info.update(kernel=f"{launched} ({tail})", kernel_short=short.replace("_kernel", ""),
                fused=kind == "fused", kpad=kp, npad=np_, rows=rows)
    LAST_UPDATE_INFO.clear()
    LAST_UPDATE_INFO.update(info)


def _aggregate(X, seg_ptr, perm, nseg, reduce, act, chunks, out=None, amax=None):
    """scatter(act(X), seg) by the chunked reduce (skewed segments) or the plain one; amax (fp32,
    1 device float) is raised to max|out| (fused into the chunked reduce, a separate pass otherwise)."""
    if chunks is not None:
        return K.segment_reduce_chunked(X, seg_ptr, perm, nseg, chunks, reduce=reduce, act=act, out=out,
                                        amax=amax)
    out = K.segment_reduce(X, seg_ptr, perm, nseg, reduce=reduce, act=act, out=out)
    if amax is not None:
        K.absmax(out, amax)
    return out


# ------------------------------------------------------------------------------------ forward
def autocast_bf16(device) -> bool:
    """bf16 autocast is active for this device: inside torch.autocast("cuda", dtype=torch.bfloat16) and
    not inside a nested autocast(enabled=False) or an autocast of another dtype."""
    if torch.device(device).type != "cuda":
        return False
    return torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16


def block_forward(
    Xv: Tensor,
    Xe: Tensor,
    src: Tensor,
    rev: Tensor,
    lay: DeviceLayout,
    weights: Sequence[Tensor],
    biases: Sequence[Optional[Tensor]],
    act: tuple[int, float],
    reduce: str,
    residual: bool,
    keep_states: bool = False,
    drop: Optional[tuple[float, int]] = None,
    bf16_compute: bool = False,
) -> tuple[Tensor, Tensor, list[tuple[Tensor, Tensor]]]:
    """Run the kernel sequence; returns (node, H_d, states) with states = [(H_l, S_l, amax_l)] for
    l = 0..d-1 (each layer's input hidden state, its aggregation and the fp32 split bounds (max|H_l|,
    max|S_l|) on the device, or an empty tensor) if keep_states, else [].
    drop = (p, seed): training-mode dropout of every layer update (layer l draws from
    dropout_offset(l, E, h)).
    bf16_compute (the block under bf16 autocast): fp32 Xv / Xe enter through nt_dmpnn_init_mixed (one
    rounding of the fp32 sum), fp32 weights and biases through nt_dmpnn_pack_weights_mixed
    (_layers_forward), and the bf16 kernel sequence runs unchanged; outputs and states are bf16.  Xv and
    Xe share one dtype here (ChempropBlock casts the odd one of an fp32 / bf16 pair)."""
    V = Xv.shape[0]
    if bf16_compute and Xv.dtype == torch.float32:
        chunks = dst_chunks(lay)
        if len(weights) == 0 or chunks is not None:  # as the bf16 path: H0, then the (chunked) reduce
            H, S = K.dmpnn_init_mixed(Xv, Xe, src)
            if len(weights):
                S = _aggregate(H, lay.dst_ptr, lay.dst_perm, V, reduce, act, chunks)
        else:
            H, S = K.dmpnn_init_mixed(Xv, Xe, src, lay.dst_ptr, lay.dst_perm, act=act, reduce=reduce)
        return _layers_forward(H, S, V, src, rev, lay, weights, biases, act, reduce, residual, keep_states,
                               drop)
    amax = _amax_buffer(len(weights), Xv, reuse=not keep_states)
    a0 = None if amax is None else amax[0]
    if len(weights) == 0:
        H, _ = K.dmpnn_init(Xv, Xe, src)
        return _layers_forward(H, None, V, src, rev, lay, weights, biases, act, reduce, residual, keep_states,
                               drop)
    chunks = dst_chunks(lay)
    pitch = row_pitch(Xv.shape[1], Xv.dtype, chunks is not None) if (not keep_states and drop is None) else None
    if chunks is not None and Xv.dtype == torch.float32 and Xv.shape[1] >= 128 and Xv.shape[1] % 4 == 0:
        # hubs: the wave-per-node init for every node of in-degree <= MAX_FUSED_IN_DEGREE, then the
        # chunked init (the initial gather inside pass 1 of the chunked reduce) over the hubs' chunks
        # alone, so no wave walks a hub's hundreds of in-edges and H0 is written once
        H, S = K.dmpnn_init(Xv, Xe, src, lay.dst_ptr, lay.dst_perm, act=act, reduce=reduce, amax=a0, pitch=pitch,
                            skip_degree=MAX_FUSED_IN_DEGREE)
        K.dmpnn_init_chunked(Xv, Xe, src, lay.dst_ptr, lay.dst_perm, chunks, act=act, reduce=reduce,
                             amax=a0, pitch=pitch, H0=H, S=S, chunk_ids=hub_chunk_ids(lay, chunks))
    elif chunks is not None and Xv.dtype == torch.float32:
        # the chunked init over every node (h < 128: no wave-per-node init)
        H, S = K.dmpnn_init_chunked(Xv, Xe, src, lay.dst_ptr, lay.dst_perm, chunks, act=act, reduce=reduce, amax=a0,
                                    pitch=pitch)
    elif chunks is not None:
        H, _ = K.dmpnn_init(Xv, Xe, src, amax=a0)
        S = _aggregate(H, lay.dst_ptr, lay.dst_perm, V, reduce, act, chunks, amax=None if a0 is None else a0[1:2])
    else:
        H, S = K.dmpnn_init(Xv, Xe, src, lay.dst_ptr, lay.dst_perm, act=act, reduce=reduce, amax=a0, pitch=pitch)
    return _layers_forward(H, S, V, src, rev, lay, weights, biases, act, reduce, residual, keep_states, drop,
                           amax)


def row_pitch(h: int, dtype: torch.dtype, hubs: bool = False) -> Optional[int]:
    """Row pitch of the intermediate H_l / S_l of an inference forward: fp32 rows of h % 8 != 0 floats
    padded to a 32-byte multiple (h = 300 -> 304), so that no row shares a 32-B sector with its
    neighbour: the dst-ordered row stores of the init and of the layer kernels then write whole
    sectors, and every 16-B gather piece of a row lies in one sector (measured with tools/r5_pitch.sh:
    the layer kernel at h = 304 runs 113.5 us against 121.1 at h = 300, the same MFMA work).  None:
    dense rows (h % 8 == 0 already, bf16, h < 128, or NT_ROW_PAD=0).  Hub graphs (hubs: a node of
    in-degree > MAX_FUSED_IN_DEGREE, dst_chunks) pad to whole 128-byte L2 lines instead (h = 300 ->
    320): polymer-16 2.44 -> 2.39 ms per step, layer 658 -> 638 us (tools/r5_align.sh), while 128-B
    rows lose at config 2 (389 -> 404 us per step) and at qm9-32k (2.99 -> 3.07 ms, tools/r5_align2.sh)."""
    align = _ROW_ALIGN or (32 if hubs else 8)
    if dtype != torch.float32 or h % 4 or h % align == 0 or h < 128 or not _ROW_PAD:
        return None
    return (h + align - 1) // align * align


_NO_AMAX = torch.empty(0)  # a state without a valid amax row (bf16, or a path that skips the chain)
_ROW_PAD = os.environ.get("NT_ROW_PAD", "1") != "0"  # A/B: 0 = dense intermediate rows
_ROW_ALIGN = int(os.environ.get("NT_ROW_ALIGN", "0"))  # A/B: pitch multiple in floats (0: by graph size)

# per (device, stream, depth): a ring of _AMAX_RING amax buffers for forwards that keep no states,
# zeroed all at once every _AMAX_RING forwards instead of one fill kernel per forward
_AMAX_RING = 64
_amax_rings: dict = {}
_amax_lock = threading.Lock()


def _amax_buffer(d: int, X: Tensor, reuse: bool = False) -> Optional[Tensor]:
    """(d + 1) x 2 zeros: row l = (max|H_l|, max|S_l|), the fp32 layer kernel's split scales (the
    init raises row 0, layer l reads row l and raises row l + 1).  None for bf16.
    reuse (forwards whose states nothing keeps): the next buffer of this stream's ring; the whole ring
    is zeroed when it wraps, which stream order makes safe (the forward that used a buffer last has
    finished before the fill that re-zeroes it runs).  Not while a graph is being captured (a replay
    must re-zero its own buffer)."""
    if X.dtype != torch.float32 or d == 0:
        return None
    if not reuse or torch.cuda.is_current_stream_capturing():
        return torch.zeros(d + 1, 2, dtype=torch.float32, device=X.device)
    key = (X.device, torch.cuda.current_stream(X.device).cuda_stream, d)
    with _amax_lock:  # threads sharing a stream take distinct slots; the wrap-time zeroing is enqueued once
        ent = _amax_rings.get(key)
        if ent is None:
            ent = _amax_rings[key] = [torch.empty(_AMAX_RING, d + 1, 2, dtype=torch.float32, device=X.device), 0]
        buf, i = ent
        if i == 0:
            buf.zero_()
        ent[1] = (i + 1) % _AMAX_RING
    return buf[i]


def dropout_offset(l: int, E: int, h: int) -> int:
    """First hash counter of layer l's dropout mask: layers draw disjoint counter ranges."""
    return l * E * h


def draw_dropout_seed() -> int:
    """One 62-bit seed from torch's default CPU generator (so torch.manual_seed reproduces masks)."""
    return int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())


def block_forward_embedded(
    node_table: Tensor,
    node_types: Tensor,
    edge_table: Tensor,
    edge_types: Tensor,
    src: Tensor,
    rev: Tensor,
    lay: DeviceLayout,
    weights: Sequence[Tensor],
    biases: Sequence[Optional[Tensor]],
    act: tuple[int, float],
    reduce: str,
    residual: bool,
    keep_states: bool = False,
    drop: Optional[tuple[float, int]] = None,
    validate: bool = True,
    bf16_compute: bool = False,
) -> tuple[Tensor, Tensor, list[tuple[Tensor, Tensor]]]:
    """block_forward with GraphEmbedding fused into the initial gather (nt_dmpnn_init_embed):
    Xv / Xe are never materialised.  Returns (node, H_d, states) like it.  bf16_compute (bf16 autocast):
    fp32 tables enter through nt_dmpnn_init_embed_mixed and the bf16 kernel sequence runs (bf16 outputs)."""
    V, d = node_types.shape[0], len(weights)
    if bf16_compute and node_table.dtype == torch.float32:
        H, S = embed_init_mixed(node_table, node_types, edge_table, edge_types, src, lay, d, act, reduce, validate)
        return _layers_forward(H, S, V, src, rev, lay, weights, biases, act, reduce, residual, keep_states, drop)
    if d == 0:
        H, _ = K.dmpnn_init_embed(node_table, node_types, edge_table, edge_types, src, validate=validate)
        return _layers_forward(H, None, V, src, rev, lay, weights, biases, act, reduce, residual, keep_states,
                               drop)
    amax = _amax_buffer(d, node_table, reuse=not keep_states)
    k72 = node_types.dim() == 2 and node_types.shape[1] == 7 and edge_types.dim() == 2 and edge_types.shape[1] == 2
    pitch = None
    if k72 and not keep_states and drop is None:
        pitch = row_pitch(node_table.shape[1], node_table.dtype)
    rec = None
    if k72 and node_table.dtype == torch.float32 and embed_wave_ok(node_table.shape[0], edge_table.shape[0],
                                                                   node_table.shape[1]):
        rec = embed_records(lay, node_types, node_table.shape[0], edge_types, edge_table.shape[0], src)
    H, S = K.dmpnn_init_embed(node_table, node_types, edge_table, edge_types, src, lay.dst_ptr,
                              lay.dst_perm, act=act, reduce=reduce, validate=validate,
                              amax=None if amax is None else amax[0], pitch=pitch, records=rec)
    return _layers_forward(H, S, V, src, rev, lay, weights, biases, act, reduce, residual, keep_states, drop,
                           amax)


def embed_init_mixed(node_table, node_types, edge_table, edge_types, src, lay, nlayers, act, reduce, validate):
    """(H0, S) in bf16 from fp32 embedding tables (nt_dmpnn_init_embed_mixed); S is None for depth 0.
    Routed as block_forward routes fp32 features: on a graph with long segments (dst_chunks) H0 alone,
    then the chunked reduce, so the fused and the unfused embedding sum S in the same order."""
    chunks = dst_chunks(lay)
    if nlayers == 0 or chunks is not None:
        H, S = K.dmpnn_init_embed_mixed(node_table, node_types, edge_table, edge_types, src, validate=validate)
        if nlayers:
            S = _aggregate(H, lay.dst_ptr, lay.dst_perm, node_types.shape[0], reduce, act, chunks)
        return H, S
    return K.dmpnn_init_embed_mixed(node_table, node_types, edge_table, edge_types, src, lay.dst_ptr,
                                    lay.dst_perm, act=act, reduce=reduce, validate=validate)


def _layers_forward(H, S, V, src, rev, lay, weights, biases, act, reduce, residual, keep_states, drop=None,
                    amax=None):
    """The d layers + final node scatter, from H0 and layer 0's aggregation S, on the launches
    forward_route picks.  drop = (p, seed): training-mode dropout of every layer's update.  amax (fp32):
    the split scales, row 0 filled by the init (see _amax_buffer)."""
    d = len(weights)
    chunks = dst_chunks(lay)
    if d == 0:
        node = _aggregate(H, lay.dst_ptr, lay.dst_perm, V, reduce, _IDENTITY, chunks)
        return node, H, []
    # a training forward (states kept for the kernel backward) packs the dA images of W^T alongside
    E, h = H.shape
    if H.dtype == torch.bfloat16 and any(p is not None and p.dtype == torch.float32
                                         for p in (*weights, *biases)):
        # bf16 compute on fp32 master parameters (bf16 autocast): their bf16 images and bias copies, and
        # in a training forward whose backward runs dA on the bf16 layer kernel the W^T images, in one launch
        Wps, biases = pack_layer_weights_bf16(
            weights, biases, with_t=keep_states and _bf16_backward_kernels(V, E, h))
    else:
        Wps = pack_layer_weights(weights, with_t=keep_states and H.dtype == torch.float32)
    if H.dtype == torch.float32 and amax is None:
        amax = _amax_buffer(d, H)
        K.absmax(H, amax[0, 0:1])
        K.absmax(S, amax[0, 1:2])
    route = forward_route(V, E, h, H.dtype, act, reduce, drop)
    plan = fused_plan(lay, V, E, route.rows, H.dtype) if route.plan else None
    if plan is not None:
        return _fused_forward(H, S, src, rev, lay, plan, route.rows, Wps, biases, act, reduce, residual,
                              keep_states, amax, drop)
    if not H.is_contiguous():  # row-padded init output (row_pitch) on a graph the fused plan cannot take
        H, S = H.contiguous(), S.contiguous()
    states = []
    spare: Optional[Tensor] = None  # ping-pong buffer when states are not kept
    persistent = route.fallback == "persistent"
    timer = UPDATE_EVENTS
    for l in range(d):
        if keep_states:  # the amax row is valid where the persistent kernel keeps the chain
            states.append((H, S, amax[l] if amax is not None and (persistent or l == 0) else _NO_AMAX))
        if timer is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        b_l = None if biases[l] is None else biases[l].detach()
        if drop is not None:
            U = K.dmpnn_update(H, S, src, rev, Wps[l], b_l, residual=False, act=act, out=spare)
            Hn = K.dropout_residual(U, drop[0], drop[1], dropout_offset(l, E, h),
                                    base=H if residual else None, out=U)
        elif persistent:
            Hn, _ = K.dmpnn_update_fused(H, S, src, rev, Wps[l], b_l, residual=residual, act=act,
                                         amax_in=amax[l], amax_out=amax[l + 1], out=spare)
        else:
            Hn = K.dmpnn_update(H, S, src, rev, Wps[l], b_l, residual=residual, act=act, out=spare)
        if timer is not None:
            ev[1].record()
            timer.append(ev)
        if l == 0:
            _note_update("persistent" if persistent else "unfused", H.dtype, h)
        if l < d - 1:
            S = _aggregate(Hn, lay.dst_ptr, lay.dst_perm, V, reduce, act, chunks,
                           out=None if keep_states else S, amax=amax[l + 1, 1:2] if persistent else None)
        if not keep_states:
            spare = H  # H_l is dead once H_{l+1} exists: reuse its buffer for H_{l+2}
        H = Hn
    node = _aggregate(H, lay.dst_ptr, lay.dst_perm, V, reduce, _IDENTITY, chunks)
    return node, H, states


EMBED_TABLE_BYTES = 72 * 1024  # LDS the wave-per-node embedding init holds the two tables in (embed.hip kTabB)


def embed_wave_ok(nv: int, ne: int, h: int) -> bool:
    """The wave-per-node fused embedding init applies (fp32, 7 + 2 type columns checked by the caller):
    both tables plus a zero row each fit its LDS, fewer than 255 types of each kind."""
    return h % 4 == 0 and h <= 512 and nv < 255 and ne < 255 and (nv + ne + 2) * h * 4 <= EMBED_TABLE_BYTES


def _fused_forward(H, S, src, rev, lay, plan, rows, Wps, biases, act, reduce, residual, keep_states, amax,
                   drop=None):
    """One launch per layer over the fused plan; drop = (p, seed): layer l's update passes the dropout
    mask of (p, seed, dropout_offset(l, E, h)) in the same launch."""
    tile_ptr, ntiles, dsts, zero_fill = plan
    E, h = H.shape
    # zero fills only where a row is read or returned (zero_rows_needed): the last layer's node output;
    # an intermediate S only if some source node has no in-edge
    zf_out, zf_mid, _ = zero_rows_needed(lay, src, S.shape[0]) if zero_fill else (False, False, False)
    d = len(Wps)
    rt = row_table(lay, dsts, src, rev, S.shape[0])
    states = []
    spare_H: Optional[Tensor] = None
    spare_S: Optional[Tensor] = None
    timer = UPDATE_EVENTS
    maxdeg = fused_max_in_degree(lay)
    hubs = hub_info(lay)
    part = None
    if hubs is not None:  # hub sub-runs: the layer writes their partials, hub_combine finishes the hubs
        rt, nslots, hub_ids, slot_ptr = hub_run_table(lay, rt, tile_ptr, dsts, max(1, maxdeg))
        part = torch.empty(max(nslots, 1), H.shape[1], dtype=torch.float32, device=H.device)
    for l in range(d):
        last = l == d - 1
        if keep_states:
            states.append((H, S, _NO_AMAX if amax is None else amax[l]))
        if timer is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        # intermediate layers keep the input's row pitch (row_pitch); the block's outputs are dense
        pitch = H.shape[1] if last else H.stride(0)
        if spare_H is not None and spare_H.stride(0) != pitch:
            spare_H = spare_S = None
        Hn, Sn = K.dmpnn_update_fused(
            H, S, src, rev, Wps[l], None if biases[l] is None else biases[l].detach(),
            residual=residual, act=act, plan=(tile_ptr, ntiles, dsts), tile_rows=rows, max_in_degree=maxdeg,
            perm=lay.dst_perm, reduce=reduce, agg_act=_IDENTITY if last else act,
            zero_fill=zf_out if last else zf_mid,
            amax_in=None if amax is None else amax[l],
            amax_out=None if (amax is None or last) else amax[l + 1],  # row d has no reader
            row_table=rt, out=spare_H, S_out=None if last else spare_S, pitch_out=pitch, S_part=part,
            dropout=None if drop is None else (drop[0], drop[1], dropout_offset(l, E, h)),
        )
        if timer is not None:
            ev[1].record()
            timer.append(ev)
        if hubs is not None:  # the hubs' S_out rows from the launch's sub-run partials
            K.hub_combine(part, hub_ids, slot_ptr, lay.dst_ptr, Sn, reduce=reduce,
                          amax=None if (amax is None or last) else amax[l + 1, 1:2])
        if l == 0:
            _note_update("fused", H.dtype, H.shape[1], rows)
        if not keep_states:
            spare_H = H
            spare_S = S
        H, S = Hn, Sn
    return S, H, states


# ------------------------------------------------------------------------------------ autograd
def _torch_scatter(x: Tensor, index: Tensor, dim_size: int, reduce: str) -> Tensor:
    """torch_scatter.scatter semantics (empty segment -> 0) in device ops, for the backward."""
    out = torch.zeros(dim_size, x.shape[1], dtype=x.dtype, device=x.device)
    idx = index.view(-1, 1).expand_as(x)
    if reduce == "sum":
        return out.scatter_add(0, idx, x)
    red = {"mean": "mean", "max": "amax", "min": "amin"}[reduce]
    return out.scatter_reduce(0, idx, x, reduce=red, include_self=False)


def _torch_block(Xv, Xe, edge_index, rev, weights, biases, act_mods, reduce, residual, masks=None):
    """The block in device torch ops (the recompute backwards differentiate it): act_mods[l] is layer
    l's activation module, masks[l] its dropout mask keep / (1 - p) or None."""
    src, dst = edge_index[0], edge_index[1]
    V = Xv.shape[0]
    H = Xv[src] + Xe
    for l, (W, b) in enumerate(zip(weights, biases)):
        M = act_mods[l](H)
        S = _torch_scatter(M, dst, V, reduce)
        U = torch.nn.functional.linear(S[src] - M[rev], W, b)
        if masks is not None and masks[l] is not None:
            U = U * masks[l]
        H = H + U if residual else U
    return _torch_scatter(H, dst, V, reduce), H


def _dropout_masks(drops, E: int, h: int, like: Tensor) -> Optional[list]:
    """Per layer the dropout mask keep / (1 - p) of drops[l] = (p, seed), regenerated by the kernel's
    hash in like's dtype (None for a layer without dropout); None if no layer has dropout."""
    if all(dr is None for dr in drops):
        return None
    ones = torch.ones(E, h, dtype=like.dtype, device=like.device)
    return [None if dr is None else K.dropout_residual(ones, dr[0], dr[1], dropout_offset(l, E, h))
            for l, dr in enumerate(drops)]


def _recompute_grads(outs, douts, leaves) -> list:
    """Gradients of the recomputed outputs whose gradient arrived (dout not None) in leaf order: None for
    a leaf that is None, needs no gradient or is unused."""
    pairs = [(o, g) for o, g in zip(outs, douts) if g is not None]
    live = [t for t in leaves if t is not None and t.requires_grad]
    got = iter(torch.autograd.grad([o for o, _ in pairs], live, [g for _, g in pairs], allow_unused=True))
    return [next(got) if t is not None and t.requires_grad else None for t in leaves]


def _save_block(ctx, inputs, params, states=(), H_last=None) -> None:
    """save_for_backward: the tensor inputs, the parameters (an empty placeholder for None), the
    flattened (H_l, S_l, amax_l) states and, for a max / min reduce, H_d (the final node scatter's arg is
    taken over it)."""
    flat = [t for hs in states for t in hs]
    if H_last is not None:
        flat.append(H_last)
    ctx.save_for_backward(*inputs, *[p if p is not None else torch.empty(0) for p in params], *flat)
    ctx.is_none = [p is None for p in params]


def _saved_block(ctx, ninputs: int):
    """_save_block's (inputs, params with their Nones, states, H_last or None)."""
    saved = ctx.saved_tensors
    n = ninputs + len(ctx.is_none)
    params = [None if none else p for p, none in zip(saved[ninputs:n], ctx.is_none)]
    flat = saved[n:]
    states = [tuple(flat[i:i + 3]) for i in range(0, len(flat) - 2, 3)]
    return saved[:ninputs], params, states, flat[-1] if len(flat) % 3 else None


def _param_grads(dWs, dbs, params, need, nfix: int, nlayers: int) -> list:
    """block_backward's dW / db as the Function's results for (*weights, *biases): None where the
    parameter is None or needs no gradient, db in the bias's dtype."""
    return [dW if need[nfix + i] else None for i, dW in enumerate(dWs)] + [
        None if p is None or not need[nfix + nlayers + i] else dbs[i].to(p.dtype)
        for i, p in enumerate(params[nlayers:])]


# ------------------------------------------------------------------------------------ layerwise
# Blocks the fused kernels do not take as one unit: an activation outside the kernels' codes (any
# nn.Module, chemprop.py:17,24,37), or layers that differ in activation or dropout.  Every layer
# runs unfused on the device: M = act(H) as the module's own elementwise op when it has no kernel
# code, then the segment-reduce and update kernels on M with the identity activation
# (S = scatter(M, dst), U = W (S[src] - M[rev]) + b), dropout by the hash kernel, residual add.
def layer_act(act_mod: torch.nn.Module) -> Optional[tuple[int, float]]:
    try:
        return K.act_code(act_mod)
    except NotImplementedError:
        return None


def block_forward_layerwise(Xv, Xe, src, rev, lay, acts, weights, biases, drops, reduce, residual):
    """acts[l] = (module, kernel code or None); drops[l] = (p, seed) or None.  Returns (node, H_d)."""
    V = Xv.shape[0]
    H, _ = K.dmpnn_init(Xv, Xe, src)
    chunks = dst_chunks(lay)
    E, h = H.shape
    for l, ((mod, code), W, b) in enumerate(zip(acts, weights, biases)):
        if code is None:
            M, code_l = mod(H).contiguous(), _IDENTITY
        else:
            M, code_l = H, code
        S = _aggregate(M, lay.dst_ptr, lay.dst_perm, V, reduce, code_l, chunks)
        Wp = pack_layer_weights([W])[0]
        U = K.dmpnn_update(M, S, src, rev, Wp, None if b is None else b.detach(), residual=False, act=code_l)
        if drops[l] is not None:
            H = K.dropout_residual(U, drops[l][0], drops[l][1], dropout_offset(l, E, h),
                                   base=H if residual else None, out=U)
        else:
            H = H + U if residual else U
    node = _aggregate(H, lay.dst_ptr, lay.dst_perm, V, reduce, _IDENTITY, chunks)
    return node, H


class LayerwiseBlockFunction(torch.autograd.Function):
    """Kernel forward (block_forward_layerwise); backward by recomputing the same math in PyTorch
    device ops under autograd (any activation module, per-layer dropout masks regenerated by the
    hash kernel).  The activation modules' own parameters (e.g. nn.PReLU's slope) are inputs of
    the Function and get their gradients from the recompute; the RNG state of the forward is
    restored for the recompute, so a stochastic activation (nn.RReLU in training) draws the same
    values in both."""

    NFIX = 11  # inputs ahead of the layer and activation parameters

    @staticmethod
    def forward(ctx, Xv, Xe, edge_index, rev, lay, acts, drops, reduce, residual, nlayers, nact, *params):
        weights, biases = list(params[:nlayers]), list(params[nlayers:2 * nlayers])
        dev = Xv.device
        ctx.rng = (torch.get_rng_state(), torch.cuda.get_rng_state(dev))
        node, H = block_forward_layerwise(Xv, Xe, edge_index[0].contiguous(), rev, lay, acts, weights,
                                          biases, drops, reduce, residual)
        _save_block(ctx, (Xv, Xe, edge_index, rev), params)
        ctx.cfg = (acts, drops, reduce, residual, nlayers)
        return node, H

    @staticmethod
    def backward(ctx, dnode, dH):
        acts, drops, reduce, residual, nlayers = ctx.cfg
        (Xv, Xe, edge_index, rev), params, _, _ = _saved_block(ctx, 4)
        need = ctx.needs_input_grad
        nfix = LayerwiseBlockFunction.NFIX
        dev = Xv.device
        with torch.enable_grad(), torch.random.fork_rng(devices=[dev]):
            torch.set_rng_state(ctx.rng[0])
            torch.cuda.set_rng_state(ctx.rng[1], dev)
            Xv_ = Xv.detach().requires_grad_(need[0])
            Xe_ = Xe.detach().requires_grad_(need[1])
            ps = [None if p is None else p.detach().requires_grad_(True) for p in params[:2 * nlayers]]
            # activation parameters: the module's own tensors (the recompute calls the modules)
            aps = [p if p is not None and need[nfix + 2 * nlayers + i] else None
                   for i, p in enumerate(params[2 * nlayers:])]
            node, H = _torch_block(Xv_, Xe_, edge_index, rev, ps[:nlayers], ps[nlayers:], [a[0] for a in acts],
                                   reduce, residual, _dropout_masks(drops, *Xe.shape, Xe))
            grads = _recompute_grads((node, H), (dnode, dH), [Xv_, Xe_, *ps, *aps])
        return (*grads[:2], *([None] * (nfix - 2)), *grads[2:])


def _weight_grad(G: Tensor, A: Tensor, out_dtype: Optional[torch.dtype] = None) -> Tensor:
    """dW = G^T A (h x h, reduction over all E edges).  A single GEMM has only (h/32)(h/64) output
    tiles, far too few for 256 CUs, so the edge dimension is split k ways into a batched GEMM
    whose k partial products are then summed (split-K).  out_dtype float32 for bf16 G (an fp32 master
    weight under bf16 compute): the library's fp32 accumulators, not rounded to bf16; otherwise the k
    partials are summed in fp32 and rounded once."""
    E, h = G.shape
    k = min(64, E // 2048)
    wide = dict(out_dtype=out_dtype) if out_dtype is not None and out_dtype != G.dtype else {}
    if k < 2:
        return torch.mm(G.t(), A, **wide)
    rows = E // k
    Eb = rows * k
    parts = torch.bmm(G[:Eb].view(k, rows, h).transpose(1, 2), A[:Eb].view(k, rows, h), **wide)
    if wide:
        dW = parts.sum(0)
        if Eb < E:
            dW += torch.mm(G[Eb:].t(), A[Eb:], **wide)
    else:
        dW = parts.sum(0, dtype=torch.float32).to(G.dtype)
        if Eb < E:
            dW.addmm_(G[Eb:].t(), A[Eb:])
    return dW


def block_backward(dnode, dH, states, weights, src, dst, rev, lay, act, reduce, residual, V, need_x,
                   drop=None, H_last=None):
    """Kernel backward of block_forward (see csrc/backward.hip), fp32 or bf16 storage, every reduce, on
    the kernels backward_route picks: max / min aggregations send each gradient element to its arg
    (torch_scatter's scatter_max / scatter_min): H_last = the forward's H_d, for the final node
    scatter's arg.  Returns (dXv, dXe, [dW_l], [db_l])."""
    maxmin = reduce in ("max", "min")
    E, h = states[0][0].shape if states else (dH.shape if dH is not None else (rev.numel(), dnode.shape[1]))
    src_ptr, src_perm, rev_ptr, rev_perm = backward_layout(lay, src, rev, V, E)
    mean_ptr = lay.dst_ptr if reduce == "mean" else None
    d = len(weights)
    gdtype = dH.dtype if dH is not None else (dnode.dtype if dnode is not None else states[0][0].dtype)
    # G = dL/dH_d: the gather of dnode below writes it whole when H_d itself has no gradient (no
    # E x h zero fill to add it to)
    G = dH.contiguous() if dH is not None else None
    if G is None and dnode is None:
        G = torch.zeros(E, h, dtype=gdtype, device=src.device)
    # fp32: max|G| of the current G, raised by the kernel that writes G (the fp16-split kernels'
    # scale); None = unknown (nt_absmax computes it).  One zero-filled buffer for every layer's row.
    fp32 = gdtype == torch.float32
    gbuf = torch.zeros(d + 1, 2, dtype=torch.float32, device=src.device) if fp32 else None
    gmax_cur = None
    if dnode is not None:
        gmax_cur = None if gbuf is None else gbuf[d]
        g1 = None if gmax_cur is None else gmax_cur[1:2]
        if maxmin:  # chemprop.py:86 with scatter_max / scatter_min
            arg = K.segment_arg(H_last, lay.dst_ptr, lay.dst_perm, V, reduce)
            G = K.gather_rows_arg(dnode.contiguous(), dst, arg, base=G, amax=g1)
        else:
            G = K.gather_rows(dnode.contiguous(), dst, base=G, seg_ptr=mean_ptr, amax=g1)
    dWs: list = [None] * d
    dbs: list = [None] * d
    route = backward_route(V, E, h, gdtype)
    split = route.dW == "fk" or route.dA in ("plan", "fk_dense")  # an fp16-split kernel runs: it scales by max|G|
    for l in range(d - 1, -1, -1):
        H_l, S_l, am_l = states[l]
        W = weights[l].detach()
        # an fp32 master weight under bf16 compute (bf16 autocast): G and the states are bf16
        master = weights[l] if (gdtype == torch.bfloat16 and W.dtype == torch.float32) else None
        # dropout: the update's gradient is keep * G / (1 - p); the residual path keeps G
        Gu = G if drop is None else K.dropout_residual(G, drop[0], drop[1], dropout_offset(l, E, h))
        Gu = Gu.contiguous()
        gmax = gmax_cur if drop is None else None  # dropout rescales G: its max is taken afresh
        if split and gmax is None:
            gmax = torch.zeros(2, dtype=torch.float32, device=Gu.device)
            K.absmax(Gu, gmax[1:2])
        if route.dW in ("fk", "bf16x6"):
            am = None
            if route.dW == "fk":  # on the forward's bounds
                am = am_l if am_l.numel() == 2 else None
                if am is None:  # a forward path that did not keep the chain
                    am = torch.zeros(2, dtype=torch.float32, device=Gu.device)
                    K.absmax(H_l.contiguous(), am[0:1])
                    K.absmax(S_l.contiguous(), am[1:2])
            dWs[l], dbs[l] = K.weight_grad(Gu, H_l.contiguous(), S_l.contiguous(), src, rev, act=act,
                                           amax_G=None if am is None else gmax[1:2], amax_HS=am)
        elif route.dW == "bf16":
            dW32, db32 = K.weight_grad(Gu, H_l.contiguous(), S_l.contiguous(), src, rev, act=act)
            # in the parameter's dtype: an fp32 master weight (bf16 autocast) keeps the fp32 result
            dWs[l], dbs[l] = dW32.to(W.dtype), db32.to(W.dtype)
        else:
            A = K.dmpnn_message(H_l, S_l, src, rev, act=act)
            dWs[l] = _weight_grad(Gu, A, W.dtype)
            dbs[l] = Gu.sum(0) if master is None else Gu.sum(0, dtype=W.dtype)
            del A
        dap = dA_plan(lay, src, V, E, src_ptr, src_perm) if route.dA == "plan" else None
        if dap is not None:
            # the layer kernel's fused mode over the src-sorted plan (A[e] = G[e]: rev = -1 everywhere, so
            # act and H are never applied)
            plan3, dmax, zf, ident, none, rt = dap
            # gmax = (0, max|G|): [0] is never written (the bound of the H term, absent here), so the
            # split scale is dense_matmul's
            dS = (torch.zeros if zf else torch.empty)(V, h, dtype=Gu.dtype, device=Gu.device)
            dA, dS = K.dmpnn_update_fused(Gu, Gu, ident, none, packed_transpose(weights[l]), None,
                                          residual=False, act=_RELU, plan=plan3, tile_rows=64, max_in_degree=dmax,
                                          perm=src_perm, reduce="sum", agg_act=_IDENTITY, amax_in=gmax,
                                          row_table=rt, S_out=dS, n_nodes=V)
        else:
            if route.dA in ("plan", "fk_dense"):
                dA = K.dense_matmul(Gu, packed_transpose(weights[l]), amax=gmax)
            elif route.dA == "bf16_dense":
                # an fp32 master weight: the W^T image the forward's pack launch wrote
                dA = K.dense_matmul(Gu, K.pack_weights(W.t().contiguous()) if master is None
                                    else packed_transpose(master, bf16=True))
            else:
                dA = torch.mm(Gu, W if master is None else W.to(Gu.dtype))
            dS = K.segment_reduce(dA, src_ptr, src_perm, V, reduce="sum", act=_IDENTITY)
        del Gu
        gmax_cur = gbuf[l - 1] if fp32 and l > 0 else None
        g1 = None if gmax_cur is None else gmax_cur[1:2]
        if maxmin:  # chemprop.py:39 with scatter_max / scatter_min: the arg of act(H_l) per node
            arg = K.segment_arg(H_l, lay.dst_ptr, lay.dst_perm, V, reduce, act=act)
            G = K.dmpnn_edge_backward_arg(G, H_l, dA, dS, arg, dst, rev_ptr, rev_perm,
                                          residual=residual, act=act, amax=g1)
        else:
            G = K.dmpnn_edge_backward(G, H_l, dA, dS, dst, rev_ptr, rev_perm, lay.dst_ptr,
                                      residual=residual, act=act, reduce=reduce, amax=g1)
    dXv = K.segment_reduce(G, src_ptr, src_perm, V, reduce="sum", act=_IDENTITY) if need_x[0] else None
    return dXv, G if need_x[1] else None, dWs, dbs


def _low_precision(bf16_compute: bool):
    """(dtype the torch recompute runs in, or None for the leaves' own; the context it runs under): under
    bf16 compute on the rounded copies, outside autocast."""
    if bf16_compute:
        return torch.bfloat16, torch.autocast("cuda", enabled=False)
    return None, contextlib.nullcontext()


class ChempropBlockFunction(torch.autograd.Function):
    """Kernel forward; kernel backward (block_backward: gather / scatter / element-wise HIP kernels and
    the MFMA dA / dW kernels) for every reduce in fp32 and bf16 storage; NT_BWD=torch selects the
    recompute-in-torch-device-ops backward (an A/B reference only).
    bf16_compute (the block under bf16 autocast): fp32 inputs and parameters are rounded once to bf16
    inside the kernels that read them, the bf16 kernel sequence runs, and every leaf's gradient comes
    back in the leaf's dtype: an fp32 weight or bias gets the weight-gradient kernel's fp32 dW / db
    as they are, fp32 Xv / Xe the bf16 gradient widened.  The NT_BWD=torch recompute then runs on the
    rounded copies and widens its results."""

    NFIX = 12  # inputs ahead of the layer parameters

    @staticmethod
    def forward(ctx, Xv, Xe, edge_index, rev, lay, act_mod, act, reduce, residual, nlayers, drop, bf16_compute,
                *params):
        src = edge_index[0].contiguous()
        kernel_bwd = (reduce in ("sum", "mean", "max", "min") and Xv.dtype in (torch.float32, torch.bfloat16)
                      and os.environ.get("NT_BWD", "kernel") != "torch")
        node, H, states = block_forward(Xv, Xe, src, rev, lay, list(params[:nlayers]), list(params[nlayers:]), act,
                                        reduce, residual, keep_states=kernel_bwd, drop=drop,
                                        bf16_compute=bf16_compute)
        _save_block(ctx, (Xv, Xe, edge_index, rev), params, states,
                    H if kernel_bwd and reduce in ("max", "min") else None)
        ctx.cfg = (act_mod, act, reduce, residual, nlayers, lay, kernel_bwd, drop, bf16_compute)
        # an output the loss does not use arrives as None instead of an E x h zero tensor: the backward
        # then writes G = dnode[dst] whole (no zero fill, no zero base read by the gather)
        ctx.set_materialize_grads(False)
        return node, H

    @staticmethod
    def backward(ctx, dnode, dH):
        act_mod, act, reduce, residual, nlayers, lay, kernel_bwd, drop, bf16_compute = ctx.cfg
        (Xv, Xe, edge_index, rev), params, states, H_last = _saved_block(ctx, 4)
        need = ctx.needs_input_grad
        nfix = ChempropBlockFunction.NFIX
        if dnode is None and dH is None:  # set_materialize_grads(False): neither output reached the loss
            return (None,) * (nfix + len(params))
        if kernel_bwd:
            dXv, dXe, dWs, dbs = block_backward(
                dnode, dH, states, params[:nlayers], edge_index[0].contiguous(), edge_index[1].contiguous(), rev,
                lay, act, reduce, residual, Xv.shape[0], (need[0], need[1]), drop, H_last,
            )
            if bf16_compute:  # fp32 features: the bf16 gradient widened
                dXv = None if dXv is None else dXv.to(Xv.dtype)
                dXe = None if dXe is None else dXe.to(Xe.dtype)
            return (dXv, dXe, *([None] * (nfix - 2)), *_param_grads(dWs, dbs, params, need, nfix, nlayers))
        low, ctxmgr = _low_precision(bf16_compute)
        with torch.enable_grad(), ctxmgr:
            Xv_ = Xv.detach().to(low or Xv.dtype).requires_grad_(need[0])
            Xe_ = Xe.detach().to(low or Xe.dtype).requires_grad_(need[1])
            ps = [None if p is None else p.detach().to(low or p.dtype).requires_grad_(True) for p in params]
            node, H = _torch_block(Xv_, Xe_, edge_index, rev, ps[:nlayers], ps[nlayers:], [act_mod] * nlayers,
                                   reduce, residual, _dropout_masks([drop] * nlayers, *Xe.shape, Xe_))
            grads = _recompute_grads((node, H), (dnode, dH), [Xv_, Xe_, *ps])
        if low is not None:  # each result in its leaf's dtype
            grads = [None if g is None else g.to(x.dtype) for g, x in zip(grads, (Xv, Xe, *params))]
        return (*grads[:2], *([None] * (nfix - 2)), *grads[2:])


def _grad_rows(g: Tensor) -> Tensor:
    """A gradient as rows nt_embed_bag_backward reads: contiguous, or a row-padded view."""
    if g.is_contiguous() or (g.dim() == 2 and g.stride(1) == 1 and g.stride(0) >= g.shape[1]):
        return g
    return g.contiguous()


class EmbedBagFunction(torch.autograd.Function):
    """One sum-mode EmbeddingBag on the kernels: nt_embed_bag forward, nt_embed_bag_backward (the
    deterministic LDS reduction, no CSR) for the table gradient."""

    @staticmethod
    def forward(ctx, table, idx, validate):
        ctx.save_for_backward(idx)
        ctx.table = (table.shape[0], table.dtype)
        ctx.set_materialize_grads(False)
        return K.embed_bag(table.detach(), idx, validate=validate)

    @staticmethod
    def backward(ctx, dX):
        if dX is None or not ctx.needs_input_grad[0]:
            return None, None, None
        (idx,) = ctx.saved_tensors
        ntypes, dtype = ctx.table
        return K.embed_bag_backward(_grad_rows(dX), idx, ntypes, out_dtype=dtype), None, None


class EmbeddedBlockFunction(torch.autograd.Function):
    """The embedded encoder (GraphEmbedding fused into the block's initial gather) under autograd.
    Forward: block_forward_embedded's kernels with the layer states kept.  Backward: block_backward
    down to G = dL/dH0 (dXv is never reduced), then nt_embed_bag_backward twice over G: the edge table
    from (G, edge_types), the node table from (G, node_types) through the src CSR.  A table or parameter
    that needs no gradient gets None and no launch.  NT_BWD=torch: the recompute-in-torch backward of
    the unfused pair (A/B reference only).  bf16_compute (bf16 autocast): fp32 tables enter through
    nt_dmpnn_init_embed_mixed, the bf16 kernels run, fp32 tables receive nt_embed_bag_backward's fp32
    output and fp32 weights / biases the weight-gradient kernel's fp32 dW / db."""

    NFIX = 15  # inputs ahead of the layer parameters

    @staticmethod
    def forward(ctx, node_table, edge_table, node_types, edge_types, edge_index, rev, lay, act_mod, act, reduce,
                residual, nlayers, drop, validate, bf16_compute, *params):
        kernel_bwd = os.environ.get("NT_BWD", "kernel") != "torch"
        node, H, states = block_forward_embedded(
            node_table.detach(), node_types, edge_table.detach(), edge_types, edge_index[0].contiguous(), rev, lay,
            list(params[:nlayers]), list(params[nlayers:]), act, reduce, residual, keep_states=kernel_bwd,
            drop=drop, validate=validate, bf16_compute=bf16_compute)
        _save_block(ctx, (node_table, edge_table, node_types, edge_types, edge_index, rev), params, states,
                    H if kernel_bwd and reduce in ("max", "min") else None)
        ctx.cfg = (act_mod, act, reduce, residual, nlayers, lay, kernel_bwd, drop, bf16_compute)
        ctx.set_materialize_grads(False)  # an unused output arrives as None (see ChempropBlockFunction)
        return node, H

    @staticmethod
    def backward(ctx, dnode, dH):
        act_mod, act, reduce, residual, nlayers, lay, kernel_bwd, drop, bf16_compute = ctx.cfg
        (node_table, edge_table, node_types, edge_types, edge_index, rev), params, states, H_last = \
            _saved_block(ctx, 6)
        nfix = EmbeddedBlockFunction.NFIX
        need = ctx.needs_input_grad
        if dnode is None and dH is None:
            return (None,) * (nfix + len(params))
        V, E = node_types.shape[0], edge_types.shape[0]
        if kernel_bwd:
            src = edge_index[0].contiguous()
            _, G, dWs, dbs = block_backward(dnode, dH, states, params[:nlayers], src, edge_index[1].contiguous(),
                                            rev, lay, act, reduce, residual, V, (False, need[0] or need[1]), drop,
                                            H_last)
            dTv = dTe = None
            if need[1]:
                dTe = K.embed_bag_backward(_grad_rows(G), edge_types, edge_table.shape[0],
                                           out_dtype=edge_table.dtype)
            if need[0]:  # R[v] = sum of G over v's out-edges (dXv), formed inside the reduction
                src_ptr, src_perm = backward_layout(lay, src, rev, V, E)[:2]
                dTv = K.embed_bag_backward(_grad_rows(G), node_types, node_table.shape[0], src_ptr, src_perm,
                                           out_dtype=node_table.dtype)
            return (dTv, dTe, *([None] * (nfix - 2)), *_param_grads(dWs, dbs, params, need, nfix, nlayers))
        low, ctxmgr = _low_precision(bf16_compute)
        with torch.enable_grad(), ctxmgr:
            tv = node_table.detach().requires_grad_(need[0])
            te = edge_table.detach().requires_grad_(need[1])
            Xv_ = torch.nn.functional.embedding_bag(node_types, tv, mode="sum").to(low or tv.dtype)
            Xe_ = torch.nn.functional.embedding_bag(edge_types, te, mode="sum").to(low or te.dtype)
            ps = [None if p is None else p.detach().to(low or p.dtype).requires_grad_(True) for p in params]
            node, H = _torch_block(Xv_, Xe_, edge_index, rev, ps[:nlayers], ps[nlayers:], [act_mod] * nlayers,
                                   reduce, residual, _dropout_masks([drop] * nlayers, E, edge_table.shape[1], Xe_))
            grads = _recompute_grads((node, H), (dnode, dH), [tv, te, *ps])
        if low is not None:  # each parameter's result in its leaf's dtype (the tables' already are)
            grads[2:] = [None if g is None else g.to(p.dtype) for g, p in zip(grads[2:], params)]
        return (*grads[:2], *([None] * (nfix - 2)), *grads[2:])


def segment_reduce_readout(X: Tensor, mol_ptr: Tensor, mol_perm: Optional[Tensor], B: int, reduce: str,
                           batch_node_index: Tensor, chunks=None) -> Tensor:
    if torch.is_grad_enabled() and X.requires_grad:
        return ReadoutFunction.apply(X, mol_ptr, mol_perm, B, reduce, batch_node_index, chunks)
    return _aggregate(X, mol_ptr, mol_perm, B, reduce, _IDENTITY, chunks)


class ReadoutFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, mol_ptr, mol_perm, B, reduce, batch_node_index, chunks=None):
        ctx.save_for_backward(X, batch_node_index)
        ctx.cfg = (B, reduce, mol_ptr)
        ctx.mol_perm = mol_perm
        return _aggregate(X, mol_ptr, mol_perm, B, reduce, _IDENTITY, chunks)

    @staticmethod
    def backward(ctx, dout):
        X, bni = ctx.saved_tensors
        B, reduce, mol_ptr = ctx.cfg
        if reduce in ("sum", "mean") and dout.dtype in (torch.float32, torch.bfloat16):
            # dX[v] = dout[batch v] (/ count for mean): one gather kernel
            dX = K.gather_rows(dout.contiguous(), bni, seg_ptr=mol_ptr if reduce == "mean" else None)
            return dX, None, None, None, None, None, None
        if reduce in ("max", "min") and dout.dtype in (torch.float32, torch.bfloat16):
            # agg.py:45 scatter_max: dX[v] = dout[batch v] where v is the molecule's arg
            mol_perm = ctx.mol_perm
            arg = K.segment_arg(X.contiguous(), mol_ptr, mol_perm, B, reduce)
            dX = K.gather_rows_arg(dout.contiguous(), bni, arg)
            return dX, None, None, None, None, None, None
        with torch.enable_grad():
            X_ = X.detach().requires_grad_(True)
            out = _torch_scatter(X_, bni, B, reduce)
            (dX,) = torch.autograd.grad(out, X_, dout)
        return dX, None, None, None, None, None, None
