"""Packed-weight cache: the MFMA fragment image of a parameter is re-derived only when the parameter
changes (torch bumps Tensor._version on every in-place update, e.g. optimizer.step(), and a new
storage changes data_ptr), so inference forwards reuse it and training forwards repack after every
step.  Keyed by id() with a weakref check: tensors cannot be WeakKeyDictionary keys because their
__eq__ is element-wise."""
from __future__ import annotations

import weakref
from dataclasses import dataclass
from typing import Iterable, Iterator, Optional, Sequence

import torch
from torch import Tensor

from notorch_amd import kernels as K


@dataclass(eq=False, slots=True)
class _Packed:
    """The images of one parameter, side by side, all dropped when its key changes."""
    ref: weakref.ref
    key: tuple
    fk: Optional[Tensor] = None  # the image of the parameter's own dtype (fp32: the fk image)
    fkT: Optional[Tensor] = None  # that of W^T
    # an fp32 parameter under bf16 autocast: the bf16 image, the bf16 image of W^T and the bf16 copy of
    # its layer's bias as (weakref, key, copy)
    bf: Optional[Tensor] = None
    bfT: Optional[Tensor] = None
    bias: Optional[tuple] = None


_PACKED: dict[int, _Packed] = {}


def _param_key(W: Tensor) -> tuple:
    return (W.data_ptr(), W._version, tuple(W.shape), W.device)


def _entry(W: Tensor) -> _Packed:
    """The cache entry of parameter W, emptied if W changed since it was made."""
    wid = id(W)
    key = _param_key(W)
    hit = _PACKED.get(wid)
    if hit is None or hit.ref() is not W or hit.key != key:
        ref = weakref.ref(W, lambda _r, wid=wid: _PACKED.pop(wid, None))
        hit = _PACKED[wid] = _Packed(ref, key)
    return hit


def _pack_chunks(items: Iterable[tuple]) -> Iterator[list]:
    """One list per pack launch: the items (tuples led by their weight) of distinct weights, grouped by
    (h, device), in chunks of at most 16."""
    groups: dict = {}
    seen = set()
    for it in items:
        W = it[0]
        if id(W) not in seen:
            seen.add(id(W))
            groups.setdefault((W.shape[0], W.device), []).append(it)
    for ws in groups.values():
        for c in range(0, len(ws), 16):
            yield ws[c:c + 16]


def _multi_packable(W: Tensor) -> bool:
    """fp32 weights whose image is the fk image alone (h % 4 == 0): packed in one launch pair for all
    layers (nt_dmpnn_pack_weights_fk), with the backward's W^T image alongside."""
    return W.dtype == torch.float32 and W.dim() == 2 and W.shape[0] % 4 == 0 and W.is_contiguous()


def pack_layer_weights(weights: Sequence[Tensor], with_t: bool = False) -> list[Tensor]:
    """One packed MFMA image per layer; shared layers (same tensor) are packed once.  with_t (a
    training forward, fp32): the images of W^T too (packed_transpose), from the same launch pair."""
    out: list = [None] * len(weights)
    stale = []  # (index, W) needing a pack
    for i, W in enumerate(weights):
        hit = _entry(W)
        if hit.fk is None or (with_t and hit.fkT is None):
            stale.append((i, W))
        else:
            out[i] = hit.fk
    for chunk in _pack_chunks((W,) for _, W in stale if _multi_packable(W)):
        imgs, imgsT = K.pack_weights_fk_multi([W.detach() for (W,) in chunk], with_t=with_t)
        for j, (W,) in enumerate(chunk):
            hit = _entry(W)
            hit.fk, hit.fkT = imgs[j], None if imgsT is None else imgsT[j]
    for i, W in stale:
        hit = _entry(W)
        if not _multi_packable(W):
            hit.fk, hit.fkT = K.pack_weights(W.detach()), None
        out[i] = hit.fk
    return out


def _bias_copy(hit: _Packed, b: Tensor) -> Optional[Tensor]:
    """The cached bf16 copy of fp32 bias b in its weight's entry, if b is unchanged since."""
    c = hit.bias
    if c is not None and c[0]() is b and c[1] == _param_key(b):
        return c[2]
    return None


def pack_layer_weights_bf16(weights: Sequence[Tensor], biases: Sequence[Optional[Tensor]],
                            with_t: bool = False) -> tuple[list[Tensor], list[Optional[Tensor]]]:
    """bf16 compute of a block whose parameters may be fp32 master weights (bf16 autocast): per layer
    the bf16 fragment image and the bf16 bias.  An fp32 weight's image, with_t (a training forward)
    the image of its W^T for the backward's dA, and the bf16 copy of its fp32 bias come from ONE
    nt_dmpnn_pack_weights_mixed launch for all stale layers (chunks of 16 distinct weights; a shared
    layer is packed once) and are cached beside the parameter's fp32 image.  A bf16 parameter is
    used as it is (the bf16 path's own packing)."""
    d = len(weights)
    stale = []  # (W, fp32 bias or None) needing a pack
    for W, b in zip(weights, biases):
        if W.dtype != torch.float32:
            continue
        hit = _entry(W)
        b32 = b if (b is not None and b.dtype == torch.float32) else None
        if (hit.bf is None or (with_t and hit.bfT is None)
                or (b32 is not None and _bias_copy(hit, b32) is None)):
            stale.append((W, b32))
    for chunk in _pack_chunks(stale):
        imgs, imgsT, b16 = K.pack_weights_mixed([W.detach().contiguous() for W, _ in chunk],
                                                [None if b is None else b.detach().contiguous()
                                                 for _, b in chunk], with_t=with_t)
        for j, (W, b32) in enumerate(chunk):
            hit = _entry(W)
            hit.bf = imgs[j]
            if imgsT is not None:
                hit.bfT = imgsT[j]
            if b32 is not None:
                hit.bias = (weakref.ref(b32), _param_key(b32), b16[j])
    Wps: list = [None] * d
    bs: list = [None] * d
    for i, (W, b) in enumerate(zip(weights, biases)):
        Wps[i] = _entry(W).bf if W.dtype == torch.float32 else pack_layer_weights([W])[0]
        if b is None:
            continue
        if b.dtype == torch.bfloat16:
            bs[i] = b.detach()
        else:  # the copy packed with its weight; a bias that is not its weight's own is cast by torch
            c = _bias_copy(_entry(W), b) if W.dtype == torch.float32 else None
            bs[i] = c if c is not None else b.detach().to(torch.bfloat16)
    return Wps, bs


def packed_transpose(W: Tensor, bf16: bool = False) -> Tensor:
    """The fk image of W^T (the backward's dA = G W): the one the training forward packed beside W's
    if W is unchanged since, else packed now.  bf16 (an fp32 master weight under bf16 compute): the
    bf16 image of W^T, likewise."""
    hit = _entry(W)
    if bf16:
        if hit.bfT is None:
            imgs, imgsT, _ = K.pack_weights_mixed([W.detach().contiguous()], None, with_t=True)
            hit.bf, hit.bfT = imgs[0], imgsT[0]
        return hit.bfT
    if hit.fkT is not None:
        return hit.fkT
    return K.pack_weights(W.detach().t().contiguous(), fk_only=True)
