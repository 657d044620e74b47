"""CPU: which launches a block takes (_engine.forward_route / backward_route) and the layout's cache
helper (_layout._cached).  Every input of a route is an integer, a dtype, a module knob or an environment
variable; the library is loaded only for K.fused_tile_rows.  The expectations are the dispatch rules
as they stood inline in _layers_forward / block_backward before the routes were extracted."""
import dataclasses

import pytest
import torch

from notorch_amd import kernels as K
from notorch_amd._lib import NT_ACT_IDENTITY, NT_ACT_RELU
from notorch_amd.data.models.graph import DeviceLayout
from notorch_amd.nn.gnn import _engine, _layout

F32, BF16 = torch.float32, torch.bfloat16
RELU, IDENTITY = (NT_ACT_RELU, 0.0), (NT_ACT_IDENTITY, 0.0)
DROP = (0.25, 1)
V, E = 10, 20
NO_PLAN = (False, "update")  # no plan asked for: the plain update (+ dropout_residual under dropout)


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for name in ("NT_FUSED", "NT_FUSED_DROPOUT", "NT_FK_NW", "NT_WGRAD", "NT_BF16_DA"):
        monkeypatch.delenv(name, raising=False)
    for name, value in (("BF16_FUSED_PIECE4", True), ("BF16_FUSED_DROPOUT_MAX_H", 512), ("BF16_WGRAD_MAX_H", 2048),
                        ("FP32_WGRAD_FK_MAX_H", 4096), ("NW4_MAX_EDGES", 131072), ("_FUSED_DA", True)):
        monkeypatch.setattr(_engine, name, value)


def cap(h, dtype):
    return min(K.fused_tile_rows(h, dtype, RELU, "sum", RELU), K.fused_tile_rows(h, dtype, RELU, "sum", IDENTITY))


def fwd(h, dtype, drop=None, E=E):
    return _engine.forward_route(V, E, h, dtype, RELU, "sum", drop)


def asked(route):
    return route.plan, route.fallback


def test_fp32_plan_and_tile_rows(monkeypatch):
    c = cap(300, F32)
    r = fwd(300, F32)
    assert r.plan and not r.dropout and r.fallback == "persistent"
    assert r.rows == (64 if c == 128 else c)  # E = 20 <= NW4_MAX_EDGES
    assert fwd(300, F32, E=_engine.NW4_MAX_EDGES + 1).rows == c
    monkeypatch.setattr(_engine, "NW4_MAX_EDGES", 0)
    assert fwd(300, F32).rows == c
    monkeypatch.setattr(_engine, "NW4_MAX_EDGES", 131072)
    monkeypatch.setenv("NT_FK_NW", "8")
    assert fwd(300, F32).rows == c


def test_fp32_64_row_override_stops_at_320():
    assert fwd(320, F32).rows == (64 if cap(320, F32) == 128 else cap(320, F32))
    for edges in (E, 10**6):
        r = fwd(324, F32, E=edges)
        assert r.plan and r.rows == cap(324, F32)


def test_fp32_unsupported_size_takes_the_plain_update():
    assert not K.fused_supported(V, E, 302, F32)
    assert asked(fwd(302, F32)) == NO_PLAN
    assert asked(fwd(302, F32, DROP)) == NO_PLAN


def test_fp32_dropout(monkeypatch):
    r = fwd(300, F32, DROP)
    # in the launch; should fused_plan have none, the plain update + dropout_residual, not the persistent kernel
    assert r.plan and r.dropout and r.fallback == "update"
    assert r.rows == fwd(300, F32).rows
    monkeypatch.setenv("NT_FUSED_DROPOUT", "0")
    r = fwd(300, F32, DROP)
    assert asked(r) == NO_PLAN and not r.dropout
    assert fwd(300, F32).plan  # the switch is about dropout only


def test_bf16_piece4(monkeypatch):
    r = fwd(300, BF16)
    assert r.plan and r.rows == cap(300, BF16) and r.fallback == "update"  # never the persistent kernel
    monkeypatch.setattr(_engine, "BF16_FUSED_PIECE4", False)
    assert asked(fwd(300, BF16)) == NO_PLAN
    assert fwd(304, BF16).plan


def test_bf16_dropout(monkeypatch):
    assert asked(fwd(300, BF16, DROP)) == NO_PLAN  # h % 8 == 4 has no dropout instances
    r = fwd(512, BF16, DROP)
    assert r.plan and r.dropout and r.rows == 64 and r.fallback == "update"
    assert asked(fwd(520, BF16, DROP)) == NO_PLAN
    assert fwd(520, BF16).plan
    monkeypatch.setattr(_engine, "BF16_FUSED_DROPOUT_MAX_H", 8192)
    r = fwd(520, BF16, DROP)
    assert r.plan and r.dropout and r.rows == 64


def test_bf16_piece4_stops_at_512():
    assert asked(fwd(516, BF16)) == NO_PLAN
    assert asked(fwd(516, BF16, DROP)) == NO_PLAN


@pytest.mark.parametrize("h,dtype,drop", [(300, F32, None), (300, F32, DROP), (304, BF16, None), (512, BF16, DROP)])
def test_nt_fused_0_asks_for_no_plan(monkeypatch, h, dtype, drop):
    assert fwd(h, dtype, drop).plan
    monkeypatch.setenv("NT_FUSED", "0")
    assert asked(fwd(h, dtype, drop)) == NO_PLAN


# (dtype, h, E, environment, module knobs) -> (dW, dA)
BACKWARD = [
    (F32, 300, E, {}, {}, ("fk", "plan")),
    (F32, 302, E, {}, {}, ("fk", "mm")),  # h <= 320; K.fused_supported is false
    (F32, 322, E, {}, {}, ("bf16x6", "mm")),
    (F32, 4096, E, {}, {}, ("fk", "plan")),
    (F32, 4100, E, {}, {}, ("bf16x6", "plan")),
    (F32, 300, E, {"NT_WGRAD": "kernel6"}, {}, ("bf16x6", "plan")),
    (F32, 302, E, {"NT_WGRAD": "kernel6"}, {}, ("bf16x6", "mm")),
    (F32, 300, E, {"NT_WGRAD": "library"}, {}, ("library", "plan")),
    (F32, 322, E, {"NT_WGRAD": "library"}, {}, ("library", "mm")),
    (F32, 300, E, {}, {"_FUSED_DA": False}, ("fk", "fk_dense")),
    (F32, 4100, E, {}, {"_FUSED_DA": False}, ("bf16x6", "fk_dense")),
    (F32, 302, E, {}, {"_FUSED_DA": False}, ("fk", "mm")),
    (BF16, 304, E, {}, {}, ("bf16", "bf16_dense")),
    (BF16, 2048, E, {}, {}, ("bf16", "bf16_dense")),
    (BF16, 4096, E, {}, {}, ("library", "bf16_dense")),
    (BF16, 300, E, {}, {}, ("library", "mm")),
    (BF16, 36, E, {}, {}, ("library", "mm")),
    (BF16, 304, E, {"NT_WGRAD": "library"}, {}, ("library", "mm")),
    (BF16, 304, E, {"NT_BF16_DA": "torch"}, {}, ("bf16", "mm")),
    (BF16, 304, 2**31, {}, {}, ("library", "mm")),
]


@pytest.mark.parametrize("dtype,h,edges,env,knobs,want", BACKWARD)
def test_backward_route(monkeypatch, dtype, h, edges, env, knobs, want):
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    for name, value in knobs.items():
        monkeypatch.setattr(_engine, name, value)
    assert tuple(_engine.backward_route(V, edges, h, dtype)) == want


def test_backward_thresholds_are_read_at_call_time(monkeypatch):
    monkeypatch.setattr(_engine, "FP32_WGRAD_FK_MAX_H", 320)
    assert _engine.backward_route(V, E, 4096, F32).dW == "bf16x6"
    monkeypatch.setattr(_engine, "BF16_WGRAD_MAX_H", 8192)
    assert _engine.backward_route(V, E, 4096, BF16).dW == "bf16"


# ------------------------------------------------------------------------------------ _cached
LAZY = ("zero_rows", "hub_runs", "hub_chunk_ids", "da_plan", "embed_checked", "bwd", "row_table", "embed_records")


def test_cached_builds_once_per_key_and_pin():
    lay = DeviceLayout()
    built = []

    def build():
        built.append(1)
        return len(built)

    pin, other = torch.zeros(1), torch.zeros(1)
    assert _layout._cached(lay, "row_table", (1, 2), build, pin) == 1
    assert _layout._cached(lay, "row_table", (1, 2), build, pin) == 1  # same key, same pin
    assert _layout._cached(lay, "row_table", (1, 3), build, pin) == 2  # a changed key
    assert _layout._cached(lay, "row_table", (1, 3), build, other) == 3  # an equal key, another pinned object
    assert _layout._cached(lay, "row_table", (1, 3), build, other) == 3
    assert _layout._cached(lay, "bwd", (1, 3), build, other) == 4  # two names on one layout do not collide
    assert _layout._cached(lay, "row_table", (1, 3), build, other) == 3
    assert _layout._cached(lay, "zero_rows", (), build) == 5  # no pin, an empty key
    assert _layout._cached(lay, "zero_rows", (), build) == 5
    assert len(built) == 5


def test_cached_keeps_a_false_value():
    lay, built = DeviceLayout(), []
    for _ in range(2):
        assert _layout._cached(lay, "mol_chunks", (), lambda: built.append(1) or False, lay) is False
    assert len(built) == 1


def test_layout_declares_what_the_engine_sets_and_a_copy_carries_none_of_it():
    names = {f.name for f in dataclasses.fields(DeviceLayout)}
    assert set(LAZY) <= names
    lay = DeviceLayout()
    for name in LAZY:
        setattr(lay, name, (None, "built"))
    moved = lay.map_tensors(lambda t: t, None, None)
    assert all(getattr(moved, name) is None for name in LAZY)
