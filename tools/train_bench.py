"""Training-step timing of ChempropBlock + Sum readout at config 2 (or config 3 with --kind zinc
--h 512 --depth 5 --dtype bf16), as the reference trains: zero_grad, forward, backward and an
Adam(lr=1e-4) step (notorch/lightning_models/model.py:153 optim_factory, :224-241 training_step,
:273 configure_optimizers; Lightning calls optimizer.step() every batch).  The step after the
optimizer sees new weights, so the forward re-packs them (one pack per layer weight).

Modes: `kernel` (the kernel backward, the weight grad per NT_WGRAD) and `torch` (the
recompute-in-torch backward, NT_BWD=torch).  bench.py's `training` key runs this in fresh processes
with --json (the default weight-grad path as the headline, NT_WGRAD=library as a comparison).
--embedded trains the model users train, EmbeddedChempropBlock (GraphEmbedding fused into the block) + Sum,
from the collated integer type indices: both embedding tables are in the optimizer and there are no
Xv / Xe leaves.  --embed-bwd kernel (default) is the kernel path (EmbeddedBlockFunction: fused init,
nt_embed_bag_backward for the tables); --embed-bwd torch is the library path that preceded it
(block(embedding(G)) with nn.EmbeddingBag under autograd, NT_EMBED_BWD=torch).
--autocast (with --dtype f32) is mixed precision as Lightning's precision="bf16-mixed" runs it: the
module, its gradients and the Adam state stay fp32, and the forward and the loss of every step run
inside torch.autocast("cuda", dtype=torch.bfloat16), so the block computes on the bf16 kernels.
--dropout P trains with nn.Dropout(P) in every layer's update (the fwd row is then a train()-mode
forward under no_grad: it drops too).  By default the layer kernel applies the mask in its epilogue
(nt_dmpnn_update_fused_dropout); NT_FUSED_DROPOUT=0 in the environment is the A/B: the unfused update,
nt_dropout_residual and a separate segment reduce.  With --dropout the JSON also carries the layer
launch the forward took and its median time (the engine's event pair around every layer launch: on
the unfused path it spans the update and the dropout kernel, not the segment reduce that follows).
--readout gated trains a Gated attention readout (its fp32 a.weight / a.bias in the optimizer) in place of
Sum; with --autocast it runs inside the region on the block's bf16 node_feats (nt_node_scores_mixed,
nt_softmax_pool_backward_mixed).  --readout gated-f32 is the A/B for that: node_feats widened to fp32 by
torch and the readout on the fp32 kernels outside the region, what mixed precision had to run before.
--loss mse|mve|evidential closes the step with a task head and a real loss in place of out.pow(2).sum(): an
nn.Linear(h, tasks * c) on the readout (c = 1, 2, 4; softplus on the variance-like channels: v + 0.1,
alpha + 1, beta + 0.1), then notorch_amd.nn.loss.MSE / MVE / Evidential against fixed randn targets.  The head
is in the optimizer.  The loss takes the kernel (nt_task_loss, one launch for loss and gradient) or, with
NT_LOSS=torch in the environment, torch ops under autograd; the JSON names the route.
The table and the JSON also report torch.cuda.max_memory_allocated over the timed steps.
Usage: python tools/train_bench.py [--kind qm9] [--mols 4096] [--h 300] [--depth 3] [--dtype f32|bf16]
                                  [--steps 30] [--warmup 10] [--warmup-s 0] [--modes kernel,torch]
                                  [--optim adam|none] [--embedded [--embed-bwd kernel|torch]] [--autocast]
                                  [--dropout P] [--readout sum|gated|gated-f32]
                                  [--loss mse|mve|evidential [--tasks 1]] [--json]"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from notorch_amd.data.synth import make_batch  # noqa: E402
from notorch_amd.nn import ChempropBlock, EmbeddedChempropBlock, Gated, GraphEmbedding, Sum  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--kind", default="qm9")
    p.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    p.add_argument("--mols", type=int, default=4096)
    p.add_argument("--seed", type=int, default=1000, help="batch seed (bench.py rank 0: 1000)")
    p.add_argument("--h", type=int, default=300)
    p.add_argument("--depth", type=int, default=3)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--warmup-s", type=float, default=0.0,
                   help="after the counted warm-ups, keep warming up until this many seconds have passed "
                        "(lets the clocks settle in a fresh process)")
    p.add_argument("--modes", default="kernel,torch")
    p.add_argument("--optim", default="adam", choices=["adam", "adam-fused", "none"],
                   help="adam: Adam(lr=1e-4).step() in every training step (the reference's default "
                        "optim_factory; torch's foreach implementation); adam-fused: the same optimizer "
                        "with torch's fused=True implementation; none: forward + backward only")
    p.add_argument("--embedded", action="store_true",
                   help="train EmbeddedChempropBlock + Sum from the type indices (the tables train; no Xv / Xe leaves)")
    p.add_argument("--embed-bwd", default="kernel", choices=["kernel", "torch"],
                   help="with --embedded: kernel = the fused kernel path; torch = block(embedding(G)) with "
                        "nn.EmbeddingBag under autograd (NT_EMBED_BWD=torch)")
    p.add_argument("--autocast", action="store_true",
                   help="fp32 module (--dtype f32) with the forward and the loss of every step inside "
                        "torch.autocast('cuda', dtype=torch.bfloat16): fp32 master weights, bf16 kernels")
    p.add_argument("--dropout", type=float, default=0.0,
                   help="dropout probability of every layer's update (training mode; NT_FUSED_DROPOUT=0 keeps "
                        "it off the fused layer launch)")
    p.add_argument("--readout", default="sum", choices=["sum", "gated", "gated-f32"],
                   help="sum: the Sum readout; gated: a trained Gated readout on the block's output as it is "
                        "(under --autocast: bf16 rows, fp32 keys, inside the region); gated-f32: the same readout "
                        "on node_feats.float(), outside the autocast region")
    p.add_argument("--loss", default=None, choices=["mse", "mve", "evidential"],
                   help="close the step with an nn.Linear(h, tasks * c) head and this loss (NT_LOSS=torch: the torch-ops "
                        "route) in place of out.pow(2).sum()")
    p.add_argument("--tasks", type=int, default=1, help="with --loss: the number of target columns t")
    p.add_argument("--json", action="store_true", help="print one JSON object instead of the table")
    a = p.parse_args()
    if a.autocast and a.dtype != "f32":
        p.error("--autocast trains an fp32 module: use --dtype f32")

    def region():
        return torch.autocast("cuda", dtype=torch.bfloat16) if a.autocast else contextlib.nullcontext()
    from notorch_amd import _lib

    _lib.load()  # fail loudly if the HIP extension is missing
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[a.dtype]
    G = make_batch(a.kind, a.mols, seed=a.seed).collate("nodes")
    torch.manual_seed(0)
    ro = Sum() if a.readout == "sum" else Gated(a.h).to("cuda", dt).train()
    E = G.num_edges
    if a.embedded:
        os.environ["NT_EMBED_BWD"] = a.embed_bwd
        Gd = G.to("cuda")  # node_feats / edge_feats stay the integer type columns
        blk = EmbeddedChempropBlock(GraphEmbedding(42, 13, a.h), ChempropBlock(a.h, depth=a.depth, dropout=a.dropout))
        blk = blk.to("cuda", dt).train()
    else:
        ev = torch.nn.EmbeddingBag(42, a.h, mode="sum")
        ee = torch.nn.EmbeddingBag(13, a.h, mode="sum")
        with torch.no_grad():
            Xv, Xe = ev(G.node_feats).to(dt), ee(G.edge_feats).to(dt)
        Gd = G.update(node_feats=Xv, edge_feats=Xe).to("cuda")
        blk = ChempropBlock(a.h, depth=a.depth, dropout=a.dropout).to("cuda", dt).train()
        Xv_d = Gd.node_feats.requires_grad_(True)
        Xe_d = Gd.edge_feats.requires_grad_(True)
    head = crit = None
    if a.loss:
        from notorch_amd.nn import loss as losses

        c = {"mse": 1, "mve": 2, "evidential": 4}[a.loss]
        head = torch.nn.Linear(a.h, a.tasks * c).to("cuda", dt).train()
        crit = {"mse": losses.MSE, "mve": losses.MVE, "evidential": losses.Evidential}[a.loss]()
        targets = torch.randn(a.mols, a.tasks, device="cuda")
        shift = torch.tensor([0.0, 0.1, 1.0, 0.1][:c], device="cuda")[1:]

    def task_loss(x):
        if head is None:
            return x.float().pow(2).sum()
        out = head(x).view(a.mols, a.tasks, -1)
        if out.shape[-1] == 1:
            return crit(out.squeeze(-1), targets)
        wide = torch.nn.functional.softplus(out[..., 1:]) + shift.to(out.dtype)
        return crit(torch.cat([out[..., :1], wide], -1), targets)

    opt = None
    if a.optim != "none":
        opt = torch.optim.Adam([*blk.parameters(), *ro.parameters(), *(head.parameters() if head else ())], lr=1e-4,
                               **({"fused": True} if a.optim == "adam-fused" else {}))

    def read(out):
        if a.readout != "gated-f32":
            return ro(out)
        with torch.autocast("cuda", enabled=False):
            return ro(out.update(node_feats=out.node_feats.float()))

    def step():
        blk.zero_grad(set_to_none=True)
        ro.zero_grad(set_to_none=True)
        if head is not None:
            head.zero_grad(set_to_none=True)
        with region():
            if a.embedded:
                out = blk(Gd)
            else:
                Xv_d.grad = Xe_d.grad = None
                out = blk(Gd.update(node_feats=Xv_d, edge_feats=Xe_d))
            loss = task_loss(read(out))
        loss.backward()
        if opt is not None:
            opt.step()

    def fwd():
        with torch.no_grad(), region():
            read(blk(Gd))

    res = {}
    mem = {}
    for mode in a.modes.split(","):
        os.environ["NT_BWD"] = mode
        for name, fn in (("fwd", fwd), (f"train[{mode}]", step)):
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            t_end = time.perf_counter() + a.warmup_s
            while time.perf_counter() < t_end:
                fn()
                torch.cuda.synchronize()
            # back-to-back steps as a training loop runs them (no host sync between steps, so the
            # host's autograd / optimizer bookkeeping overlaps the device work of the previous step):
            # rounds of `chunk` steps between two events, the median round per step
            ts = []
            torch.cuda.reset_peak_memory_stats()
            chunk = max(1, min(10, a.steps))
            for _ in range(max(1, a.steps // chunk)):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(chunk):
                    fn()
                e.record()
                e.synchronize()
                ts.append(s.elapsed_time(e) / chunk)
            res[name] = statistics.median(ts)
            mem[name] = torch.cuda.max_memory_allocated()
    layer = {}
    if a.dropout > 0:  # which layer launch the forward takes, and its median time
        from notorch_amd.nn.gnn import _engine

        _engine.UPDATE_EVENTS = evs = []
        for _ in range(10):
            fwd()
        torch.cuda.synchronize()
        _engine.UPDATE_EVENTS = None
        layer = {"dropout": a.dropout, "fused_dropout": os.environ.get("NT_FUSED_DROPOUT", "1") != "0",
                 "layer_kernel": _engine.LAST_UPDATE_INFO.get("kernel"),
                 "layer_us": statistics.median(s.elapsed_time(e) for s, e in evs) * 1e3}
    if a.json:
        print(json.dumps({
            "V": G.num_nodes, "E": E, "h": a.h, "depth": a.depth, "dtype": a.dtype,
            "weight_grad": os.environ.get("NT_WGRAD", "default"), "optim": a.optim,
            **({"embedded": True, "embed_bwd": a.embed_bwd} if a.embedded else {}),
            **({"autocast": "bf16"} if a.autocast else {}),
            **({"readout": a.readout} if a.readout != "sum" else {}),
            **({"loss": a.loss, "tasks": a.tasks,
                "loss_route": "kernel" if crit._kernel_route(torch.empty(1, 1, device="cuda", dtype=dt),
                                                             targets[:1, :1]) else "torch"} if a.loss else {}),
            **layer,
            "max_memory_allocated": mem,
            "warmup": a.warmup, "steps": a.steps,
            "ms": res, "edge_messages_per_s": {k: E * a.depth / (v * 1e-3) for k, v in res.items()},
        }), flush=True)
        return
    print(f"{a.kind} V={G.num_nodes} E={E} h={a.h} depth={a.depth} {a.dtype} optim={a.optim}"
          + (f" embedded embed-bwd={a.embed_bwd}" if a.embedded else "") + (" autocast=bf16" if a.autocast else "")
          + (f" readout={a.readout}" if a.readout != "sum" else "")
          + (f" loss={a.loss} tasks={a.tasks} NT_LOSS={os.environ.get('NT_LOSS', '') or 'default'}" if a.loss else "")
          + (f" dropout={a.dropout} layer {layer['layer_us']:.1f} us: {layer['layer_kernel']}" if layer else ""))
    for k, v in res.items():
        print(f"{k:14s} {v:8.3f} ms/step  {E * a.depth / (v * 1e-3):.3e} edge-msg/s  "
              f"max allocated {mem[k] / 2**20:.1f} MiB")


if __name__ == "__main__":
    main()
