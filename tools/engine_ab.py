"""Bit-identity of two checkouts of the Python engine (notorch_amd/nn/gnn/, data/models/graph.py) on one
built library: run --save TAG in a fresh process per side (--root DIR imports notorch_amd from another
tree, e.g. a `git archive` of the parent commit with the same notorch_amd/lib/ copied in), then
--compare TAG_A TAG_B.  Every cell digests node_feats, edge_feats, the Sum readout, after loss.backward()
every parameter / table / input gradient, and the layer launch the forward reported.

Cells: qm9 batches of 37 and 1000 molecules (seed 7) and one polymer with a hub (in-degree > 32);
h = 36, 300, 304 in fp32, bf16 storage and bf16 autocast, 520 in bf16; depth 0 and 3; reduce sum and max;
eval, train (p = 0) and train with dropout 0.25 (torch.manual_seed(0): equal masks); the plain block, the
embedded pair (fuse=True) and an nn.PReLU block (layer by layer); training cells under NT_BWD=kernel and
NT_BWD=torch (the torch recompute, and the PReLU block's backward, under torch.use_deterministic_algorithms:
their scatter_add is otherwise not reproducible from run to run).  A combination the package rejects is
recorded as its exception type."""
import argparse
import contextlib
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("OUT", os.path.join(HERE, "out"))  # the tools' output folder, as the shell scripts' $OUT
DEV = "cuda"
HIDDEN = {"fp32": (36, 300, 304), "bf16": (36, 300, 304, 520), "autocast": (36, 300, 304)}


def digest(t):
    """sha256 of the raw bytes (bf16 through its int16 view)"""
    if t is None:
        return None
    a = t.detach().contiguous()
    if a.dtype == torch.bfloat16:
        a = a.view(torch.int16)
    return hashlib.sha256(a.cpu().numpy().tobytes()).hexdigest()


def graphs():
    from notorch_amd.data.synth import make_batch

    out = {f"qm9-{n}": make_batch("qm9", n, seed=7).collate() for n in (37, 1000)}
    for seed in range(64):  # the first single polymer with a hub
        P = make_batch("polymer", 1, seed=seed).collate()
        if P._nt_layout.deg_range[0] > 32:
            out[f"polymer-s{seed}"] = P
            return out
    raise RuntimeError("no polymer with a hub")


def cells():
    for prec, hs in HIDDEN.items():
        for h in hs:
            for depth in (0, 3):
                for reduce in ("sum", "max"):
                    kinds = ["plain", "embedded"] + (["prelu"] if prec == "fp32" and h != 304 and depth else [])
                    for kind in kinds:
                        for mode in ("eval", "train", "dropout"):
                            for bwd in (("kernel",) if mode == "eval" else ("kernel", "torch")):
                                yield prec, h, depth, reduce, kind, mode, bwd


def run_cell(G, prec, h, depth, reduce, kind, mode, bwd):
    import torch.nn as nn

    from notorch_amd.nn import ChempropBlock, EmbeddedChempropBlock, GraphEmbedding, Sum
    from notorch_amd.nn.gnn import _engine

    os.environ["NT_BWD"] = bwd
    torch.manual_seed(0)
    p = 0.25 if mode == "dropout" else 0.0
    blk = ChempropBlock(hidden_dim=h, depth=depth, reduce=reduce, dropout=p,
                        act=nn.PReLU if kind == "prelu" else nn.ReLU)
    leaves = {}
    if kind == "embedded":
        model = EmbeddedChempropBlock(GraphEmbedding(hidden_dim=h), blk, fuse=True)
        Gd = G.to(DEV)
    else:
        model = blk
        Xv, Xe = torch.randn(G.num_nodes, h), torch.randn(G.num_edges, h)
        if prec == "bf16":
            Xv, Xe = Xv.bfloat16(), Xe.bfloat16()
        Gd = G.update(node_feats=Xv, edge_feats=Xe).to(DEV)
        if mode != "eval":
            leaves = {"Xv": Gd.node_feats.requires_grad_(), "Xe": Gd.edge_feats.requires_grad_()}
    model = model.to(DEV)
    if prec == "bf16":
        model = model.to(torch.bfloat16)
    model.train(mode != "eval")
    leaves.update(model.named_parameters())
    cast = torch.autocast("cuda", dtype=torch.bfloat16) if prec == "autocast" else contextlib.nullcontext()
    _engine.LAST_UPDATE_INFO.clear()
    torch.manual_seed(0)  # the dropout seed draw
    with cast, (torch.no_grad() if mode == "eval" else contextlib.nullcontext()):
        out = model(Gd)
        r = Sum()(out)
        res = {"node": digest(out.node_feats), "edge": digest(out.edge_feats), "readout": digest(r),
               "kernel": _engine.LAST_UPDATE_INFO.get("kernel"), "rows": _engine.LAST_UPDATE_INFO.get("rows")}
        if mode != "eval":
            loss = r.float().square().sum() + 1e-3 * out.edge_feats.float().square().sum()
    if mode != "eval":
        # the torch recompute scatters with atomics unless asked not to: without this its sum cells differ
        # from run to run of one package (every other cell, and every forward, is reproducible as it is)
        torch.use_deterministic_algorithms(bwd == "torch" or kind == "prelu", warn_only=True)
        try:
            loss.backward()
        finally:
            torch.use_deterministic_algorithms(False)
        res.update({f"grad {name}": digest(t.grad) for name, t in leaves.items()})
    torch.cuda.synchronize()
    return res


def run(tag):
    torch.utils.deterministic.fill_uninitialized_memory = False  # torch.empty stays what the engine asked for
    res = {}
    for gname, G in graphs().items():
        for cell in cells():
            key = " ".join(map(str, (gname, *cell)))
            try:
                res[key] = run_cell(G.update(), *cell)
            except (NotImplementedError, RuntimeError, ValueError) as e:
                if any(s in str(e) for s in ("HIP", "hip", "memory access")):  # a device error is no rejection
                    raise
                res[key] = {"rejected": type(e).__name__}
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, f"engine_ab_{tag}.json"), "w") as f:
        json.dump(res, f, indent=0)
    rejected = sum("rejected" in v for v in res.values())
    print(f"{tag}: {len(res)} cells ran ({rejected} rejected), saved")


def compare(ta, tb):
    A = json.load(open(os.path.join(OUT, f"engine_ab_{ta}.json")))
    B = json.load(open(os.path.join(OUT, f"engine_ab_{tb}.json")))
    bad = [k for k in sorted(set(A) | set(B)) if A.get(k) != B.get(k)]
    for k in bad[:40]:
        a, b = A.get(k) or {}, B.get(k) or {}
        print("DIFF", k, sorted(n for n in set(a) | set(b) if a.get(n) != b.get(n)))
    values = sum(len(v) for v in A.values())
    rejected = sum("rejected" in v for v in A.values())
    print(f"{ta}: {len(A)} cells, {tb}: {len(B)} cells, {rejected} rejected on {ta}, {values} values compared, "
          f"{len(bad)} cells differ")
    ok = not bad and len(A) == len(B) and len(A) >= 100
    print("ENGINE_AB", "OK" if ok else "DIFF")
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--save")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--root", default=HERE, help="the tree notorch_amd is imported from")
    a = ap.parse_args()
    if a.save:
        sys.path.insert(0, os.path.abspath(a.root))
        import notorch_amd

        print("notorch_amd from", os.path.dirname(notorch_amd.__file__))
        run(a.save)
    else:
        sys.exit(compare(*a.compare))
