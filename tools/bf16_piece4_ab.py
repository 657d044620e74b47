"""A/B of the bf16 layer kernel's 8-byte-piece instances (h % 8 == 4) against another build of the library.

Side "ref" runs NT_LIB=variant:<name> (notorch_amd/lib/libnotorch_amd_<name>.so, e.g. the parent
commit's `make`) with _engine.BF16_FUSED_PIECE4 = False, i.e. the routing without these instances;
side "new" runs the shipping library and engine.  Every measurement is a fresh process, the two sides
alternate, and the repeats of one side give the spread.  Raw JSON lines go to --out.

  python tools/bf16_piece4_ab.py --variant parent --out profiles/bf16_piece4/ab.jsonl [--runs 3]

Legs: tools/train_bench.py at h = 300 (config 2 batch in bf16 storage and under bf16 autocast, and
zinc-4096 depth 5), forward alone and the training step; the sha256 of a seeded block's outputs per side
(bf16 and autocast, h = 300 and 36: must be equal); bench.py on config 3 and config 2 fp32 with
--dump-outputs (h % 8 == 0 and fp32: times inside the spread, dumps byte-equal).
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _digest_main():
    """Child process: sha256 of a seeded block's outputs (the engine gate is set by the parent process)."""
    sys.path.insert(0, ROOT)
    import torch

    from notorch_amd.data.synth import make_batch
    from notorch_amd.nn import ChempropBlock
    from notorch_amd.nn.gnn import _engine

    if os.environ.get("PIECE4_GATE") == "0":
        _engine.BF16_FUSED_PIECE4 = False
    res = {}
    G = make_batch("qm9", 512, seed=7).collate("nodes")
    for h in (300, 36):
        for reduce in ("sum", "max"):
            for autocast in (False, True):
                torch.manual_seed(0)
                dt = torch.float32 if autocast else torch.bfloat16
                Xv, Xe = torch.randn(G.num_nodes, h).to(dt), torch.randn(G.num_edges, h).to(dt)
                blk = ChempropBlock(hidden_dim=h, depth=3, reduce=reduce).eval().to(dt).cuda()
                Gd = G.update(node_feats=Xv, edge_feats=Xe).to("cuda")
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    out = blk(Gd)
                torch.cuda.synchronize()
                sha = hashlib.sha256()
                for t in (out.edge_feats, out.node_feats):
                    sha.update(t.contiguous().view(torch.int16).cpu().numpy().tobytes())
                res[f"h{h}-{reduce}-{'autocast' if autocast else 'bf16'}"] = dict(
                    sha256=sha.hexdigest(), fused=_engine.LAST_UPDATE_INFO.get("fused"))
    print(json.dumps(res))


def _train_main():
    """Child process: tools/train_bench.py with the engine gate down."""
    sys.path.insert(0, ROOT)
    import runpy

    from notorch_amd.nn.gnn import _engine

    _engine.BF16_FUSED_PIECE4 = False
    sys.argv = ["train_bench.py"] + sys.argv[2:]
    runpy.run_path(os.path.join(ROOT, "tools", "train_bench.py"), run_name="__main__")


def _run(cmd, env, timeout):
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{' '.join(cmd)} exited with {r.returncode}: stopping")
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return json.loads(lines[-1])


def _dir_digest(d):
    sha = hashlib.sha256()
    names = sorted(os.listdir(d))
    for n in names:
        with open(os.path.join(d, n), "rb") as f:
            sha.update(n.encode() + b"\0" + f.read())
    return dict(files=names, sha256=sha.hexdigest())


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--digest-child":
        return _digest_main()
    if len(sys.argv) > 1 and sys.argv[1] == "--train-child":
        return _train_main()
    p = argparse.ArgumentParser()
    p.add_argument("--variant", default="parent")
    p.add_argument("--out", default=os.path.join(ROOT, "out", "bf16_piece4_ab.jsonl"))
    p.add_argument("--dumps", default=os.path.join(ROOT, "out", "bf16_piece4_dumps"))
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--legs", default="digest,train,bench")
    a = p.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    py, me = sys.executable, os.path.abspath(__file__)
    ref_env = dict(os.environ, NT_LIB=f"variant:{a.variant}", PIECE4_GATE="0")
    new_env = {k: v for k, v in os.environ.items() if k != "NT_LIB"}
    legs = a.legs.split(",")

    def emit(rec):
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)

    if "digest" in legs:
        ref = _run([py, me, "--digest-child"], ref_env, 300)
        new = _run([py, me, "--digest-child"], new_env, 300)
        for k in ref:
            emit(dict(leg="digest", case=k, ref=ref[k], new=new[k], equal=ref[k]["sha256"] == new[k]["sha256"]))
    if "train" in legs:
        classes = {
            "config2_bf16_h300": ["--dtype", "bf16", "--h", "300"],
            "config2_autocast_h300": ["--autocast", "--h", "300"],
            "zinc4096_bf16_h300_d5": ["--kind", "zinc", "--dtype", "bf16", "--h", "300", "--depth", "5"],
        }
        common = ["--modes", "kernel", "--steps", str(a.steps), "--warmup", "10", "--json"]
        for run in range(a.runs):
            for name, args in classes.items():
                emit(dict(leg="train", cls=name, side="ref", run=run,
                          result=_run([py, me, "--train-child"] + args + common, ref_env, 300)))
                emit(dict(leg="train", cls=name, side="new", run=run,
                          result=_run([py, os.path.join(ROOT, "tools", "train_bench.py")] + args + common, new_env,
                                      300)))
    if "bench" in legs:
        for run in range(a.runs):
            for wl in ("zinc-4096-bf16", "qm9-4096"):
                for side, env in (("ref", ref_env), ("new", new_env)):
                    d = os.path.join(a.dumps, f"{wl}_{side}")
                    cmd = [py, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.steps), "--warmup", "10",
                           "--workload", wl, "--no-cpu-baseline"]
                    if run == 0:
                        cmd += ["--dump-outputs", d]
                    res = _run(cmd, env, 420)
                    emit(dict(leg="bench", workload=wl, side=side, run=run,
                              result={k: res[k] for k in res if k in ("metric", "value", "unit", "layer_us", "kernel",
                                                                      "step_ms", "ms_per_step")} or res))
                if run == 0:
                    dr, dn = (_dir_digest(os.path.join(a.dumps, f"{wl}_{s}")) for s in ("ref", "new"))
                    emit(dict(leg="dump", workload=wl, ref=dr, new=dn, equal=dr == dn))


if __name__ == "__main__":
    main()
