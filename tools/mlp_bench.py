#!/usr/bin/env python3
"""Time the MLP head's inference forward on the GPU: the fused kernel route (nt_mlp_head_forward, NT_MLP=kernel)
against the torch route as the parent of this kernel ran it, a plain nn.Sequential over the same children
(nn.Linear, activation, nn.Dropout modules: one library launch per module).

    python tools/mlp_bench.py [--runs 3] [--rounds 10] [--calls 50] [--out profiles/mlp_head/mlp_bench.jsonl]

Shapes: B in {64, 512, 4096, 32768} x heads [300, 256, 1] and [300, 300, 300, 1] x {fp32, bf16 autocast}, eval
mode under torch.no_grad().  Protocol: `--runs` fresh processes, one after the other; in
each, per shape, both routes are warmed, then take turns for `--rounds` rounds of `--calls` calls.  Device time
per call is the time between two HIP events around the calls; wall time per call is a host clock from the first
call to the end of a device synchronise.  Per run and route the figure is the median over the rounds.

Prints one JSON line per shape: per route the median over the runs' figures, the runs' figures, their run-to-run
spread (max - min) and the spread over all rounds of all runs.  kernel_wins: in every run the kernel's wall
figure is below the torch route's by more than that route's run-to-run spread, and so is its device figure.

--train times a training step through the head instead: forward plus backward on a fixed dY (x requires grad;
gradients are cleared outside the timed region), the head in .train() with NT_MLP_TRAIN=kernel
(nt_mlp_head_forward_train + nt_mlp_head_backward) against the same plain nn.Sequential; B in {64, 512, 4096}.
    python tools/mlp_bench.py --train --out profiles/mlp_head/mlp_train_bench.jsonl
Fails without a GPU."""
import argparse
import contextlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (64, 512, 4096, 32768)
HEADS = ((300, 256, 1), (300, 300, 300, 1))


def child(args) -> int:
    import torch
    import torch.nn as nn

    if not torch.cuda.is_available():
        print("mlp_bench: no GPU; a time measured without one means nothing", file=sys.stderr)
        return 2
    os.environ["NT_MLP"] = "kernel"
    if args.train:
        os.environ["NT_MLP_TRAIN"] = "kernel"
    from notorch_amd import _lib
    from notorch_amd.nn import MLP

    for dims in HEADS:
        torch.manual_seed(0)
        head = MLP(dims[0], dims[-1], hidden_dim=dims[1], num_layers=len(dims) - 2).cuda().train(args.train)
        plain = nn.Sequential(*head)  # the parent's head: the same children in a plain nn.Sequential
        for mode in ("fp32", "bf16"):
            for rows in (BATCHES[:3] if args.train else BATCHES):
                x = torch.randn(rows, dims[0], device="cuda", requires_grad=args.train)
                dy = torch.randn(rows, dims[-1], device="cuda", dtype=torch.bfloat16 if mode == "bf16" else None)
                routes = {"kernel": head, "torch": plain}
                ctx = torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "bf16")
                want = ("mlp_head_train_" if args.train else "mlp_head_") + ("bf16" if mode == "bf16" else "f32")

                def call(mod):
                    if args.train:
                        with ctx:
                            y = mod(x)
                        y.backward(dy)
                    else:
                        mod(x)

                def clear():
                    x.grad = None
                    head.zero_grad(set_to_none=True)

                # inference: one autocast region around everything; training: around each forward only
                with torch.set_grad_enabled(args.train), (contextlib.nullcontext() if args.train else ctx):
                    for name, mod in routes.items():
                        for _ in range(10):
                            call(mod)
                        if name == "kernel":
                            assert _lib.load().nt_last_kernel().decode() == want
                    torch.cuda.synchronize()
                    dev = {n: [] for n in routes}
                    wall = {n: [] for n in routes}
                    for _ in range(args.rounds):
                        for name, mod in routes.items():
                            clear()
                            torch.cuda.synchronize()
                            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            t0 = time.perf_counter()
                            start.record()
                            for _ in range(args.calls):
                                call(mod)
                            stop.record()
                            torch.cuda.synchronize()
                            wall[name].append((time.perf_counter() - t0) * 1e3 / args.calls)
                            dev[name].append(start.elapsed_time(stop) / args.calls)
                print(json.dumps({"dims": list(dims), "mode": mode, "rows": rows, "device_ms": dev, "wall_ms": wall}),
                      flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default="")
    ap.add_argument("--train", action="store_true", help="time forward + backward (NT_MLP_TRAIN=kernel)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    runs = []  # per run: {(dims, mode, rows): row}
    for _ in range(args.runs):  # fresh processes, one at a time; this one never opens the GPU
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(args.rounds),
                            "--calls", str(args.calls)] + (["--train"] if args.train else []), stdout=subprocess.PIPE, text=True, timeout=900)
        if p.returncode != 0:
            return p.returncode
        rows = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
        runs.append({(tuple(r["dims"]), r["mode"], r["rows"]): r for r in rows})
        print(f"mlp_bench: run {len(runs)} of {args.runs} done", file=sys.stderr, flush=True)

    lines = []
    for key in runs[0]:
        dims, mode, rows = key
        row = {"dims": list(dims), "mode": mode, "rows": rows, "runs": args.runs, "rounds": args.rounds,
               "calls": args.calls}
        wins = True
        for clock in ("device_ms", "wall_ms"):
            fig = {}
            for route in ("kernel", "torch"):
                per_run = [statistics.median(r[key][clock][route]) for r in runs]
                every = [v for r in runs for v in r[key][clock][route]]
                fig[route] = {"median": round(statistics.median(per_run), 4), "per_run": [round(v, 4) for v in per_run],
                              "spread": round(max(per_run) - min(per_run), 4),
                              "round_spread": round(max(every) - min(every), 4)}
            row[clock] = fig
            wins = wins and all(t - k > fig["torch"]["spread"]
                                for k, t in zip(fig["kernel"]["per_run"], fig["torch"]["per_run"]))
        row["kernel_wins"] = wins
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
