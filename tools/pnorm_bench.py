#!/usr/bin/env python3
"""Time PNorm's pairwise kernels (nt_pairwise_pnorm / nt_pairwise_pnorm_backward) against the torch.cdist
route they would replace, on the GPU.

    python tools/pnorm_bench.py [--n 256 1024 4096] [--rounds 10] [--calls 5]

DESIGN.md section 4's protocol: the inputs stay on the device; per shape the contenders take turns,
`--rounds` rounds in one process, each timing `--calls` calls between two HIP events; the figure is the median
over the rounds, the spread max - min.  Shapes: p = 1 with d in {1, 12} (the label distance of
RankNContrastLoss), p = 2 negated with d in {8, 300} (its similarity), self mode, fp32.  Contenders: the
module under NT_PNORM=kernel and under NT_PNORM=torch (torch.cdist with PNorm's row-block guard), forward
only (no_grad) and forward + backward (X.backward(G) for a fixed random G).

Prints one JSON line per shape and a last line with PNORM_KERNEL_P as nn/loss/rnc.py defines it: a p is listed
only if at every shape timed for it the kernel's median is below torch's by more than torch's spread, forward
and forward + backward.  Fails without a GPU: a CPU run says nothing about time."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS = {1: (1, 12), 2: (8, 300)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("pnorm_bench: no GPU; a time measured without one means nothing", file=sys.stderr)
        return 2

    from notorch_amd.nn.loss.rnc import PNorm

    def routed(knob, call):
        def run():
            os.environ["NT_PNORM"] = knob  # read per call by PNorm
            call()
        return run

    listed = []
    for p, dims in DIMS.items():
        all_win = True
        norm = PNorm(p=float(p), negate=p == 2)
        for n in sorted(args.n):
            for d in dims:
                gen = torch.Generator().manual_seed(args.seed + 31 * n + d)
                A = (0.5 * torch.randn(n, d, generator=gen)).cuda()
                G = torch.randn(n, n, generator=gen).cuda()
                leaf = A.clone().requires_grad_()

                def fwd():
                    with torch.no_grad():
                        norm(A)

                def fwd_bwd():
                    leaf.grad = None
                    norm(leaf).backward(G)

                contenders = {f"{route}_{name}": routed(route, call) for route in ("kernel", "torch")
                              for name, call in (("fwd", fwd), ("fwd_bwd", fwd_bwd))}
                try:
                    for call in contenders.values():  # every shape once before it is timed
                        call()
                        call()
                    torch.cuda.synchronize()
                except RuntimeError as exc:  # a route that refuses a shape has no time: its p is not listed
                    print(json.dumps({"p": p, "n": n, "d": d, "error": str(exc).splitlines()[0]}), flush=True)
                    all_win = False
                    continue
                ms = {name: [] for name in contenders}
                for _ in range(args.rounds):
                    for name, call in contenders.items():
                        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        start.record()
                        for _ in range(args.calls):
                            call()
                        stop.record()
                        stop.synchronize()
                        ms[name].append(start.elapsed_time(stop) / args.calls)
                row = {"p": p, "n": n, "d": d, "rounds": args.rounds, "calls": args.calls}
                for name, v in ms.items():
                    row[name] = {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}
                row["kernel_wins"] = all(
                    row[f"torch_{w}"]["median_ms"] - row[f"kernel_{w}"]["median_ms"] > row[f"torch_{w}"]["spread_ms"]
                    for w in ("fwd", "fwd_bwd"))
                all_win = all_win and row["kernel_wins"]
                print(json.dumps(row), flush=True)
        if all_win:
            listed.append(p)
    os.environ.pop("NT_PNORM", None)
    print(json.dumps({"PNORM_KERNEL_P": listed}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
