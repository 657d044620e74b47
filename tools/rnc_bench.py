#!/usr/bin/env python3
"""Time the ranking part of RankNContrastLoss above 4096 rows on the GPU: nt_rnc_rank_long against the
module's torch route (rank_loss_torch), which is what runs there without the kernel.

    python tools/rnc_bench.py [--n 4097 6144 8192 12288 16384] [--rounds 10] [--calls 5]

DESIGN.md section 4's RnC protocol: Sim and D (fp32, from the default PNorms of X = 0.5 randn(N, 8) and
distinct targets) stay on the device; per N the contenders take turns, `--rounds` rounds in one process,
each timing `--calls` calls between two HIP events; the figure is the median over the rounds, the spread
max - min.  Contenders: rnc_rank_long with dSim, rnc_rank_long forward only, RnCRankLongFunction forward +
backward (what the module adds: the row sum and grad_out * dSim), the torch route forward + backward, the
torch route forward only.

Prints one JSON line per N and a last line with RNC_LONG_DEFAULT_MAX_N as nn/loss/rnc.py defines it: the
largest timed N at which, as at every smaller timed N, the median of rnc_rank_long with dSim is below the
median of the torch route forward + backward by more than that route's spread (0 if at none).  Fails
without a GPU: a CPU run says nothing about time."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TEMP, EPS = 2.0, 1e-6


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[4097, 6144, 8192, 12288, 16384])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("rnc_bench: no GPU; a time measured without one means nothing", file=sys.stderr)
        return 2

    from notorch_amd import kernels as K
    from notorch_amd.nn.loss.rnc import RankNContrastLoss, RnCRankLongFunction, rank_loss_torch

    crit = RankNContrastLoss(temp=TEMP)
    default, unbroken = 0, True  # the largest N of the unbroken run of wins from the smallest timed N
    for n in sorted(args.n):
        gen = torch.Generator().manual_seed(args.seed + n)
        with torch.no_grad():
            sim = crit.similarity((0.5 * torch.randn(n, 8, generator=gen)).cuda()).contiguous()
            dist = crit.distance(torch.randn(n, 2, generator=gen).cuda()).contiguous()
        leaf = sim.clone().requires_grad_()

        def function_fwd_bwd():
            leaf.grad = None
            RnCRankLongFunction.apply(leaf, dist, TEMP, EPS, True).backward()

        def torch_fwd_bwd():
            leaf.grad = None
            rank_loss_torch(leaf, dist, TEMP, EPS).backward()

        def torch_fwd():
            with torch.no_grad():
                rank_loss_torch(sim, dist, TEMP, EPS)

        contenders = {
            "long_dsim": lambda: K.rnc_rank_long(sim, dist, TEMP, EPS, True),
            "long_fwd": lambda: K.rnc_rank_long(sim, dist, TEMP, EPS, False),
            "function_fwd_bwd": function_fwd_bwd,
            "torch_fwd_bwd": torch_fwd_bwd,
            "torch_fwd": torch_fwd,
        }
        for call in contenders.values():  # every shape once before it is timed
            call()
            call()
        torch.cuda.synchronize()
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
        row = {"n": n, "rounds": args.rounds, "calls": args.calls}
        for name, v in ms.items():
            row[name] = {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4)}
        wins = (row["torch_fwd_bwd"]["median_ms"] - row["long_dsim"]["median_ms"]) > row["torch_fwd_bwd"]["spread_ms"]
        row["kernel_wins"] = wins
        unbroken = unbroken and wins
        if unbroken:
            default = n
        print(json.dumps(row), flush=True)
        del sim, dist, leaf
        torch.cuda.empty_cache()
    print(json.dumps({"RNC_LONG_DEFAULT_MAX_N": default, "rnc_long_max_n": K.rnc_long_max_n()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
