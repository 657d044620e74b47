#!/usr/bin/env python3
"""Time one ranking-metric call on the GPU: the kernel route (nt_rank_metric up to 4096 rows, nt_rank_metric_long
above) against the torch route (rank_metric_torch on the device).

    python tools/rank_bench.py --n 49152 --t 1 --route kernel --calls 200 --warmup 20

Seeded inputs, about 40 % positives, no mask.  Reports ms per call from a host clock around ``--calls`` calls
that end in one device synchronise, as one JSON line.  Fails without a GPU: a CPU run says nothing about time.
Compare routes from fresh processes, alternating them (DESIGN.md section 4 has the table).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, required=True, help="ranked rows")
    ap.add_argument("--t", type=int, default=1, help="columns")
    ap.add_argument("--route", choices=("kernel", "torch"), required=True)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("rank_bench: no GPU; a time measured without one means nothing", file=sys.stderr)
        return 2

    from notorch_amd import kernels as K
    from notorch_amd.nn.metrics import rank_metric_torch

    gen = torch.Generator().manual_seed(args.seed)
    scores = torch.randn(args.n, args.t, generator=gen).cuda()
    targets = (torch.rand(args.n, args.t, generator=gen) < 0.4).float().cuda()
    if args.route == "torch":
        name, call = "rank_metric_torch", lambda: rank_metric_torch(scores, targets)
    elif args.n <= K.rank_metric_max_n():
        name, call = "nt_rank_metric", lambda: K.rank_metric(scores, targets)
    else:
        name, call = "nt_rank_metric_long", lambda: K.rank_metric_long(scores, targets)

    for _ in range(args.warmup):
        res = call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.calls):
        res = call()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / max(args.calls, 1)
    print(json.dumps({"n": args.n, "t": args.t, "route": args.route, "entry": name, "calls": args.calls,
                      "warmup": args.warmup, "ms_per_call": round(ms, 5),
                      "result": [round(v, 6) for v in res[0].tolist()]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
