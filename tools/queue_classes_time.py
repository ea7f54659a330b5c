#!/usr/bin/env python3
"""Cost of the class lookups of a queueing engine with limit classes (tbe_create_queue_classes)
against the plain engine, on config D's shape per batch.

Two engines take the same batches through tbe_wait_batch_tick_device (a 2^26-request batch over
1e8 keys plus the fused replenish tick; TokenLimit 4, 1 token/s, QueueLimit 16 OldestFirst,
permits 1, 1 ms of injected time per batch: the trace of bench.py --workload queue): a plain
engine, and one created with three extra classes that all equal class 0's options, its keys
spread over the four.  Requests, decisions and work are identical, so the difference is the
classed layout: wide records and 4-byte replies instead of packed records and narrow replies
(the larger part, as on the token-bucket kind), plus the class bytes and per-decision class
records of the CLS fold.  --no-pack gives the plain engine the same wide layout, which leaves
the lookups alone.  Per batch, HIP events around the one call; median over --repeats batches
after --warm.  Replies and drain counts of the two engines are compared after every batch.
Prints one JSON line and, with --out, writes it to that file (profiles/).

    python tools/queue_classes_time.py [--keys 100000000] [--batch 67108864] [--repeats 7] [--out profiles/queue_classes_time.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keys", type=int, default=100_000_000)
    ap.add_argument("--batch", type=int, default=1 << 26)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--no-pack", action="store_true", help="plain engine with wide records and 4-byte replies too")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from bench_kinds import SEED_D, T0_US, _gen
    from distributedratelimiting.redis_amd import QueueingTokenBucketEngine, _capi

    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    lib = _capi.load()
    n, interval_us = args.batch, 1_000
    opts = (4, 1, 10_000_000, 16, 0)
    kw = {"pack": False, "narrow": False} if args.no_pack else {}
    plain = QueueingTokenBucketEngine(args.keys, *opts, device=0, max_batch=n, **kw)
    classed = QueueingTokenBucketEngine(args.keys, *opts, device=0, max_batch=n, classes=[opts] * 3)
    ids = torch.arange(args.keys, dtype=torch.int64, device=dev)
    cls = (ids % 4).to(torch.uint8)
    torch.cuda.synchronize()
    classed.set_class_device(ids, cls)
    classed.synchronize()
    del ids, cls
    out = {}
    for e in (plain, classed):
        # the drain log: tbe_refresh_bound after any batch is at most n_keys * min(QueueLimit,
        # TokenLimit), and at most every request sent so far
        c = min(args.keys * 4, n * (args.warm + args.repeats + 1), 0xFFFFFFFF)
        out[e] = (torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                  torch.empty(c, dtype=torch.int64, device=dev), torch.empty(c, dtype=torch.int64, device=dev),
                  torch.empty(c, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
    times = {"plain": [], "classed": []}
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        cur = torch.cuda.current_stream(dev).cuda_stream

        def call(eng, k, p, t, s):
            st, rem, ks, li, lr, cnt = out[eng]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.wait_batch_tick_device(k, p, t, st, rem, s * n, T0_US + (s + 1) * interval_us, ks, li, lr, cnt,
                                       stream=cur)
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b)

        for s in range(args.warm + args.repeats):
            k, p, t = _gen(lib, SEED_D, args.keys, s, n, interval_us, dev)
            torch.cuda.synchronize()
            tp, tc = call(plain, k, p, t, s), call(classed, k, p, t, s)
            assert torch.equal(out[plain][0], out[classed][0]) and torch.equal(out[plain][1], out[classed][1])
            assert int(out[plain][5].item()) == int(out[classed][5].item())
            if s >= args.warm:
                times["plain"].append(tp)
                times["classed"].append(tc)
    med = {w: round(statistics.median(v), 4) for w, v in times.items()}
    line = {"keys": args.keys, "batch": n, "repeats": args.repeats, "plain_layout": plain.layout(),
            "classed_layout": classed.layout(), "plain_ms": med["plain"], "classed_ms": med["classed"],
            "ratio": round(med["classed"] / med["plain"], 4),
            "all_ms": {w: [round(x, 4) for x in v] for w, v in times.items()}}
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    plain.close()
    classed.close()


if __name__ == "__main__":
    main()
