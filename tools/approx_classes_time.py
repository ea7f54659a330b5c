#!/usr/bin/env python3
"""Cost of limit classes on an approximate engine (tbe_create_approx_classes) against the plain
engine, on config E's shape: batches of AcquireCore decisions over 1e7 keys (TokenLimit 100, one
token per 10 ms period, QueueLimit 0, permits 1; the trace of bench.py --workload approx), each
followed by one refresh epoch at the batch's time.

Engines, all fed the same batches and epochs:
  plain         tbe_create, packed records, lazy client views (one-client refresh)
  plain_wide    the same with TBE_FLAG_NO_PACK: the records a classed engine moves
  plain_views   plain, but each epoch is tbe_approx_collect + tbe_approx_sync with two clients
                (the second one's counts all zero): the sync that also writes the 16-byte client
                views, which is what a classed engine's sync always does.  Its decisions differ
                from the others' (two clients halve the caps), so it is timed, not compared
  classed_0     three extra classes equal to class 0, every key left in class 0
  classed_4     four different classes, keys spread over them by key % 4; the refresh is unmasked
plain - plain_wide is the record layout, plain_views' sync against plain's the written views, and
classed_0 against plain_wide what is left: the class bytes and the per-decision class records.
Replies of plain, plain_wide and classed_0 are compared after every batch.  A batch is timed by HIP
events around the call on the stream it runs on; an epoch, which returns when its drain count is
read, by the host's clock.  Medians over --repeats steps after --warm.  Prints one JSON line and, with --out,
writes it to that file (profiles/).

    python tools/approx_classes_time.py [--keys 10000000] [--batch 67108864] [--repeats 7] [--out profiles/approx_classes_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keys", type=int, default=10_000_000)
    ap.add_argument("--batch", type=int, default=1 << 26)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from bench_kinds import SEED_E, T0_US, _gen
    from distributedratelimiting.redis_amd import ApproximateEngine, _capi

    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    lib = _capi.load()
    n, interval_us = args.batch, 10_000
    opts = (100, 1, 100_000, 0, 0)
    four = [opts, (50, 1, 100_000, 0, 0), (200, 3, 100_000, 0, 0), (100, 1, 200_000, 0, 0)]

    def make(name):
        kw = dict(device=0, max_batch=n)
        if name == "plain_wide":
            kw["pack"] = False
        if name == "classed_0":
            kw["approx_classes"] = [opts] * 3
        if name == "classed_4":
            kw["approx_classes"] = four[1:]
        return ApproximateEngine(args.keys, *opts, **kw)

    names = ["plain", "plain_wide", "plain_views", "classed_0", "classed_4"]
    engines = {w: make(w) for w in names}
    ids = torch.arange(args.keys, dtype=torch.int64, device=dev)
    cls = (ids % 4).to(torch.uint8)
    torch.cuda.synchronize()
    engines["classed_4"].set_class_device(ids, cls)
    engines["classed_4"].synchronize()
    del ids, cls
    st = {w: torch.empty(n, dtype=torch.uint8, device=dev) for w in names}
    av = {w: torch.empty(n, dtype=torch.int32, device=dev) for w in names}
    counts = torch.zeros(2 * args.keys, dtype=torch.int32, device=dev)     # plain_views: [2][n_keys], client 1 all 0
    torch.cuda.synchronize()
    batch_ms = {w: [] for w in names}
    sync_ms = {w: [] for w in names}

    side = torch.cuda.Stream(dev)
    cur = side.cuda_stream

    def batch(e, k, p, w, s):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            a.record()
            e.acquire_batch_device(k, p, st[w], av[w], wait=False, id_base=s * n, stream=cur)
            b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3

    for s in range(args.warm + args.repeats):
        k, p, _ = _gen(lib, SEED_E, args.keys, s, n, interval_us, dev)
        torch.cuda.synchronize()
        ts = T0_US + (s + 1) * interval_us
        for w in names:
            e = engines[w]
            tb = batch(e, k, p, w, s)
            if w == "plain_views":
                e.collect(counts[: args.keys])
                tsync = wall(lambda: e.sync(counts, 2, 0, ts, 0))
            else:
                tsync = wall(lambda: e.refresh(ts))
            if s >= args.warm:
                batch_ms[w].append(tb)
                sync_ms[w].append(tsync)
        for w in ("plain_wide", "classed_0"):
            assert torch.equal(st["plain"], st[w]) and torch.equal(av["plain"], av[w]), w
    med = lambda d: {w: round(statistics.median(v), 4) for w, v in d.items()}   # noqa: E731
    line = {"keys": args.keys, "batch": n, "repeats": args.repeats,
            "layouts": {w: engines[w].layout() for w in names},
            "batch_ms": med(batch_ms), "sync_ms": med(sync_ms),
            "all_batch_ms": {w: [round(x, 4) for x in v] for w, v in batch_ms.items()},
            "all_sync_ms": {w: [round(x, 4) for x in v] for w, v in sync_ms.items()}}
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
