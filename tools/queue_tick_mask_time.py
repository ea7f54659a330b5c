#!/usr/bin/env python3
"""What a per-class replenish tick of the queueing kind costs and saves (tbe_refresh_classes_device,
tbe_wait_batch_tick_classes_device), on config D's shape.

One engine with four classes that all equal config D's options (TokenLimit 4, 1 token/s,
QueueLimit 16 OldestFirst), its keys spread evenly over the classes by mix64(key) % 4, takes the
trace of bench.py --workload queue (a 2^26-request batch over 1e8 keys, permits 1, 1 ms of
injected time per batch).  Four variants, each on a fresh engine and the same batches, per call:

    a  refresh_device, unmasked          (after an untimed wait_batch_device of the step's batch)
    b  refresh_device, one class of four (the class rotates with the step; --mask-class fixes it)
    c  wait_batch_tick_device, unmasked  (the batch plus the fused tick)
    d  wait_batch_tick_device, the fused tick masked to one class of four

HIP events around the one call on a stream of its own, --warm calls discarded, median and
quartiles of --repeats calls.  Prints one JSON line and, with --out, writes it to that file
(profiles/).

    python tools/queue_tick_mask_time.py [--keys 100000000] [--batch 67108864] [--out profiles/queue_tick_mask_time.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def mix64_mod4(ids):
    """mix64(id) % 4 on int64 tensors (splitmix64's finalizer; logical shifts by masking)."""
    m1, m2 = 0xBF58476D1CE4E5B9 - (1 << 64), 0x94D049BB133111EB - (1 << 64)
    z = ids
    z = (z ^ ((z >> 30) & ((1 << 34) - 1))) * m1
    z = (z ^ ((z >> 27) & ((1 << 37) - 1))) * m2
    z = z ^ ((z >> 31) & ((1 << 33) - 1))
    return (z & 3).to(ids.dtype)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keys", type=int, default=100_000_000)
    ap.add_argument("--batch", type=int, default=1 << 26)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--variants", default="abcd", help="which of a, b, c, d to run")
    ap.add_argument("--mask-class", type=int, default=-1, help="the one class of b and d; -1: rotate with the step")
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
    steps = args.warm + args.repeats
    cap = min(args.keys * 4, n * (steps + 1), 0xFFFFFFFF)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    rem = torch.empty(n, dtype=torch.int32, device=dev)
    ks = torch.empty(cap, dtype=torch.int64, device=dev)
    li = torch.empty(cap, dtype=torch.int64, device=dev)
    lr = torch.empty(cap, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    cls = torch.empty(args.keys, dtype=torch.uint8, device=dev)
    chunk = 1 << 24
    for k0 in range(0, args.keys, chunk):
        ids = torch.arange(k0, min(args.keys, k0 + chunk), dtype=torch.int64, device=dev)
        cls[k0:k0 + ids.numel()] = mix64_mod4(ids).to(torch.uint8)
    share = [round(float((cls == c).float().mean().item()), 4) for c in range(4)]
    times, grants, layout = {}, {}, None
    stream = torch.cuda.Stream(dev)
    for variant in args.variants:
        eng = QueueingTokenBucketEngine(args.keys, *opts, device=0, max_batch=n, classes=[opts] * 3)
        layout = eng.layout()
        for k0 in range(0, args.keys, chunk):
            ids = torch.arange(k0, min(args.keys, k0 + chunk), dtype=torch.int64, device=dev)
            eng.set_class_device(ids, cls[k0:k0 + ids.numel()])
        eng.synchronize()
        times[variant], grants[variant] = [], []
        with torch.cuda.stream(stream):
            cur = stream.cuda_stream
            for s in range(steps):
                k, p, t = _gen(lib, SEED_D, args.keys, s, n, interval_us, dev)
                tick = T0_US + (s + 1) * interval_us
                classes = [s % 4 if args.mask_class < 0 else args.mask_class] if variant in "bd" else None
                if variant in "ab":
                    eng.wait_batch_device(k, p, t, st, rem, s * n, stream=cur)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                if variant in "ab":
                    eng.refresh_device(tick, ks, li, lr, cnt, stream=cur, classes=classes)
                else:
                    eng.wait_batch_tick_device(k, p, t, st, rem, s * n, tick, ks, li, lr, cnt, stream=cur,
                                               classes=classes)
                b.record()
                torch.cuda.synchronize()
                if s >= args.warm:
                    times[variant].append(a.elapsed_time(b))
                    grants[variant].append(int(cnt.item()))
        eng.close()
        del eng

    def summary(v):
        q = statistics.quantiles(v, n=4)
        return {"median_ms": round(statistics.median(v), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4),
                "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    names = {"a": "refresh_device", "b": "refresh_device_one_class", "c": "wait_batch_tick_device",
             "d": "wait_batch_tick_device_one_class"}
    line = {"keys": args.keys, "batch": n, "warm": args.warm, "repeats": args.repeats, "layout": layout,
            "class_shares": share, "mask_class": "rotates" if args.mask_class < 0 else args.mask_class,
            **{names[v]: summary(times[v]) for v in args.variants},
            "grants_per_call": {names[v]: [min(grants[v]), max(grants[v])] for v in args.variants},
            "all_ms": {names[v]: [round(x, 4) for x in times[v]] for v in args.variants}}
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
