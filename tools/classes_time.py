#!/usr/bin/env python3
"""What limit classes cost at config B's shape.

1e8 keys, batches of 2^26 uniform requests of 1 permit, device-resident, one GPU; --warmup
batches, then --steps timed ones.  Three engines over the same request stream:

    wide       a plain engine with TBE_FLAG_NO_PACK | NO_HOT | NO_NARROW: the existing
               wide-record path, which a classed engine is laid out as
    classed0   a classed engine (the four test classes), every key in class 0
    classed4   the same with the keys spread over the four classes

Per engine: the batch time (HIP events around the timed batches, pipelined), the fold's time
from TBE_FLAG_FOLD_TIMING, the grant rate, and the bytes the fold must move per batch -- the
records in, the touched buckets' table slices in, their dirty lines out (counted as whole
slices: an upper bound), the replies out, and for a classed engine one class byte per row of
a touched slice.  Prints one JSON line.

    python tools/classes_time.py [--keys 100000000] [--batch 67108864] [--warmup 5] [--steps 20]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 0x5EED000B
T0_US = 1_760_000_000_000_000
INTERVAL_US = 10_000
# (TokenLimit, TokensPerPeriod, ticks): class 0 is config B's limiter
CLASSES = [(10, 1, 10_000_000), (3, 1, 30_000_000), (100, 50, 1_000_000), (5, 10, 10_000_000)]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keys", type=int, default=100_000_000)
    ap.add_argument("--batch", type=int, default=1 << 26)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from distributedratelimiting.redis_amd import TokenBucketEngine, _capi

    n, n_keys, total = args.batch, args.keys, args.warmup + args.steps
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    lib = _capi.load()
    lib.tbe_gen_batch_device.restype = ctypes.c_int
    lib.tbe_gen_batch_device.argtypes = [ctypes.c_uint64] * 4 + [ctypes.c_int32] * 2 + [ctypes.c_int64] * 2 + \
        [ctypes.c_void_p] * 4
    bufs = []
    for s in range(total):
        k = torch.empty(n, dtype=torch.int64, device=dev)
        p = torch.empty(n, dtype=torch.int32, device=dev)
        t = torch.empty(n, dtype=torch.int64, device=dev)
        assert lib.tbe_gen_batch_device(SEED, n_keys, s * n, n, 1, 1, T0_US + s * INTERVAL_US, INTERVAL_US,
                                        k.data_ptr(), p.data_ptr(), t.data_ptr(), None) == 0
        bufs.append((k, p, t))
    g = torch.empty(n, dtype=torch.uint8, device=dev)
    r = torch.empty(n, dtype=torch.int32, device=dev)
    d_ids = torch.arange(n_keys, dtype=torch.int64, device=dev)
    # a fixed odd multiplier and a middle bit pair: the four classes evenly over the ids
    d_spread = (((d_ids * 0x9E3779B1) >> 13) & 3).to(torch.uint8)
    torch.cuda.synchronize()

    result = {"keys": n_keys, "batch": n, "warmup": args.warmup, "steps": args.steps, "classes": CLASSES,
              "configs": {}}
    for name in ("wide", "classed0", "classed4"):
        if name == "wide":
            eng = TokenBucketEngine(n_keys, *CLASSES[0], device=0, stage_timing="fold", max_batch=n,
                                    pack=False, hot=False, narrow=False)
        else:
            eng = TokenBucketEngine(n_keys, *CLASSES[0], device=0, stage_timing="fold", max_batch=n,
                                    classes=CLASSES[1:])
        lay = eng.layout()
        assert not lay["packed"] and not lay["hot"] and not lay["narrow"], lay
        if name == "classed4":
            eng.set_class_device(d_ids, d_spread)
        for s in range(args.warmup):
            eng.acquire_batch_device(*bufs[s], g, r)
        eng.synchronize()
        eng.stage_times()   # discard the warm-up's
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        granted = 0
        a.record()
        for s in range(args.warmup, total):
            eng.acquire_batch_device(*bufs[s], g, r)
        eng.synchronize()
        b.record()
        torch.cuda.synchronize()
        granted = int(g.sum().item())   # of the last batch
        fold_ms = eng.stage_times()["fold"] / args.steps
        # bytes the fold moves per batch: wide records {key 4, permits 4, ts 8} in, 4-byte
        # replies out, the touched buckets' 16-byte rows in and (at most) out again, and the
        # class bytes of those buckets
        rows = 1 << lay["r_bits"]
        nb = (n_keys + rows - 1) // rows
        touched = nb if n >= 8 * nb else min(nb, n)          # a dense batch touches every bucket
        slice_rows = min(touched * rows, n_keys)
        moved = {"records_in": 16 * n, "replies_out": 4 * n, "rows_in": 16 * slice_rows,
                 "rows_out_at_most": 16 * slice_rows, "class_bytes_in": slice_rows if name != "wide" else 0}
        result["configs"][name] = {
            "batch_ms": round(a.elapsed_time(b) / args.steps, 4),
            "fold_ms": round(fold_ms, 4),
            "grant_rate_last_batch": round(granted / n, 4),
            "fold_bytes": moved,
            "fold_GB": round(sum(moved.values()) / 1e9, 3),
            "fold_GB_per_s_at_most": round(sum(moved.values()) / fold_ms / 1e6, 1),
        }
        eng.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
