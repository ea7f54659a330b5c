#!/usr/bin/env python3
"""What lease statistics cost (TBE_FLAG_STATS; DESIGN.md §2d, table "What statistics cost").

Two shapes, device-resident, one GPU; --warmup batches, then --steps timed ones:

    uniform   config B: 1e8 keys, batches of 2^26 uniform requests of 1 permit
    zipf      config C's per-GPU slice: Zipf(1.1) over 1.25e8 keys, the same batches

Each shape with the flag off and on, over the same request stream:

    batch_ms          HIP events around the timed batches of the default (pipelined) engine
    serial_ms         the same on a TBE_FLAG_NO_PIPELINE engine, where nothing overlaps
    count_ms          serial_ms(on) - serial_ms(off): the counting kernel's own time (it is the
                      only thing the flag adds to a token-bucket batch)

and the bytes the counting kernel moves per batch: 9 bytes read per request (key, reply byte)
and one 8-byte atomic add per (tile, distinct key, outcome).  Prints one JSON line.

    python tools/stats_time.py [--shapes uniform,zipf] [--batch 67108864] [--warmup 5] [--steps 20]
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
LIMIT = (10, 1, 10_000_000)
SHAPES = {"uniform": 100_000_000, "zipf": 125_000_000}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="uniform,zipf")
    ap.add_argument("--batch", type=int, default=1 << 26)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from distributedratelimiting.redis_amd import TokenBucketEngine, _capi

    n, total = args.batch, args.warmup + args.steps
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    lib = _capi.load()
    lib.tbe_gen_batch_device.restype = ctypes.c_int
    lib.tbe_gen_batch_device.argtypes = [ctypes.c_uint64] * 4 + [ctypes.c_int32] * 2 + [ctypes.c_int64] * 2 + \
        [ctypes.c_void_p] * 4
    result = {"batch": n, "warmup": args.warmup, "steps": args.steps, "tile": _capi.STATS_TILE,
              "slots": _capi.STATS_SLOTS, "shapes": {}}
    for shape in args.shapes.split(","):
        n_keys = SHAPES[shape]
        bufs = []
        for s in range(total):
            k = torch.empty(n, dtype=torch.int64, device=dev)
            p = torch.empty(n, dtype=torch.int32, device=dev)
            t = torch.empty(n, dtype=torch.int64, device=dev)
            assert lib.tbe_gen_batch_device(SEED, n_keys, s * n, n, 1, 1, T0_US + s * INTERVAL_US, INTERVAL_US,
                                            k.data_ptr(), p.data_ptr(), t.data_ptr(), None) == 0
            if shape == "zipf":
                assert lib.tbe_gen_zipf_keys_device(SEED, n_keys, 1.1, s * n, n, k.data_ptr(), None) == 0
            bufs.append((k, p, t))
        g = torch.empty(n, dtype=torch.uint8, device=dev)
        r = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        # global adds per batch: distinct (tile, key) pairs per outcome, from the last batch's
        # keys and an all-granted / all-denied bound (the outcome split is at most 2x)
        tiles = torch.arange(n, device=dev, dtype=torch.int64) // _capi.STATS_TILE
        pairs = int(torch.unique(tiles * (1 << 32) + bufs[-1][0]).numel())
        del tiles
        out = {"keys": n_keys, "distinct_tile_key_pairs": pairs}
        ms = {}
        for pipeline in (True, False):
            for stats in (False, True):
                eng = TokenBucketEngine(n_keys, *LIMIT, device=0, max_batch=n, pipeline=pipeline, stats=stats)
                for s in range(args.warmup):
                    eng.acquire_batch_device(*bufs[s], g, r)
                eng.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for s in range(args.warmup, total):
                    eng.acquire_batch_device(*bufs[s], g, r)
                eng.synchronize()
                b.record()
                torch.cuda.synchronize()
                ms[(pipeline, stats)] = a.elapsed_time(b) / args.steps
                if stats:
                    ok, failed = eng.stats_totals()
                    assert ok + failed == total * n, (ok, failed)
                    out["granted_fraction"] = round(ok / (ok + failed), 4)
                eng.close()
        out["batch_ms"] = {"off": round(ms[(True, False)], 4), "on": round(ms[(True, True)], 4)}
        out["serial_ms"] = {"off": round(ms[(False, False)], 4), "on": round(ms[(False, True)], 4)}
        count_ms = ms[(False, True)] - ms[(False, False)]
        out["count_ms"] = round(count_ms, 4)
        out["read_GB"] = round(9 * n / 1e9, 3)
        out["atomic_GB_at_least"] = round(8 * pairs / 1e9, 3)
        if count_ms > 0:
            out["read_GB_per_s"] = round(9 * n / count_ms / 1e6, 1)
            out["atomic_GB_per_s_at_least"] = round(8 * pairs / count_ms / 1e6, 1)
        result["shapes"][shape] = out
        del bufs, g, r
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
