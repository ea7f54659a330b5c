#!/usr/bin/env python3
"""Time of one reclaim of the device u64 key directory at scale, and of the assign path it
touches (include/tbe_cluster.h).

--part reclaim: a directory of --capacity ids behind an engine of as many keys, every id
held and every key with a bucket row.  For 1 %, 50 % and 100 % of the rows lapsed, the median
of --repeats warmed repeats of tbe_dir_reclaim_device, HIP events around the one call (the
flags come from expired_device before the first event).  Between repeats the removed keys are
assigned and decided again (untimed), so every repeat removes the same number.  In the same
run, what a caller without a reclaim must do instead: tbe_dir_create plus one
tbe_dir_assign_device of the surviving keys (wall clock around both, device synchronised).

--part assign: tbe_dir_assign_device on a directory that is never reclaimed, median and
min-max of --repeats repeats: 2^24 requests over the 1e7 known keys, and a batch of 2^20
new keys.  It calls the library through ctypes alone, so --lib runs the same measurement
against a library built from another commit.

Prints one JSON line per part.

    python tools/dir_reclaim_time.py [--part reclaim|assign|all] [--capacity 10000000] [--repeats 7] [--lib PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T0 = 1_760_000_000_000_000
MULT = -7046029254386353131          # 0x9E3779B97F4A7C15 as int64: key = index * MULT + 1 (a bijection)


def _keys(idx):
    return idx * MULT + 1


def _ms(ev0, ev1):
    return round(ev0.elapsed_time(ev1), 3)


def part_reclaim(args) -> dict:
    import torch
    from distributedratelimiting.redis_amd import TokenBucketEngine
    from distributedratelimiting.redis_amd.cluster import DeviceDirectory

    n = args.capacity
    dev = torch.device("cuda:0")
    out = {"part": "reclaim", "capacity": n, "repeats": args.repeats, "levels": {}}
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        cur = torch.cuda.current_stream(dev).cuda_stream
        d = DeviceDirectory(n, device=0)
        eng = TokenBucketEngine(n, 5, 2, 10_000_000, device=0)
        keys = _keys(torch.arange(n, dtype=torch.int64, device=dev))
        ones = torch.ones(n, dtype=torch.int32, device=dev)
        g = torch.empty(n, dtype=torch.uint8, device=dev)
        r = torch.empty(n, dtype=torch.int32, device=dev)
        dead = torch.empty(n, dtype=torch.uint8, device=dev)
        base = T0
        for name, every in (("1%", 100), ("50%", 2), ("100%", 1)):
            victim = torch.zeros(n, dtype=torch.bool, device=dev)
            victim[::every] = True
            n_dead = int(victim.sum().item())
            alive_keys = keys[~victim].contiguous()
            times = []
            for rep in range(args.repeats + 1):            # the first repeat warms up
                base += 100_000_000
                ids = d.assign(keys)                        # the removed keys come back
                eng.acquire_batch_device(ids, ones, torch.full((n,), base, dtype=torch.int64, device=dev), g, r,
                                         stream=cur)
                alive = ids[~victim].contiguous()
                m = alive.numel()
                if m:
                    eng.acquire_batch_device(alive, ones[:m], torch.full((m,), base + 5_000_000, dtype=torch.int64,
                                                                         device=dev), g[:m], r[:m], stream=cur)
                eng.expired_device(base + 6_000_000, dead, clear=True, stream=cur)
                torch.cuda.synchronize(dev)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                count = d.reclaim_device(dead)
                ev[1].record()
                torch.cuda.synchronize(dev)
                assert int(count.item()) == n_dead and d.size() == n - n_dead, (int(count.item()), d.size())
                if rep:
                    times.append(_ms(ev[0], ev[1]))
            # today's alternative: a new directory and the survivors assigned into it
            recreate = []
            for rep in range(3):
                torch.cuda.synchronize(dev)
                t1 = time.perf_counter()
                d2 = DeviceDirectory(n, device=0)
                if alive_keys.numel():
                    d2.assign(alive_keys)
                torch.cuda.synchronize(dev)
                recreate.append(round((time.perf_counter() - t1) * 1e3, 3))
                d2.close()
            out["levels"][name] = {"reclaimed": n_dead, "reclaim_device_ms": statistics.median(times),
                                   "all_ms": times, "create_plus_assign_survivors_ms": statistics.median(recreate),
                                   "create_plus_assign_all_ms": recreate}
        eng.close()
        d.close()
    return out


def part_assign(args) -> dict:
    import torch
    path = args.lib or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "distributedratelimiting.redis_amd", "libtbe.so")
    lib = ctypes.CDLL(path)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.tbe_dir_create.restype = ctypes.c_int32
    lib.tbe_dir_create.argtypes = [u64, ctypes.c_int32, ctypes.POINTER(vp)]
    lib.tbe_dir_destroy.restype = None
    lib.tbe_dir_destroy.argtypes = [vp]
    lib.tbe_dir_assign_device.restype = ctypes.c_int32
    lib.tbe_dir_assign_device.argtypes = [vp, vp, u64, vp, vp]
    lib.tbe_dir_size.restype = ctypes.c_int32
    lib.tbe_dir_size.argtypes = [vp, ctypes.POINTER(u64)]

    known, n_req, n_new = 10_000_000, 1 << 24, 1 << 20
    cap = known + (args.repeats + 1) * n_new
    dev = torch.device("cuda:0")
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        cur = torch.cuda.current_stream(dev).cuda_stream
        h = vp()
        assert lib.tbe_dir_create(cap, 0, ctypes.byref(h)) == 0
        ids = torch.empty(n_req, dtype=torch.int64, device=dev)

        def assign(k):
            assert lib.tbe_dir_assign_device(h, k.data_ptr(), k.numel(), ids.data_ptr(), cur) == 0

        assign(_keys(torch.arange(known, dtype=torch.int64, device=dev)))
        gen = torch.Generator(device=dev)
        gen.manual_seed(7)
        t_known, t_new = [], []
        for rep in range(args.repeats + 1):                 # the first repeat warms up
            req = _keys(torch.randint(0, known, (n_req,), generator=gen, device=dev, dtype=torch.int64))
            new = _keys(torch.arange(known + rep * n_new, known + (rep + 1) * n_new, dtype=torch.int64, device=dev))
            torch.cuda.synchronize(dev)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            assign(req)
            ev[1].record()
            ev[2].record()
            assign(new)
            ev[3].record()
            torch.cuda.synchronize(dev)
            if rep:
                t_known.append(_ms(ev[0], ev[1]))
                t_new.append(_ms(ev[2], ev[3]))
        held = u64()
        assert lib.tbe_dir_size(h, ctypes.byref(held)) == 0 and held.value == cap, held.value
        lib.tbe_dir_destroy(h)

    def stat(t):
        return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "all_ms": t}

    return {"part": "assign", "lib": os.path.basename(path), "capacity": cap, "repeats": args.repeats,
            "known_2p24_requests_over_1e7_keys": stat(t_known), "new_2p20_keys": stat(t_new)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("reclaim", "assign", "all"), default="all")
    ap.add_argument("--capacity", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--lib", default=None, help="--part assign: the libtbe.so to measure (default: this tree's)")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    if args.part in ("reclaim", "all"):
        print(json.dumps(part_reclaim(args)), flush=True)
    if args.part in ("assign", "all"):
        print(json.dumps(part_assign(args)), flush=True)


if __name__ == "__main__":
    main()
