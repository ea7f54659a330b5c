#!/usr/bin/env python3
"""Time of one reclaim of the device string directory at scale (include/tbe_strdir.h).

capacity keys "user-<k>" (~16 bytes of arena each) are held, every one with a bucket row;
half of the rows have lapsed.  Timed with HIP events on one stream, --repeats times, median:

    expired_device(ts, d_dead, clear=True)      one pass over the engine's rows
    reclaim_device(d_dead)                      victims out, survivors compacted and re-placed

Between repeats the removed half is assigned and decided again (untimed), so every repeat
reclaims the same number of keys.  For scale only, the step a host-side reclaim needs at the
same shape is timed in the same run (wall clock): tbe_export_state of the same rows in
1M-row chunks.  Prints one JSON line.

    python tools/sdir_reclaim_time.py [--capacity 10000000] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T0 = 1_760_000_000_000_000


def model_bytes(n: int, nslots: int, live: int, dead: int, text: int) -> dict:
    """Bytes the two calls move, from what each kernel reads and writes (no cache effects):
    the scan reads every 16-byte row, writes a flag and rewrites the lapsed rows; the reclaim
    reads the flags and iloc, writes and re-reads the victim flags, pushes the victims, walks
    the slot ids twice, moves the survivors' text and 20-byte records, resets the slot table
    (16 bytes per slot) and writes the survivors' slots back."""
    scan = 16 * n + n + 16 * dead
    reclaim = (8 * n + n + n) + 2 * n + (4 + 8) * dead \
        + 2 * (4 * nslots + (8 + 1) * (live + dead)) + (8 + 2 * text + 20 + 8) * live \
        + 16 * nslots + (20 + 20) * live
    return {"expired_GB": round(scan / 1e9, 3), "reclaim_GB": round(reclaim / 1e9, 3)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--capacity", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from distributedratelimiting.redis_amd import TokenBucketEngine
    from distributedratelimiting.redis_amd.strdir import StringDirectory, synthetic_key_text

    n = args.capacity
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        cur = torch.cuda.current_stream(dev).cuda_stream
        d = StringDirectory(n, 16 * n + (1 << 20), prefix="bench:", device=0)
        eng = TokenBucketEngine(n, 5, 2, 10_000_000, device=0)
        keys = torch.arange(n, dtype=torch.int64, device=dev)
        buf, offs, nb = synthetic_key_text(keys, "user-")
        ones = torch.ones(n, dtype=torch.int32, device=dev)
        g = torch.empty(n, dtype=torch.uint8, device=dev)
        r = torch.empty(n, dtype=torch.int32, device=dev)
        dead = torch.empty(n, dtype=torch.uint8, device=dev)
        times, counts = [], []
        for rep in range(args.repeats):
            base = T0 + rep * 100_000_000
            ids = d.assign(buf, offs, nb)                       # the removed half comes back
            eng.acquire_batch_device(ids, ones, torch.full((n,), base, dtype=torch.int64, device=dev), g, r,
                                     stream=cur)
            alive = ids[::2].contiguous()                       # every other string stays in use
            m = alive.numel()
            eng.acquire_batch_device(alive, ones[:m], torch.full((m,), base + 5_000_000, dtype=torch.int64,
                                                                 device=dev), g[:m], r[:m], stream=cur)
            torch.cuda.synchronize(dev)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            eng.expired_device(base + 6_000_000, dead, clear=True, stream=cur)
            ev[1].record()
            count = d.reclaim_device(dead)
            ev[2].record()
            torch.cuda.synchronize(dev)
            times.append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
            counts.append(int(count.item()))
            assert counts[-1] == n - m and d.size() == m, (counts[-1], d.size())
        # the host-side reclaim's first step at the same shape: every row to the host
        t1 = time.perf_counter()
        chunk = 1_000_000
        for first in range(0, n, chunk):
            eng.export_state(first, min(chunk, n - first))
        export_ms = (time.perf_counter() - t1) * 1e3
        nslots = 1
        while nslots < 2 * n:
            nslots <<= 1
        text = 16
        scan_ms = statistics.median(t[0] for t in times)
        rec_ms = statistics.median(t[1] for t in times)
        gb = model_bytes(n, nslots, n - counts[-1], counts[-1], text)
        print(json.dumps({
            "capacity": n, "reclaimed_per_repeat": counts[-1], "repeats": args.repeats,
            "text_bytes_per_key": round(nb / n, 2),
            "expired_device_ms": round(scan_ms, 3), "reclaim_device_ms": round(rec_ms, 3),
            "total_ms": round(scan_ms + rec_ms, 3),
            "all_ms": [[round(a, 3), round(b, 3)] for a, b in times],
            **gb,
            "GB_per_s": round((gb["expired_GB"] + gb["reclaim_GB"]) / ((scan_ms + rec_ms) / 1e3), 1),
            "host_export_state_1M_chunks_ms": round(export_ms, 1),
        }), flush=True)
        eng.close()
        d.close()


if __name__ == "__main__":
    main()
