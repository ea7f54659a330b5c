#!/usr/bin/env python3
"""Time of the portable-snapshot device calls at scale (include/tbe.h).

A token-bucket table of --keys rows is seeded with 1%, 50% and 100% of its rows live at the
snapshot's timestamp (the others lapsed).  Timed with HIP events on one stream, median over
--repeats warmed repeats, device-resident throughout:

    tbe_export_live_device, capacity 0     the counting call: one read of the table
    tbe_export_live_device, capacity = n   the filling call: count, scan, second read, write
    tbe_import_rows_device                 the exported rows back by id (check, then write)

and, for scale, the dense host export of the same range (tbe_export_state, wall clock; this
call is the same code as before the snapshot calls existed) and the streaming-read rate of
the machine over the table's byte count (tbe_calib_device mode 0, 16 bytes per lane).  The
effective table-read bandwidth of a call is 16 bytes x rows x (table reads) / time.
Prints one JSON line.

    python tools/snapshot_time.py [--keys 10000000] [--repeats 7]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TS = 1_760_000_100_000_123
TTL_MS = 3_000


def timed(fn, repeats, warm=2):
    import torch
    out = []
    for rep in range(warm + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if rep >= warm:
            out.append(a.elapsed_time(b))
    return statistics.median(out)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keys", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch
    from distributedratelimiting.redis_amd import TokenBucketEngine, _capi, snapshot

    n = args.keys
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    lib = _capi.load()
    lib.tbe_calib_device.restype = ctypes.c_int
    lib.tbe_calib_device.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                     ctypes.c_void_p, ctypes.c_void_p]
    rng = np.random.default_rng(1)
    result = {"keys": n, "repeats": args.repeats, "table_MB": round(16 * n / 1e6, 1), "shares": {}}
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        cur = torch.cuda.current_stream(dev).cuda_stream
        # the machine's streaming-read rate over the same byte count
        table_bytes = (16 * n + 127) // 128 * 128
        buf = torch.zeros(table_bytes, dtype=torch.uint8, device=dev)
        sink = torch.zeros(1, dtype=torch.int64, device=dev)
        calib_ms = timed(lambda: lib.tbe_calib_device(0, buf.data_ptr(), table_bytes, n, sink.data_ptr(), cur),
                         args.repeats)
        del buf
        result["stream_read_ms"] = round(calib_ms, 4)
        result["stream_read_GB_per_s"] = round(16 * n / calib_ms / 1e6, 1)
        eng = TokenBucketEngine(n, 5, 2, 10_000_000, device=0)
        lapsed = (TS // 1000 - TTL_MS) * 1000 - 1 - rng.integers(0, 3_000_000, n)
        fresh = TS - rng.integers(0, 2_900_000, n)
        v = rng.uniform(0.0, 5.0, n)
        d_n = torch.zeros(1, dtype=torch.int64, device=dev)
        for share in (0.01, 0.5, 1.0):
            t = np.where(rng.random(n) < share, fresh, lapsed) if share < 1.0 else fresh
            eng.import_state(v, t)
            want = snapshot.live_rows(v, t, TS, TTL_MS)
            count_ms = timed(lambda: eng.export_live_device(TS, None, None, None, d_n, stream=cur), args.repeats)
            live = int(d_n.item())
            assert live == want.shape[0], (live, want.shape[0])
            d_ids = torch.empty(live, dtype=torch.int64, device=dev)
            d_v = torch.empty(live, dtype=torch.float64, device=dev)
            d_t = torch.empty(live, dtype=torch.int64, device=dev)
            fill_ms = timed(lambda: eng.export_live_device(TS, d_ids, d_v, d_t, d_n, stream=cur), args.repeats)
            assert np.array_equal(d_ids.cpu().numpy(), want)
            import_ms = timed(lambda: eng.import_rows(d_ids, d_v, d_t, stream=cur), args.repeats)
            eng.synchronize()
            dense = []
            for _ in range(3):
                t1 = time.perf_counter()
                eng.export_state()
                dense.append((time.perf_counter() - t1) * 1e3)
            result["shares"][str(share)] = {
                "live_rows": live,
                "count_ms": round(count_ms, 4), "count_read_GB_per_s": round(16 * n / count_ms / 1e6, 1),
                "fill_ms": round(fill_ms, 4), "fill_read_GB_per_s": round(2 * 16 * n / fill_ms / 1e6, 1),
                "count_plus_fill_ms": round(count_ms + fill_ms, 4),
                "import_rows_ms": round(import_ms, 4),
                "import_GB_per_s": round((24 + 16 + 16) * live / import_ms / 1e6, 1),
                "dense_export_state_ms": round(statistics.median(dense), 2),
            }
        eng.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
