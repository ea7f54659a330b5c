#!/usr/bin/env python3
"""Time of the approximate limiter's idle-key and tier-snapshot device calls at scale
(include/tbe.h).

An approximate engine of --keys keys gets a tier in which about half of the rows are worth
no tokens at the scan's timestamp.  Timed with HIP events on one stream, median over
--repeats warmed repeats, device-resident throughout:

    tbe_approx_idle_device, view written    the scan after a sync that wrote the client view
                                            (it reads the 4-byte global score of each 16-byte
                                            AClient row: whole lines come in, a quarter is used)
    tbe_approx_idle_device, view derived    the scan after a one-client refresh: no AClient read
    tbe_approx_export_live_device           capacity 0 (count: one read of t) and capacity = n
                                            (count, scan, second read of t, v and p of the
                                            exported rows, write), with the idle flags as mask
    tbe_approx_import_rows_device           the exported rows back by id (check, then write)
    tbe_approx_reset_device                 the idle keys reset (only flagged rows are written)

and, for scale, the host path that existed before these calls for the same information
(tbe_approx_export_state over the range, wall clock) and the machine's streaming-read rate
over the derived-view scan's byte count (tbe_calib_device mode 0, 16 bytes per lane).  The
scan's result is checked against snapshot.approx_idle_rows on the way.  Prints one JSON line.

    python tools/approx_idle_time.py [--keys 10000000] [--repeats 7]
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
    from distributedratelimiting.redis_amd import ApproximateEngine, _capi, fill_rate, snapshot

    n = args.keys
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    lib = _capi.load()
    lib.tbe_calib_device.restype = ctypes.c_int
    lib.tbe_calib_device.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                     ctypes.c_void_p, ctypes.c_void_p]
    rng = np.random.default_rng(1)
    rate = fill_rate(2, 10_000_000)
    result = {"keys": n, "repeats": args.repeats}
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        cur = torch.cuda.current_stream(dev).cuda_stream
        # the machine's streaming-read rate over the derived-view scan's bytes (ALocal 16, v 8, t 8)
        scan_bytes = (32 * n + 127) // 128 * 128
        buf = torch.zeros(scan_bytes, dtype=torch.uint8, device=dev)
        sink = torch.zeros(1, dtype=torch.int64, device=dev)
        calib_ms = timed(lambda: lib.tbe_calib_device(0, buf.data_ptr(), scan_bytes, scan_bytes // 16, sink.data_ptr(),
                                                      cur), args.repeats)
        del buf
        result["stream_read_MB"] = round(scan_bytes / 1e6, 1)
        result["stream_read_ms"] = round(calib_ms, 4)
        result["stream_read_GB_per_s"] = round(scan_bytes / calib_ms / 1e6, 1)

        eng = ApproximateEngine(n, 5, 2, 10_000_000, 1, zero_wait_slots=1, device=0)
        t = TS - rng.integers(0, 3_000_000, n)
        v = np.where(rng.random(n) < 0.5, 0.0, 4.0 + rng.random(n))    # 4+: worth something for 2 s
        p = rng.uniform(0.5, 1.5, n)
        eng.import_global(v, p, t)
        d_idle = torch.empty(n, dtype=torch.uint8, device=dev)
        zeros = np.zeros(n, dtype=np.int64)

        # a new engine's view is written ({est 1, global 0}): the scan reads AClient
        written_ms = timed(lambda: eng.idle_device(TS, d_idle, stream=cur), args.repeats)
        want = snapshot.approx_idle_rows(zeros, zeros, zeros, v, t, TS, rate)
        assert np.array_equal(d_idle.cpu().numpy(), want.astype(np.uint8))
        result["scan_view_written"] = {"ms": round(written_ms, 4), "idle": int(want.sum()),
                                       "GB_per_s_of_48B_per_key": round(48 * n / written_ms / 1e6, 1)}
        # after a one-client refresh the view is derived from the row
        eng.refresh(TS)
        v, p, t = eng.export_global()
        ts2 = TS + 1_000_000
        lazy_ms = timed(lambda: eng.idle_device(ts2, d_idle, stream=cur), args.repeats)
        want = snapshot.approx_idle_rows(zeros, np.trunc(v).astype(np.int64), zeros, v, t, ts2, rate)
        assert np.array_equal(d_idle.cpu().numpy(), want.astype(np.uint8))
        result["scan_view_derived"] = {"ms": round(lazy_ms, 4), "idle": int(want.sum()),
                                       "GB_per_s_of_32B_per_key": round(32 * n / lazy_ms / 1e6, 1)}

        # snapshot of the rows that are not idle
        d_n = torch.zeros(1, dtype=torch.int64, device=dev)
        count_ms = timed(lambda: eng.export_live_device(ts2, None, None, None, d_n, stream=cur, d_skip=d_idle,
                                                        tier=True), args.repeats)
        live = int(d_n.item())
        rows = snapshot.approx_live_rows(t, ts2, skip=want)
        assert live == rows.shape[0], (live, rows.shape[0])
        d_ids = torch.empty(live, dtype=torch.int64, device=dev)
        d_v = torch.empty(live, dtype=torch.float64, device=dev)
        d_p = torch.empty(live, dtype=torch.float64, device=dev)
        d_t = torch.empty(live, dtype=torch.int64, device=dev)
        fill_ms = timed(lambda: eng.export_live_device(ts2, d_ids, d_v, d_t, d_n, stream=cur, d_p=d_p, d_skip=d_idle),
                        args.repeats)
        assert np.array_equal(d_ids.cpu().numpy(), rows)
        assert np.array_equal(d_p.cpu().numpy().view(np.uint64), p[rows].view(np.uint64))
        import_ms = timed(lambda: eng.import_rows(d_ids, d_v, d_t, stream=cur, d_p=d_p), args.repeats)
        eng.synchronize()
        result["export"] = {"rows": live, "count_ms": round(count_ms, 4),
                            "count_GB_per_s_of_9B_per_key": round(9 * n / count_ms / 1e6, 1),
                            "fill_ms": round(fill_ms, 4), "count_plus_fill_ms": round(count_ms + fill_ms, 4)}
        result["import_rows"] = {"ms": round(import_ms, 4),
                                 "GB_per_s_of_56B_per_row": round(56 * live / import_ms / 1e6, 1)}
        dense = []
        for _ in range(3):
            t1 = time.perf_counter()
            eng.export_global()
            dense.append((time.perf_counter() - t1) * 1e3)
        result["host_export_state_ms"] = round(statistics.median(dense), 2)

        # the reset last: it is the one call that changes the state (the same flags every repeat)
        reset_ms = timed(lambda: eng.reset_device(d_idle, stream=cur), args.repeats)
        flagged = int(want.sum())
        result["reset"] = {"ms": round(reset_ms, 4), "flagged": flagged,
                           "GB_per_s_of_1B_per_key_plus_56B_per_flagged": round((n + 56 * flagged) / reset_ms / 1e6, 1)}
        vr, pr, tr = eng.export_global()
        assert (tr[want] == np.iinfo(np.int64).min).all() and np.array_equal(tr[~want], t[~want])
        eng.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
