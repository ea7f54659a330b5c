#!/usr/bin/env python3
"""Cost of grouping a batch keyed by text for the routing all-to-all (the sender's steps of
cluster.route_text_requests) beside the u64 route of the same batch.

One GPU, no ranks.  --requests names (default 2^22) made by synthetic_key_text from uniform u64
keys below --keys ("resource-<key>", about 20 bytes each), --owners owners (default 8), hash
partition.  Timed with HIP events around --inner calls back to back (default 20, so that a window
lasts milliseconds), ms per call, median of --repeats windows after a warm-up of every call:

  keys     tbe_route_text_keys_device        reads the text and offsets, writes 8 B per string
  plan     tbe_route_plan_map_device         over those keys (the u64 route's own call)
  offsets  tbe_route_text_offsets_device     lengths scattered, scanned, per-owner byte counts
  pack     tbe_route_text_pack_device        the text and the {len, ts_us, permits} rows
  text     the four together
  u64      tbe_route_plan_map_device + tbe_route_pack_device of the u64 keys: yardstick (a)

Yardstick (b): the bytes the four steps must move (`text_bytes`: per step, each input read
once and each output written once) over the 6.29 TB/s an on-device copy reaches on this GPU;
`text_of_copy_rate` is that time over the measured one.  The exchange between GPUs (RCCL) and
the receiver's side (its offsets, the string directory) are not part of this; the exchange
needs more than one GPU and stays unmeasured.  Prints one JSON line and, with --out, writes it.

    python tools/text_route_time.py [--requests 4194304] [--owners 8] [--repeats 5] [--inner 20] [--out profiles/text_route_time.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 6.29e12


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--requests", type=int, default=1 << 22)
    ap.add_argument("--keys", type=int, default=10**9)
    ap.add_argument("--owners", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from distributedratelimiting.redis_amd import _capi, cluster
    from distributedratelimiting.redis_amd.strdir import synthetic_key_text

    if not torch.cuda.is_available():
        raise SystemExit("text_route_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    lib = _capi.load()
    world = args.owners

    def check(st):
        if st != _capi.TBE_OK:
            raise SystemExit(f"a routing call failed: {_capi.STATUS_NAMES.get(st, st)}")

    def run(n: int, repeats: int, inner: int) -> dict:
        st = cluster.device_stream(dev)
        g = torch.Generator(device=dev).manual_seed(11)
        keys = torch.randint(0, args.keys, (n,), dtype=torch.int64, device=dev, generator=g)
        permits = torch.randint(0, 4, (n,), dtype=torch.int32, device=dev, generator=g)
        ts = 1_760_000_000_000_000 + torch.arange(n, dtype=torch.int64, device=dev)
        buf, offs, nb = synthetic_key_text(keys)
        tkeys = torch.empty(n, dtype=torch.int64, device=dev)
        n_bad = torch.zeros(1, dtype=torch.int64, device=dev)
        pos = torch.empty(n, dtype=torch.int32, device=dev)
        counts = torch.zeros(world, dtype=torch.int64, device=dev)
        byte_counts = torch.zeros(world, dtype=torch.int64, device=dev)
        send_offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        out_bytes = torch.empty((nb + 7) // 8 * 8 + 8, dtype=torch.uint8, device=dev)
        rows = torch.empty((n, 3), dtype=torch.int64, device=dev)
        work = torch.empty(max(8, lib.tbe_route_workspace_bytes(n, world), lib.tbe_route_text_workspace_bytes(n)),
                           dtype=torch.uint8, device=dev)
        steps = {
            "keys": lambda: check(lib.tbe_route_text_keys_device(buf.data_ptr(), nb, offs.data_ptr(), n, 0,
                                                                 tkeys.data_ptr(), n_bad.data_ptr(), st)),
            "plan": lambda: check(lib.tbe_route_plan_map_device(tkeys.data_ptr(), n, world, None, work.data_ptr(),
                                                                pos.data_ptr(), counts.data_ptr(), st)),
            "offsets": lambda: check(lib.tbe_route_text_offsets_device(offs.data_ptr(), nb, n, pos.data_ptr(),
                                                                       counts.data_ptr(), world, work.data_ptr(),
                                                                       send_offs.data_ptr(), byte_counts.data_ptr(), st)),
            "pack": lambda: check(lib.tbe_route_text_pack_device(buf.data_ptr(), nb, offs.data_ptr(), n, pos.data_ptr(),
                                                                 send_offs.data_ptr(), permits.data_ptr(), ts.data_ptr(),
                                                                 out_bytes.data_ptr(), out_bytes.numel(), rows.data_ptr(),
                                                                 st)),
        }

        def text():
            for f in steps.values():
                f()

        def u64():
            check(lib.tbe_route_plan_map_device(keys.data_ptr(), n, world, None, work.data_ptr(), pos.data_ptr(),
                                                counts.data_ptr(), st))
            check(lib.tbe_route_pack_device(pos.data_ptr(), n, keys.data_ptr(), permits.data_ptr(), ts.data_ptr(),
                                            rows.data_ptr(), st))

        def timed(fn) -> float:
            """ms per call: one event window around `inner` calls back to back (every call writes
            the same outputs from the same inputs), so that a window lasts milliseconds."""
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / inner

        text()                      # every call once (the steps feed each other), then the u64 route
        u64()
        torch.cuda.synchronize()
        res = {"requests": n, "owners": world, "text_len_mean": round(nb / n, 2), "n_bytes": nb}
        ms = {name: [] for name in list(steps) + ["text", "u64"]}
        for _ in range(repeats):    # alternating, so that drift hits every row alike
            ms["u64"].append(timed(u64))
            ms["text"].append(timed(text))
            for name, f in steps.items():
                ms[name].append(timed(f))
        assert int(n_bad.item()) == 0 and int(send_offs[-1].item()) == nb and int(byte_counts.sum().item()) == nb
        for name, v in ms.items():
            res[f"{name}_ms"] = round(statistics.median(v), 4)
            res[f"{name}_all_ms"] = [round(x, 4) for x in v]
        nt = -(-n // 4096)
        step_bytes = {
            "keys": nb + 8 * (n + 1) + 8 * n,
            "plan": 2 * 8 * n + 4 * n + 2 * 4 * nt * world,
            "offsets": 8 * (n + 1) + 4 * n + 4 * n + 2 * 4 * n + 8 * (n + 1),
            "pack": nb + 8 * (n + 1) + 4 * n + 8 * n + 4 * n + 8 * n + nb + 24 * n,
        }
        res["text_bytes"] = sum(step_bytes.values())
        res["u64_bytes"] = step_bytes["plan"] + 4 * n + 8 * n + 4 * n + 8 * n + 24 * n
        for name, b in step_bytes.items():
            res[f"{name}_of_copy_rate"] = round(b / (res[f"{name}_ms"] * 1e-3) / COPY_RATE, 4)
        res["text_of_copy_rate"] = round(res["text_bytes"] / (res["text_ms"] * 1e-3) / COPY_RATE, 4)
        res["u64_of_copy_rate"] = round(res["u64_bytes"] / (res["u64_ms"] * 1e-3) / COPY_RATE, 4)
        res["text_over_u64"] = round(res["text_ms"] / res["u64_ms"], 3)
        return res

    with torch.cuda.stream(torch.cuda.Stream(dev)):
        run(1 << 16, 2, 2)          # warm-up: code objects loaded, every call once at a small size
        line = run(args.requests, args.repeats, args.inner)
    line["repeats"], line["calls_per_window"] = args.repeats, args.inner
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
