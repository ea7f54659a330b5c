#!/usr/bin/env python3
"""Cost of deciding RetryAfter on the device (tbe_approx_acquire_batch_retry_device) against
the batch without it (tbe_approx_acquire_batch_device), and against what it replaces: one
tbe_approx_query round trip per denied key.

Config E's shape per client: --batch (2^25) AcquireCore requests over --keys (1e7) keys,
--token-limit 100, the trace of bench.py --workload approx.  That trace grants everything
(3.4 one-permit requests per key and batch against 100 tokens, refreshed every batch); a
smaller --token-limit (2) makes the same trace denial-heavy.  Two twin engines take the same
batches, one through each entry point, on one stream; a one-client refresh follows every
batch (so the client view is lazy and the new entry point's next batch also writes it).
Per batch, HIP events around the one call; median over --repeats batches after --warm.  The
first batch after each refresh ("after_refresh") and the same batch again without a refresh
in between ("steady": the view is already written) are timed separately.  Status and
available of the twins are compared after every batch.  Prints one JSON line.

    python tools/retry_after_time.py [--keys 10000000] [--batch 33554432] [--token-limit 100] [--repeats 7]
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
    ap.add_argument("--batch", type=int, default=1 << 25)
    ap.add_argument("--token-limit", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--queries", type=int, default=1000)
    args = ap.parse_args()
    import torch
    from bench_kinds import SEED_E, T0_US, _gen
    from distributedratelimiting.redis_amd import ApproximateEngine, _capi

    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    lib = _capi.load()
    n, interval_us = args.batch, 10_000
    mk = lambda: ApproximateEngine(args.keys, args.token_limit, 10, interval_us * 10, 0, 0, device=0, max_batch=n)
    old, new = mk(), mk()
    outs = {e: (torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
            for e in (old, new)}
    ticks = torch.empty(n, dtype=torch.int64, device=dev)
    times = {"old": {"after_refresh": [], "steady": []}, "new": {"after_refresh": [], "steady": []}}
    failed_share = []
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        cur = torch.cuda.current_stream(dev).cuda_stream

        def call(eng, k, p, s):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st, av = outs[eng]
            a.record()
            eng.acquire_batch_device(k, p, st, av, wait=False, id_base=s * n, stream=cur,
                                     **({"d_retry_after": ticks} if eng is new else {}))
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b)

        for s in range(args.warm + args.repeats):
            k, p, _ = _gen(lib, SEED_E, args.keys, s, n, interval_us, dev)
            torch.cuda.synchronize()
            for phase in ("after_refresh", "steady"):
                t_old, t_new = call(old, k, p, s), call(new, k, p, s)
                assert torch.equal(outs[old][0], outs[new][0]) and torch.equal(outs[old][1], outs[new][1])
                failed = outs[new][0] == 0
                assert bool(((ticks >= 0) == failed).all())
                if s >= args.warm:
                    times["old"][phase].append(t_old)
                    times["new"][phase].append(t_new)
                    if phase == "after_refresh":
                        failed_share.append(float(failed.float().mean().item()))
            for e in (old, new):
                e.refresh(T0_US + (s + 1) * interval_us)
        # the alternative: one tbe_approx_query per denied key (a stream synchronisation, the
        # one-key derive launch after a one-client refresh, two copies), wall clock; keys of
        # denied requests where the batch has enough of them (the call costs the same on any key)
        denied = torch.nonzero(outs[old][0] == 0).flatten()[: args.queries * 50]
        dk = torch.unique(k[denied])[: args.queries].cpu().tolist()
        queried = "denied keys"
        if len(dk) < args.queries:
            dk, queried = torch.unique(k[: args.queries * 50])[: args.queries].cpu().tolist(), "keys of the batch"
        t1 = time.perf_counter()
        for key in dk:
            old.local_state(key)
        query_ms = (time.perf_counter() - t1) * 1e3
    med = {w: {ph: round(statistics.median(v), 4) for ph, v in d.items()} for w, d in times.items()}
    print(json.dumps({
        "keys": args.keys, "batch": n, "token_limit": args.token_limit, "repeats": args.repeats,
        "failed_share": round(statistics.median(failed_share), 4),
        "old_ms": med["old"], "new_ms": med["new"],
        "extra_ms": {ph: round(med["new"][ph] - med["old"][ph], 4) for ph in med["new"]},
        "query_round_trips": {"keys": len(dk), "which": queried, "total_ms": round(query_ms, 2),
                              "ms_per_key": round(query_ms / max(1, len(dk)), 4)},
    }), flush=True)
    old.close()
    new.close()


if __name__ == "__main__":
    main()
