#!/usr/bin/env python3
"""Cost of a live owner-map change on one owner (cluster.migrate's local steps) beside the
snapshot route, the only way to change a map before tbe_migrate_out_device existed.

One GPU, no ranks.  A TokenBucketEngine and a DeviceDirectory hold --keys live keys (default
2^26); the change is n_owners = 2, self = 0 and map B (the hash owner map with every odd
virtual node moved to the other owner), which gives about half of the keys away.  Timed, HIP
events around each call, after a warm-up of every call on a small engine:

  count    migrate_out_device, counting and flagging only (capacity 0)       median of --repeats
  commit   migrate_out_device(commit) into a buffer of the counted size      median of --repeats
           (the rows are put back with import_rows between repeats)
  reclaim  the source directory's reclaim_device(leaving flags)              once
  install  assign + import_rows of the packed rows on a second engine and
           directory on the same GPU                                        once
  snapshot snapshot.save of the same table, then snapshot.load(owner=...)
           of the file into fresh engines for both new owners               once (host clock)

Bytes a migrate_out pass must move: 16 B per row of the table and 8 B per id of the key-of-id
table, plus 32 B per row sent; the count call is one such pass, the commit call two (count,
write) plus the clearing pass (8 B per id, 16 B per leaving row).  `of_copy_rate` is those
bytes over the call's time as a fraction of the 6.29 TB/s an on-device copy reaches on this GPU.
The exchange between owners (RCCL) is not part of this: it needs more than one GPU.
Prints one JSON line and, with --out, writes it to that file (profiles/).

    python tools/migrate_time.py [--keys 67108864] [--repeats 5] [--no-snapshot] [--out profiles/migrate_time.json]

--text: the same change for text-keyed buckets (cluster.migrate with a StringDirectory).  The
engine's ids are held by --keys names ``resource-<k>`` (strdir.synthetic_key_text) in a
StringDirectory, every row live.  Each of the --repeats rounds runs the local steps of one
rank once, each between HIP events, and the medians are reported:

  route_keys  StringDirectory.route_keys: iloc and the arena text in, 8 B per id out
  count       migrate_out_device over the routing keys, counting and flagging only
  pack        migrate_out_device(capacity = rows, row_ids): rows and their ids, no commit
  text        the rows' text (StringDirectory.text_of): tbe_sdir_text_lengths_device, a scan, one
              read-back of the byte total, a zero-filled buffer, tbe_sdir_text_device
  commit      migrate_out_device(commit) into the same row buffer
  reclaim     reclaim_device(leaving flags)
  install     the receiver's side, on the same directory and engine: assign of the packed text
              (into the ids the reclaim freed, beside the names that stayed) + import_rows

The install puts every name and row back under other ids, so the next round finds the same
table.  Bytes: what each step must read and write at least (see the code); `of_copy_rate` as
above.  Single-GPU local steps only: the three exchanges need more than one GPU.

    python tools/migrate_time.py --text [--keys 67108864] [--repeats 5] [--out profiles/migrate_text_time.json]

--queue: the same change for a queueing engine (cluster.migrate_queueing's local steps): a
QueueingTokenBucketEngine with QueueLimit 16 whose --keys queues are all saturated (sixteen
one-permit entries each, put there with queue_import_ids_device), every row live.  Each of the
--repeats rounds runs one rank's local steps once, each between HIP events; medians are reported:

  count    queue_migrate_out_device, counting and flagging only
  commit   queue_migrate_out_device(commit) with the rows' ids
  export   queue_export_ids_device(row ids, clear) into a buffer of 16 entries per row
  reclaim  reclaim_device(leaving flags)
  install  the receiver's side, on the same directory and engine: assign (into the ids the
           reclaim freed) + import_rows + queue_import_ids_device

The install puts every key, row and queue back, so the next round finds the same table.  The
token-bucket figures of the default mode at the same --keys (without the snapshot route) are
measured in the same run and stored under "token_bucket".

    python tools/migrate_time.py --queue [--keys 4194304] [--repeats 5] [--out profiles/migrate_queue_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 6.29e12
TS = 1_760_000_100_000_000
OPTS = (5, 1, 10_000_000)      # TTL 5 s


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keys", type=int, default=1 << 26)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-snapshot", action="store_true")
    ap.add_argument("--text", action="store_true", help="text-keyed buckets behind a StringDirectory")
    ap.add_argument("--queue", action="store_true", help="a queueing engine with saturated queues")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from distributedratelimiting.redis_amd import TokenBucketEngine, cluster, snapshot

    if not torch.cuda.is_available():
        raise SystemExit("migrate_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    world, me = 2, 0
    map_b = cluster.hash_owner_map(world).astype(np.int64)
    map_b[1::2] = (map_b[1::2] + 1) % world
    map_b = map_b.astype(np.uint8)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    def run(n: int, repeats: int, with_snapshot: bool) -> dict:
        cur = torch.cuda.current_stream(dev).cuda_stream
        eng, directory = TokenBucketEngine(n, *OPTS, device=0), cluster.DeviceDirectory(n, device=0)
        keys = torch.arange(n, dtype=torch.int64, device=dev)
        g = torch.Generator(device=dev).manual_seed(7)
        v = torch.rand(n, dtype=torch.float64, device=dev, generator=g) * OPTS[0]
        t = TS - torch.randint(0, 2_000_000, (n,), dtype=torch.int64, device=dev, generator=g)   # every row live
        ids = directory.assign(keys)
        directory.check()
        eng.import_rows(ids, v, t, stream=cur)
        eng.synchronize()
        dmap = torch.from_numpy(map_b).to(dev)
        kof = directory.keys_of(torch.arange(n, dtype=torch.int64, device=dev))
        counts = torch.zeros(world + 2, dtype=torch.int64, device=dev)
        leaving = torch.empty(n, dtype=torch.uint8, device=dev)
        res = {"keys": n}
        ms = [timed(lambda: eng.migrate_out_device(TS, kof, dmap, world, me, None, counts, leaving, stream=cur))[0]
              for _ in range(repeats)]
        c = counts.tolist()
        n_rows, n_leave = sum(c[:world]), c[world]
        assert c[world + 1] == 0 and n_rows == n_leave
        rows = torch.empty((n_rows, 4), dtype=torch.int64, device=dev)
        res.update(rows_sent=n_rows, count_ms=round(statistics.median(ms), 4), count_all_ms=[round(x, 4) for x in ms])
        ms = []
        for r in range(repeats):
            ms.append(timed(lambda: eng.migrate_out_device(TS, kof, dmap, world, me, rows, counts, leaving, commit=True,
                                                           capacity=n_rows, stream=cur))[0])
            eng.synchronize()
            if r + 1 < repeats:     # put the cleared rows back for the next repeat
                eng.import_rows(ids, v, t, stream=cur)
                eng.synchronize()
        res.update(commit_ms=round(statistics.median(ms), 4), commit_all_ms=[round(x, 4) for x in ms])
        res["reclaim_ms"] = round(timed(lambda: directory.reclaim_device(leaving))[0], 4)
        assert directory.size() == n - n_leave
        # the receiving side: a second engine and directory on the same GPU
        eng2, dir2 = TokenBucketEngine(n, *OPTS, device=0), cluster.DeviceDirectory(n, device=0)

        def install():
            rid = dir2.assign(rows[:, 0].contiguous())
            eng2.import_rows(rid, rows[:, 1].contiguous().view(torch.float64), rows[:, 2].contiguous(), stream=cur)
        res["install_ms"] = round(timed(install)[0], 4)
        eng2.synchronize()
        assert dir2.size() == n_rows
        eng2.close()
        dir2.close()
        count_bytes = 24 * n + n
        commit_bytes = count_bytes + 24 * n + 32 * n_rows + 8 * n + 16 * n_leave
        res.update(count_bytes=count_bytes, commit_bytes=commit_bytes,
                   count_of_copy_rate=round(count_bytes / (res["count_ms"] * 1e-3) / COPY_RATE, 4),
                   commit_of_copy_rate=round(commit_bytes / (res["commit_ms"] * 1e-3) / COPY_RATE, 4),
                   migrate_local_ms=round(res["count_ms"] + res["commit_ms"] + res["reclaim_ms"] + res["install_ms"], 4))
        if with_snapshot:
            # the same change by the snapshot route: the table as it was before the commit
            eng.import_rows(ids, v, t, stream=cur)
            eng.synchronize()
            old = cluster.DeviceDirectory(n, device=0)
            old.assign(keys)
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "owner0.npz")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                snapshot.save(path, eng, TS, old)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                res["snapshot_file_bytes"] = os.path.getsize(path)
                eng.close()
                old.close()
                for owner in range(world):
                    e, d = TokenBucketEngine(n, *OPTS, device=0), cluster.DeviceDirectory(n, device=0)
                    snapshot.load(path, e, d, owner=(owner, world, map_b), stream=cur)
                    e.synchronize()
                    e.close()
                    d.close()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
            res.update(snapshot_save_ms=round((t1 - t0) * 1e3, 1), snapshot_load_ms=round((t2 - t1) * 1e3, 1),
                       snapshot_ms=round((t2 - t0) * 1e3, 1))
            res["snapshot_over_migrate"] = round(res["snapshot_ms"] / res["migrate_local_ms"], 1)
        else:
            eng.close()
        directory.close()
        return res

    def run_text(n: int, repeats: int) -> dict:
        from distributedratelimiting.redis_amd import _capi
        from distributedratelimiting.redis_amd.strdir import StringDirectory, synthetic_key_text
        lib = _capi.load()
        cur = torch.cuda.current_stream(dev).cuda_stream
        buf, offs, nb = synthetic_key_text(torch.arange(n, dtype=torch.int64, device=dev))
        arena = int(((offs[1:] - offs[:-1] + 7) & ~7).sum().item())
        eng, directory = TokenBucketEngine(n, *OPTS, device=0), StringDirectory(n, arena + (1 << 20), device=0)
        g = torch.Generator(device=dev).manual_seed(7)
        v = torch.rand(n, dtype=torch.float64, device=dev, generator=g) * OPTS[0]
        t = TS - torch.randint(0, 2_000_000, (n,), dtype=torch.int64, device=dev, generator=g)   # every row live
        ids = directory.assign(buf, offs, nb)
        assert directory.usage()[:2] == (n, arena)
        eng.import_rows(ids, v, t, stream=cur)
        eng.synchronize()
        del buf, offs, ids, v, t
        dmap = torch.from_numpy(map_b).to(dev)
        counts = torch.zeros(world + 2, dtype=torch.int64, device=dev)
        leaving = torch.empty(n, dtype=torch.uint8, device=dev)
        steps = ("route_keys", "count", "pack", "text", "commit", "reclaim", "install")
        ms = {k: [] for k in steps}
        for _ in range(repeats):
            dt, rk = timed(lambda: directory.route_keys(0))
            ms["route_keys"].append(dt)
            ms["count"].append(timed(lambda: eng.migrate_out_device(TS, rk, dmap, world, me, None, counts, leaving,
                                                                    stream=cur))[0])
            c = counts.tolist()
            n_rows, n_leave = sum(c[:world]), c[world]
            assert c[world + 1] == 0 and n_rows == n_leave
            rows = torch.empty((n_rows, 4), dtype=torch.int64, device=dev)
            row_ids = torch.empty(n_rows, dtype=torch.int64, device=dev)
            ms["pack"].append(timed(lambda: eng.migrate_out_device(TS, rk, dmap, world, me, rows, counts, None,
                                                                   capacity=n_rows, stream=cur, row_ids=row_ids))[0])
            dt, (sbuf, soffs) = timed(lambda: directory.text_of(row_ids))
            ms["text"].append(dt)
            n_bytes = int(soffs[-1].item())
            room = int(((soffs[1:] - soffs[:-1] + 7) & ~7).sum().item())
            ms["commit"].append(timed(lambda: eng.migrate_out_device(TS, rk, dmap, world, me, rows, counts, leaving,
                                                                     commit=True, capacity=n_rows, stream=cur))[0])
            eng.synchronize()
            ms["reclaim"].append(timed(lambda: directory.reclaim_device(leaving))[0])
            assert directory.usage()[:2] == (n - n_leave, arena - room)

            def install():
                rid = directory.assign(sbuf, soffs, n_bytes)
                eng.import_rows(rid, rows[:, 1].contiguous().view(torch.float64), rows[:, 2].contiguous(), stream=cur)
            ms["install"].append(timed(install)[0])
            eng.synchronize()
            assert directory.usage()[:2] == (n, arena)
            del rk, rows, row_ids, sbuf, soffs
        ns = 1
        while ns < 2 * n:
            ns <<= 1
        stay = n - n_leave
        count_bytes = 24 * n + n
        # at least: per step, the arrays it must read and write once
        nbytes = {
            "route_keys": 16 * n + arena,                             # iloc, the padded text, the keys
            "count": count_bytes,
            "pack": count_bytes + 24 * n + 40 * n_rows,               # count pass, row pass, rows + ids out
            # lengths (ids, iloc in, lens out), scan, bytes (ids, iloc, offsets in), zero fill, text in and out
            "text": 24 * n_rows + 16 * n_rows + 24 * n_rows + 3 * n_bytes,
            "commit": count_bytes + 24 * n + 32 * n_rows + 8 * n + 16 * n_leave,
            "reclaim": 9 * n + 8 * n_leave + 20 * ns + 2 * (arena - room) + 40 * stay + 16 * ns + 20 * stay,
            "install": 2 * n_bytes + 16 * n_rows + room + 20 * n_rows + 40 * n_rows,
        }
        res = {"keys": n, "rows_sent": n_rows, "text_bytes_sent": n_bytes, "arena_bytes": arena, "arena_bytes_sent": room}
        for k in steps:
            med = statistics.median(ms[k])
            res[f"{k}_ms"] = round(med, 4)
            res[f"{k}_all_ms"] = [round(x, 4) for x in ms[k]]
            res[f"{k}_bytes"] = nbytes[k]
            res[f"{k}_of_copy_rate"] = round(nbytes[k] / (med * 1e-3) / COPY_RATE, 4)
        res["migrate_local_ms"] = round(sum(res[f"{k}_ms"] for k in steps), 4)
        eng.close()
        directory.close()
        return res

    QL = 16

    def run_queue(n: int, repeats: int) -> dict:
        from distributedratelimiting.redis_amd import QueueingTokenBucketEngine
        cur = torch.cuda.current_stream(dev).cuda_stream
        eng, directory = QueueingTokenBucketEngine(n, *OPTS, QL, 0, device=0), cluster.DeviceDirectory(n, device=0)
        keys = torch.arange(n, dtype=torch.int64, device=dev)
        g = torch.Generator(device=dev).manual_seed(7)
        v = torch.rand(n, dtype=torch.float64, device=dev, generator=g) * OPTS[0]
        t = TS - torch.randint(0, 2_000_000, (n,), dtype=torch.int64, device=dev, generator=g)   # every row live
        ids = directory.assign(keys)
        directory.check()
        eng.import_rows(ids, v, t, stream=cur)
        full = torch.full((n,), QL, dtype=torch.int32, device=dev)
        words = (torch.arange(n * QL, dtype=torch.int64, device=dev) << 16) | 1
        eng.queue_import_ids_device(ids, full, words, stream=cur)
        eng.synchronize()
        del keys, v, t, words
        dmap = torch.from_numpy(map_b).to(dev)
        counts = torch.zeros(world + 2, dtype=torch.int64, device=dev)
        leaving = torch.empty(n, dtype=torch.uint8, device=dev)
        n_out = torch.zeros(1, dtype=torch.int64, device=dev)
        steps = ("count", "commit", "export", "reclaim", "install")
        ms = {k: [] for k in steps}
        for _ in range(repeats):
            kof = directory.keys_of(torch.arange(n, dtype=torch.int64, device=dev))
            ms["count"].append(timed(lambda: eng.queue_migrate_out_device(TS, kof, dmap, world, me, None, counts,
                                                                          leaving, stream=cur))[0])
            c = counts.tolist()
            n_rows, n_leave = sum(c[:world]), c[world]
            assert c[world + 1] == 0 and n_rows == n_leave
            rows = torch.empty((n_rows, 4), dtype=torch.int64, device=dev)
            row_ids = torch.empty(n_rows, dtype=torch.int64, device=dev)
            qcount = torch.empty(n_rows, dtype=torch.int32, device=dev)
            entries = torch.empty(n_rows * QL, dtype=torch.int64, device=dev)
            ms["commit"].append(timed(lambda: eng.queue_migrate_out_device(
                TS, kof, dmap, world, me, rows, counts, leaving, commit=True, capacity=n_rows, stream=cur,
                row_ids=row_ids))[0])
            ms["export"].append(timed(lambda: eng.queue_export_ids_device(row_ids, qcount, None, entries, n_out,
                                                                          clear=True, stream=cur))[0])
            eng.synchronize()
            n_ent = int(n_out.item())
            assert n_ent == n_rows * QL
            ms["reclaim"].append(timed(lambda: directory.reclaim_device(leaving))[0])
            assert directory.size() == n - n_leave

            def install():
                rid = directory.assign(rows[:, 0].contiguous())
                eng.import_rows(rid, rows[:, 1].contiguous().view(torch.float64), rows[:, 2].contiguous(), stream=cur)
                eng.queue_import_ids_device(rid, qcount, entries, stream=cur)
            ms["install"].append(timed(install)[0])
            eng.synchronize()
            assert directory.size() == n
            del kof, rows, row_ids, qcount, entries
        hdr = 4                                                       # QueueLimit 16: 32-bit headers
        count_bytes = (24 + hdr + 1) * n
        # at least: per step, the arrays it must read and write once per pass
        nbytes = {
            "count": count_bytes,
            "commit": count_bytes + (24 + hdr) * n + 40 * n_rows + 8 * n + 16 * n_leave,
            # ids and headers in two passes, counts out, ring words in, entries out, headers cleared
            "export": 2 * (8 + hdr) * n_rows + 4 * n_rows + 16 * n_ent + hdr * n_rows,
            "reclaim": 9 * n + 8 * n_leave,
            # assign (keys in, ids out), import_rows (ids, v, t in; rows out), queue import: counts in three
            # passes, ids and headers in two, entries in twice, ring words and headers out
            "install": 16 * n_rows + 40 * n_rows + 12 * n_rows + 2 * (8 + hdr) * n_rows + 16 * n_ent + 8 * n_ent
                       + hdr * n_rows,
        }
        res = {"keys": n, "queue_limit": QL, "rows_sent": n_rows, "entries_sent": n_ent}
        for k in steps:
            med = statistics.median(ms[k])
            res[f"{k}_ms"] = round(med, 4)
            res[f"{k}_all_ms"] = [round(x, 4) for x in ms[k]]
            res[f"{k}_bytes"] = nbytes[k]
            res[f"{k}_of_copy_rate"] = round(nbytes[k] / (med * 1e-3) / COPY_RATE, 4)
        res["migrate_local_ms"] = round(sum(res[f"{k}_ms"] for k in steps), 4)
        eng.close()
        directory.close()
        return res

    with torch.cuda.stream(torch.cuda.Stream(dev)):
        if args.queue:
            run_queue(1 << 14, 2)                      # warm-up: every call at a small size
            line = run_queue(args.keys, args.repeats)
            run(1 << 16, 2, False)
            line["token_bucket"] = run(args.keys, args.repeats, False)
        elif args.text:
            run_text(1 << 16, 2)                       # warm-up: every call at a small size
            line = run_text(args.keys, args.repeats)
        else:
            run(1 << 16, 2, not args.no_snapshot)      # warm-up: every call once at a small size
            line = run(args.keys, args.repeats, not args.no_snapshot)
    line["repeats"] = args.repeats
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
