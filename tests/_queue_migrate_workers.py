"""Rank bodies for tests/test_queue_migrate_gloo.py (oracle stand-in engines, gloo on the CPU)
and tests/test_gpu_queue_migrate.py (HIP engines, two ranks on one GPU over gloo): two routed
wait steps with a replenish tick each under the hash partition, cluster.migrate_queueing to
map B of tests/_migrate_workers.py, a routed cancel of requests queued before the move, two
more steps under B.

1000 keys, demand far above the fill rate: 1 token per second per key against about three
requests per key, rank and step.  Request ids are (owner rank << 40) + the owner's counter, so
they stay unique when a queue changes owner.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _dist_workers as W      # noqa: E402
from tests import _migrate_workers as M   # noqa: E402

ABSENT = np.iinfo(np.int64).min
NO = np.uint64(0xFFFFFFFFFFFFFFFF)
N_KEYS, STEPS, N, T0 = 1000, 4, 3000, 1_760_000_000_000_000
# (TokenLimit, TokensPerPeriod, ticks, QueueLimit, order); class of key k is k % 3 when classed
QCLASSES = [(4, 1, 10_000_000, 6, 0), (3, 1, 10_000_000, 5, 1), (6, 2, 10_000_000, 40, 0)]
QUEUED = 2


def batch(rank: int, step: int):
    rng = np.random.default_rng(7000 + 100 * rank + step)
    keys = rng.integers(0, N_KEYS, N, dtype=np.uint64)
    permits = rng.choice(np.array([0, 1, 1, 2, 3], dtype=np.int32), N)
    ts = T0 + step * 700_000 + np.sort(rng.integers(0, 1_000, N))
    return keys, permits, ts.astype(np.int64)


def tick_ts(step: int) -> int:
    return T0 + step * 700_000 + 500_000


def migrate_ts() -> int:
    return T0 + 2 * 700_000


def cancel_pick(status) -> np.ndarray:
    """Of a rank's own requests of a step: every third queued one and a few that are not."""
    return np.array([i for i in range(N) if (i % 3 == 0 and status[i] == QUEUED) or i % 37 == 5], dtype=np.int64)


def classes_of(classed: bool):
    return QCLASSES if classed else QCLASSES[:1]


def tight_rank(world: int):
    """(rank, keys it holds after steps 0-1) of the rank that gains the most keys by map B."""
    from distributedratelimiting.redis_amd import cluster
    keys = np.unique(np.concatenate([batch(r, s)[0] for r in range(world) for s in (0, 1)]))
    old, new = cluster.key_owner(keys, world), cluster.key_owner(keys, world, M.map_b(world))
    gain = [int(((new == r) & (old != r)).sum() - ((old == r) & (new != r)).sum()) for r in range(world)]
    r = int(np.argmax(gain))
    assert gain[r] > 0
    return r, int((old == r).sum())


class OracleQueueEngine:
    """Stand-in with the slice of QueueingTokenBucketEngine that cluster.migrate_queueing's host
    path and the rank bodies use: one oracle.semantics.QueueingTokenBucketTable per class over
    dense ids."""

    def __init__(self, n_keys: int, classes):
        from distributedratelimiting.redis_amd import _capi
        from oracle.semantics import QueueingTokenBucketTable, TokenBucketConfig
        self.KIND = _capi.TBE_KIND_QUEUEING
        self.n_keys = n_keys
        self._classes = [tuple(c) for c in classes]
        self.classed = len(classes) > 1
        self.tables = [QueueingTokenBucketTable(TokenBucketConfig.from_options(*c[:3]), c[3], c[4]) for c in classes]
        self.cls = np.zeros(n_keys, dtype=np.uint8)

    def queue_classes(self):
        return list(self._classes)

    def get_class(self, ids):
        return self.cls[np.asarray(ids, dtype=np.int64)].copy()

    def set_class(self, ids, cls):
        ids, cls = np.asarray(ids, dtype=np.int64).tolist(), np.asarray(cls).tolist()
        if any(self.tables[self.cls[i]].queues.get(i) for i in ids):
            raise ValueError("an id's queue is not empty")
        for i, c in zip(ids, cls):
            if self.cls[i] != c:
                st = self.tables[self.cls[i]].tb.state.pop(i, None)
                if st is not None:
                    self.tables[c].tb.state[i] = st
                self.cls[i] = c

    def wait_batch(self, ids, permits, ts, id_base: int):
        st, rem = [], []
        for j, (i, p, t) in enumerate(zip(np.asarray(ids).tolist(), np.asarray(permits).tolist(),
                                          np.asarray(ts).tolist())):
            s, r, _ = self.tables[self.cls[i]].acquire(int(i), int(p), int(t), id_base + j)
            st.append(s)
            rem.append(r)
        return np.array(st, dtype=np.uint8), np.array(rem, dtype=np.int32), None

    def refresh(self, ts_us: int):
        log = sorted((e for tab in self.tables for e in tab.refresh(ts_us)), key=lambda e: e[0])   # stable: drain order
        a = np.array(log, dtype=np.int64).reshape(-1, 3)
        return a[:, 0].astype(np.uint64), a[:, 1].copy(), a[:, 2].astype(np.int32)

    def cancel(self, ids, request_ids):
        return np.array([int(self.tables[self.cls[i]].cancel(int(i), int(q)))
                         for i, q in zip(np.asarray(ids).tolist(), np.asarray(request_ids).tolist())], dtype=np.uint8)

    def export_state(self):
        v = np.array([self._classes[c][0] for c in self.cls.tolist()], dtype=np.float64)
        t = np.full(self.n_keys, ABSENT, dtype=np.int64)
        for tab in self.tables:
            for i, st in tab.tb.state.items():
                v[i], t[i] = st.v, st.t_us
        return v, t

    def import_state(self, v, t_us, first: int = 0):
        from oracle.semantics import BucketState
        for j, (x, t) in enumerate(zip(np.asarray(v).tolist(), np.asarray(t_us).tolist())):
            i = first + j
            tab = self.tables[self.cls[i]].tb
            if t == ABSENT:
                tab.state.pop(i, None)
            else:
                tab.state[i] = BucketState(x, t)

    def queue_of(self, i: int):
        return self.tables[self.cls[i]].queue_of(int(i))

    def queue_export_ids(self, ids, clear: bool = False, capacity=None):
        ids = np.asarray(ids, dtype=np.int64).tolist()
        qs = [self.queue_of(i) for i in ids]
        qcount = np.array([len(q) for q in qs], dtype=np.uint32)
        start = np.zeros(len(ids) + 1, dtype=np.uint64)
        start[1:] = np.cumsum(qcount, dtype=np.uint64)
        ent = np.array([(r << 16) | p for q in qs for r, p in q], dtype=np.uint64)
        total = int(start[-1])
        if capacity is None:
            capacity = total
        if clear:
            if total > capacity:
                raise ValueError("entries do not fit in capacity")
            for i in ids:
                tab = self.tables[self.cls[i]]
                tab.queues.pop(i, None)
                tab.qsum.pop(i, None)
        return qcount, start, ent[:capacity], total

    def queue_import_ids(self, ids, qcount, entries):
        from oracle.semantics import QueueEntry
        ids, qcount = np.asarray(ids, dtype=np.int64).tolist(), np.asarray(qcount, dtype=np.int64).tolist()
        entries = np.asarray(entries, dtype=np.uint64).tolist()
        if sum(qcount) != len(entries):
            raise ValueError("the counts do not sum to n_entries")
        at, plan = 0, []
        for i, c in zip(ids, qcount):
            tl, _, _, ql, _ = self._classes[self.cls[i]]
            q = [QueueEntry(e >> 16, e & 0xFFFF) for e in entries[at:at + c]]
            at += c
            if self.queue_of(i) or c > max(1, ql) or any(not 1 <= e.permits <= tl or e.request_id >> 47 for e in q) \
                    or sum(e.permits for e in q) > ql:
                raise ValueError("an id's queue is not empty, or its entries break its class's limits")
            plan.append((i, q))
        for i, q in plan:
            tab = self.tables[self.cls[i]]
            tab.queues[i], tab.qsum[i] = q, sum(e.permits for e in q)

    def synchronize(self):
        pass

    def close(self):
        pass


def _dump(engine, directory, world, torch=None, dev=None):
    """The engine's rows and, of all keys, those the directory holds with their ids and queues."""
    from distributedratelimiting.redis_amd import cluster
    engine.synchronize()
    v, t = engine.export_state()
    keys = np.arange(N_KEYS, dtype=np.uint64)
    if isinstance(directory, cluster.DeviceDirectory):
        ids = directory.lookup(torch.from_numpy(keys.view(np.int64)).to(dev)).cpu().numpy().view(np.uint64)
    else:
        ids = directory.lookup(keys)
    have = ids != NO
    qcount, _, ent, _ = engine.queue_export_ids(ids[have])
    return {"v": np.asarray(v).copy(), "t": np.asarray(t).copy(), "dir_keys": keys[have], "dir_ids": ids[have],
            "dir_size": np.int64(directory.size()), "q_count": qcount, "q_entries": ent}


def _run(rank, world, out_dir, case, engine, directory, wait, cancel, to_dev, to_host, keys_of, torch=None, dev=None):
    """wait(local ids, permits, ts) -> (status, remaining, request ids) and cancel(local ids,
    request ids) -> hits run on the owner; keys_of(local ids u64 array) -> global keys."""
    from distributedratelimiting.redis_amd import cluster
    mb = M.map_b(world)
    out = {}

    def step(s, omap):
        k, p, t = (to_dev(x) for x in batch(rank, s))
        st, rem, ids = cluster.route_batch(wait, k, p, t, directory, owner_map=omap)
        out[f"st{s}"], out[f"rem{s}"], out[f"ids{s}"] = to_host(st), to_host(rem), to_host(ids).astype(np.int64)
        lk, li, lr = engine.refresh(tick_ts(s))
        out[f"log{s}"] = np.stack([keys_of(lk).astype(np.int64), np.asarray(li, dtype=np.int64),
                                   np.asarray(lr, dtype=np.int64)], axis=1).reshape(-1, 3)

    step(0, None)
    step(1, None)
    if case == "tight":
        before = _dump(engine, directory, world, torch, dev)
        try:
            cluster.migrate_queueing(engine, directory, mb, migrate_ts())
            raised = 0
        except ValueError:
            raised = 1
        after = _dump(engine, directory, world, torch, dev)
        out.update({f"before_{k}": x for k, x in before.items()})
        out.update({f"after_{k}": x for k, x in after.items()})
        out["raised"] = np.int64(raised)
    else:
        out["moved"] = np.array(cluster.migrate_queueing(engine, directory, mb, migrate_ts()), dtype=np.int64)
        # cancel requests this rank issued before the move, wherever their keys live now
        ck, ci = [], []
        for s in (0, 1):
            pick = cancel_pick(out[f"st{s}"])
            ck.append(batch(rank, s)[0][pick])
            ci.append(out[f"ids{s}"][pick])
        ck, ci = np.concatenate(ck), np.concatenate(ci)
        out["hit"] = to_host(cluster.route_cancel(cancel, to_dev(ck), to_dev(ci), directory, owner_map=mb))
        step(2, mb)
        step(3, mb)
        out.update(_dump(engine, directory, world, torch, dev))
    np.savez(os.path.join(out_dir, f"qmig_{rank}.npz"), **out)


def _capacity(rank: int, world: int, case: str) -> int:
    from distributedratelimiting.redis_amd import cluster
    if case == "tight":
        r, held = tight_rank(world)
        if rank == r:
            return held          # room for what it holds, none for what map B adds
    return cluster.keys_per_rank(N_KEYS, world)


def queue_migrate_worker(rank: int, world: int, port: int, out_dir: str, case: str = "ok", classed: str = "plain"):
    """Oracle stand-in engines, HostDirectory, numpy batches over gloo."""
    dist = W._init(rank, world, port)
    from distributedratelimiting.redis_amd import cluster
    cap = _capacity(rank, world, case)
    classes = classes_of(classed == "classed")
    engine = OracleQueueEngine(cap, classes)
    directory = cluster.HostDirectory(cap)
    next_id = [rank << 40]

    def keys_of(ids):
        key_of = {i: k for k, i in directory.ids.items()}
        return np.array([key_of[i] for i in np.asarray(ids, dtype=np.uint64).tolist()], dtype=np.uint64)

    def wait(lk, lp, lt):
        if engine.classed and lk.shape[0]:   # a key new to this owner: its class before its first request
            want = (keys_of(lk) % np.uint64(3)).astype(np.uint8)
            new = engine.get_class(lk) != want
            engine.set_class(lk[new], want[new])
        base = next_id[0]
        next_id[0] += lk.shape[0]
        st, rem, _ = engine.wait_batch(lk, lp, lt, base)
        return st, rem, base + np.arange(lk.shape[0], dtype=np.int64)

    _run(rank, world, out_dir, case, engine, directory, wait, engine.cancel, lambda x: x, lambda x: np.asarray(x),
         keys_of)
    dist.barrier()
    dist.destroy_process_group()


def queue_migrate_worker_hip(rank: int, world: int, port: int, out_dir: str, path: str, case: str = "ok",
                             classed: str = "plain"):
    """HIP engines on cuda:0; path "host": numpy batches, HostDirectory, host-buffer engine
    calls; path "device": CUDA tensors end to end with a DeviceDirectory."""
    dist = W._init(rank, world, port)
    torch, dev, stream = W._hip_setup()
    from distributedratelimiting.redis_amd import QueueingTokenBucketEngine, cluster
    cap = _capacity(rank, world, case)
    c = classed == "classed"
    classes = classes_of(c)
    engine = QueueingTokenBucketEngine(cap, *classes[0], device=0, classes=classes[1:] if c else None)
    next_id = [rank << 40]
    device = path == "device"
    directory = cluster.DeviceDirectory(cap, device=0) if device else cluster.HostDirectory(cap)

    def keys_of(ids):
        ids = np.asarray(ids, dtype=np.uint64)
        if device:
            return directory.keys_of(torch.from_numpy(ids.view(np.int64).copy()).to(dev)).cpu().numpy().view(np.uint64)
        key_of = {i: k for k, i in directory.ids.items()}
        return np.array([key_of[i] for i in ids.tolist()], dtype=np.uint64)

    def wait(lk, lp, lt):
        m = lk.shape[0]
        base = next_id[0]
        next_id[0] += m
        if device:
            if c and m:
                want = (directory.keys_of(lk) % 3).to(torch.uint8)
                have = torch.empty(m, dtype=torch.uint8, device=dev)
                engine.get_class_device(lk.contiguous(), have, stream=stream.cuda_stream)
                new = torch.nonzero(have != want).flatten()
                if new.numel():
                    engine.set_class_device(torch.unique(lk[new]), (directory.keys_of(torch.unique(lk[new])) % 3)
                                            .to(torch.uint8), stream=stream.cuda_stream)
            st = torch.empty(m, dtype=torch.uint8, device=dev)
            rem = torch.empty(m, dtype=torch.int32, device=dev)
            if m:
                engine.wait_batch_device(lk, lp, lt, st, rem, base, wait=True, stream=stream.cuda_stream)
            return st, rem, base + torch.arange(m, dtype=torch.int64, device=dev)
        if c and m:
            want = (keys_of(lk) % np.uint64(3)).astype(np.uint8)
            new = engine.get_class(lk) != want
            engine.set_class(lk[new], want[new])
        st, rem, _ = engine.wait_batch(lk, lp, lt, base)
        return st, rem, base + np.arange(m, dtype=np.int64)

    def cancel(lk, ids):    # host-buffer cancel (tbe_queue_cancel); device inputs staged
        if device:
            engine.synchronize()
            return engine.cancel(lk.cpu().numpy().view(np.uint64), ids.cpu().numpy())
        return engine.cancel(lk, ids)

    if device:
        def to_dev(x):
            x = np.asarray(x)
            return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)

        _run(rank, world, out_dir, case, engine, directory, wait, cancel, to_dev, lambda x: x.cpu().numpy(), keys_of,
             torch, dev)
    else:
        _run(rank, world, out_dir, case, engine, directory, wait, cancel, lambda x: x, lambda x: np.asarray(x), keys_of)
    engine.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    # python tests/_queue_migrate_workers.py <worker> <rank> <world> <port> <out_dir> [args]
    fn = globals()[sys.argv[1]]
    fn(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), *sys.argv[5:])
