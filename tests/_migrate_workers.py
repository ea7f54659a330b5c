"""Rank bodies for tests/test_migrate_gloo.py (oracle stand-in engines, gloo on the CPU) and
tests/test_gpu_migrate.py (HIP engines, two ranks on one GPU over gloo): route two steps
under the hash partition, cluster.migrate to map B, route two more steps under B.

The stream is tests/_dist_workers.py's (TB, tb_batch): 1000 keys, 4 steps of 3000 requests
per rank.  Map B = the hash owner map with every odd virtual node moved to the next owner.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _dist_workers as W   # noqa: E402

ABSENT = np.iinfo(np.int64).min
NO = np.uint64(0xFFFFFFFFFFFFFFFF)
# class of key k is k % 3; class 0 is W.TB's own options (TTLs 5 s, 5 s, 2 s)
CLASSES = [(W.TB["token_limit"], W.TB["tokens_per_period"], W.TB["period_ticks"]), (9, 2, 10_000_000),
           (3, 1, 5_000_000)]
LAPSE_SHIFT = 6_000_000


def map_b(world: int) -> np.ndarray:
    from distributedratelimiting.redis_amd import cluster
    m = cluster.hash_owner_map(world).astype(np.int64)
    m[1::2] = (m[1::2] + 1) % world
    return m.astype(np.uint8)


def batch(rank: int, step: int, shift: int = 0):
    """W.tb_batch with steps 2.. stamped `shift` us later."""
    k, p, t = W.tb_batch(rank, step)
    return k, p, (t + shift if step >= 2 else t)


def migrate_ts(world: int, shift: int = 0) -> int:
    """The first timestamp of step 2 on any rank (every rank computes the same one)."""
    return int(min(batch(r, 2, shift)[2][0] for r in range(world)))


def touched(world: int, steps) -> np.ndarray:
    return np.unique(np.concatenate([W.tb_batch(r, s)[0] for r in range(world) for s in steps]))


def tight_rank(world: int):
    """(rank, keys it holds after steps 0-1) of the rank that gains the most keys by map B."""
    from distributedratelimiting.redis_amd import cluster
    keys = touched(world, (0, 1))
    old, new = cluster.key_owner(keys, world), cluster.key_owner(keys, world, map_b(world))
    gain = [int(((new == r) & (old != r)).sum() - ((old == r) & (new != r)).sum()) for r in range(world)]
    r = int(np.argmax(gain))
    assert gain[r] > 0
    return r, int((old == r).sum())


class OracleEngine:
    """Stand-in with the slice of TokenBucketEngine that cluster.migrate's host path uses:
    oracle.semantics.TokenBucketTable per class over dense ids, export_state / import_state,
    and get_class / set_class / classes when classed."""

    def __init__(self, n_keys: int, classes):
        from oracle.semantics import TokenBucketConfig, TokenBucketTable
        self.n_keys = n_keys
        self._classes = [tuple(c) for c in classes]
        self.classed = len(classes) > 1
        self.tables = [TokenBucketTable(TokenBucketConfig.from_options(*c)) for c in classes]
        self.cls = np.zeros(n_keys, dtype=np.uint8)

    def classes(self):
        return list(self._classes)

    def get_class(self, ids):
        return self.cls[np.asarray(ids, dtype=np.int64)].copy()

    def set_class(self, ids, cls):
        for i, c in zip(np.asarray(ids, dtype=np.int64).tolist(), np.asarray(cls).tolist()):
            if self.cls[i] != c:
                st = self.tables[self.cls[i]].state.pop(i, None)
                if st is not None:
                    self.tables[c].state[i] = st
                self.cls[i] = c

    def acquire_batch(self, ids, permits, ts):
        g, r = [], []
        for i, p, t in zip(np.asarray(ids).tolist(), np.asarray(permits).tolist(), np.asarray(ts).tolist()):
            ok, rem = self.tables[self.cls[i]].acquire(int(i), int(p), int(t))
            g.append(1 if ok else 0)
            r.append(rem)
        return np.array(g, dtype=np.uint8), np.array(r, dtype=np.int32)

    def export_state(self):
        v = np.array([self._classes[c][0] for c in self.cls.tolist()], dtype=np.float64)
        t = np.full(self.n_keys, ABSENT, dtype=np.int64)
        for tab in self.tables:
            for i, st in tab.state.items():
                v[i], t[i] = st.v, st.t_us
        return v, t

    def import_state(self, v, t_us, first: int = 0):
        from oracle.semantics import BucketState
        for j, (x, t) in enumerate(zip(np.asarray(v).tolist(), np.asarray(t_us).tolist())):
            i = first + j
            tab = self.tables[self.cls[i]]
            if t == ABSENT:
                tab.state.pop(i, None)
            else:
                tab.state[i] = BucketState(x, t)

    def synchronize(self):
        pass

    def close(self):
        pass


def _dump(engine, directory, world, torch=None, dev=None):
    """{v, t, dir_keys, dir_ids}: the engine's rows and, of all touched keys, those the
    directory holds with their ids."""
    from distributedratelimiting.redis_amd import cluster
    engine.synchronize()
    v, t = engine.export_state()
    keys = touched(world, range(W.TB_STEPS)).astype(np.uint64)
    if isinstance(directory, cluster.DeviceDirectory):
        ids = directory.lookup(torch.from_numpy(keys.view(np.int64)).to(dev)).cpu().numpy().view(np.uint64)
    else:
        ids = directory.lookup(keys)
    have = ids != NO
    return {"v": np.asarray(v).copy(), "t": np.asarray(t).copy(), "dir_keys": keys[have], "dir_ids": ids[have],
            "dir_size": np.int64(directory.size())}


def _run(rank, world, out_dir, case, engine, directory, decide, to_dev, to_host, cap, torch=None, dev=None):
    """Steps 0-1 under the hash partition, migrate, steps 2-3 under map B (case "ok" or
    "lapse"); case "tight": steps 0-1, a migrate that every rank must refuse, dumps around it."""
    from distributedratelimiting.redis_amd import cluster
    shift = LAPSE_SHIFT if case == "lapse" else 0
    mb = map_b(world)
    out = {}

    def step(s, omap):
        k, p, t = (to_dev(x) for x in batch(rank, s, shift))
        g, r = cluster.route_batch(decide, k, p, t, directory, owner_map=omap)
        out[f"g{s}"], out[f"r{s}"] = to_host(g), to_host(r)

    step(0, None)
    step(1, None)
    if case == "tight":
        before = _dump(engine, directory, world, torch, dev)
        try:
            cluster.migrate(engine, directory, mb, migrate_ts(world))
            raised = 0
        except ValueError:
            raised = 1
        after = _dump(engine, directory, world, torch, dev)
        out.update({f"before_{k}": x for k, x in before.items()})
        out.update({f"after_{k}": x for k, x in after.items()})
        out["raised"] = np.int64(raised)
    else:
        sent, recv = cluster.migrate(engine, directory, mb, migrate_ts(world, shift))
        out["sent"], out["recv"] = np.int64(sent), np.int64(recv)
        step(2, mb)
        step(3, mb)
        out.update(_dump(engine, directory, world, torch, dev))
    np.savez(os.path.join(out_dir, f"mig_{rank}.npz"), **out)


def _capacity(rank: int, world: int, case: str) -> int:
    from distributedratelimiting.redis_amd import cluster
    if case == "tight":
        r, held = tight_rank(world)
        if rank == r:
            return held          # room for what it holds, none for what map B adds
    return cluster.keys_per_rank(W.TB["n_keys"], world)


def migrate_worker(rank: int, world: int, port: int, out_dir: str, case: str = "ok", classed: str = "plain"):
    """Oracle stand-in engines, HostDirectory, numpy batches over gloo."""
    dist = W._init(rank, world, port)
    from distributedratelimiting.redis_amd import cluster
    cap = _capacity(rank, world, case)
    engine = OracleEngine(cap, CLASSES if classed == "classed" else CLASSES[:1])
    directory = cluster.HostDirectory(cap)

    def decide(lk, lp, lt):
        if engine.classed:
            key_of = {i: k for k, i in directory.ids.items()}
            engine.set_class(lk, np.array([key_of[i] % 3 for i in lk.tolist()], dtype=np.uint8))
        return engine.acquire_batch(lk, lp, lt)

    _run(rank, world, out_dir, case, engine, directory, decide, lambda x: x, lambda x: np.asarray(x), cap)
    dist.barrier()
    dist.destroy_process_group()


def migrate_worker_hip(rank: int, world: int, port: int, out_dir: str, path: str, case: str = "ok",
                       classed: str = "plain"):
    """HIP engines on cuda:0; path "host": numpy batches, HostDirectory, host-buffer engine
    calls; path "device": CUDA tensors end to end with a DeviceDirectory."""
    dist = W._init(rank, world, port)
    torch, dev, stream = W._hip_setup()
    from distributedratelimiting.redis_amd import TokenBucketEngine, cluster
    cap = _capacity(rank, world, case)
    c = classed == "classed"
    engine = TokenBucketEngine(cap, *CLASSES[0], device=0, classes=CLASSES[1:] if c else None)
    if path == "device":
        directory = cluster.DeviceDirectory(cap, device=0)

        def decide(lk, lp, lt):
            if c and lk.numel():
                engine.set_class_device(lk, (directory.keys_of(lk) % 3).to(torch.uint8), stream=stream.cuda_stream)
            g = torch.empty(lk.numel(), dtype=torch.uint8, device=dev)
            r = torch.empty(lk.numel(), dtype=torch.int32, device=dev)
            engine.acquire_batch_device(lk, lp, lt, g, r, stream=stream.cuda_stream)
            return g, r

        def to_dev(x):
            return torch.from_numpy(np.asarray(x).view(np.int64) if x.dtype == np.uint64 else x).to(dev)

        _run(rank, world, out_dir, case, engine, directory, decide, to_dev, lambda x: x.cpu().numpy(), cap, torch, dev)
    else:
        directory = cluster.HostDirectory(cap)

        def decide(lk, lp, lt):
            if c and lk.shape[0]:
                key_of = {i: k for k, i in directory.ids.items()}
                engine.set_class(lk, np.array([key_of[i] % 3 for i in lk.tolist()], dtype=np.uint8))
            return engine.acquire_batch(lk, lp, lt)

        _run(rank, world, out_dir, case, engine, directory, decide, lambda x: x, lambda x: np.asarray(x), cap)
    engine.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    # python tests/_migrate_workers.py <worker> <rank> <world> <port> <out_dir> [args]
    fn = globals()[sys.argv[1]]
    fn(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), *sys.argv[5:])
