"""Rank bodies and checks for tests/test_text_migrate_gloo.py (oracle stand-in engines,
HostStringDirectory, gloo on the CPU) and tests/test_gpu_text_migrate.py (HIP engines, two
ranks on one GPU over gloo): route two steps by text under the hash partition,
cluster.migrate to map B, route two more steps under B.

The stream is tests/_dist_workers.py's (tb_batch: 1000 keys, 4 steps of 3000 requests per
rank); key k travels as the name b"r<k>" followed by k % 19 dashes, 2 to 22 bytes, so the
names cross the 8- and 16-byte word boundaries.  Map B, the oracle stand-in and the batch
timing are tests/_migrate_workers.py's.
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

N = W.TB["n_keys"]
NO = np.uint64(0xFFFFFFFFFFFFFFFF)


def name(k: int) -> bytes:
    return b"r%d" % k + b"-" * (k % 19)


NAMES = [name(k) for k in range(N)]
ROOM = np.array([(len(s) + 7) & ~7 for s in NAMES], dtype=np.int64)   # arena bytes per name


def route_keys(seed: int) -> np.ndarray:
    """The routing key of every name (index = key number)."""
    from distributedratelimiting.redis_amd import cluster
    from distributedratelimiting.redis_amd.strdir import pack_strings
    buf, offs = pack_strings(NAMES)
    return cluster.text_route_keys(buf, offs, seed, int(offs[-1]))


def owners(world: int, seed: int):
    """(owner under the hash partition, owner under map B) of every name."""
    from distributedratelimiting.redis_amd import cluster
    rk = route_keys(seed)
    return cluster.key_owner(rk, world), cluster.key_owner(rk, world, M.map_b(world))


def tight_rank(world: int, seed: int):
    """(rank, names it holds after steps 0-1) of the rank that gains the most names by map B."""
    assert M.touched(world, (0, 1)).size == N
    old, new = owners(world, seed)
    gain = [int((new == r).sum() - (old == r).sum()) for r in range(world)]
    r = int(np.argmax(gain))
    assert gain[r] > 0
    return r, int((old == r).sum())


def tight_arena_rank(world: int, seed: int):
    """(rank, arena bytes it holds after steps 0-1) of the rank whose padded key text grows the
    most under map B."""
    assert M.touched(world, (0, 1)).size == N
    old, new = owners(world, seed)
    gain = [int(ROOM[new == r].sum() - ROOM[old == r].sum()) for r in range(world)]
    r = int(np.argmax(gain))
    assert gain[r] > 0
    return r, int(ROOM[old == r].sum())


def _key_number(text: bytes) -> int:
    return int(text[1:].rstrip(b"-"))


# ------------------------------------------------------------------ checks
def check_text_migrate(res, classed: bool = False, shift: int = 0, device_path: bool = False, seed: int = 0,
                       moved: int = None):
    """Replies of all four steps and the final rows against the serial reference of
    test_migrate_gloo.check_migrate (one CTokenBucket per class, class of key k = k % 3 when
    classed) behind ONE HostStringDirectory; every name held by exactly the rank map B names
    for its routing key."""
    from oracle import cref
    from oracle.semantics import fill_rate_per_second
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory
    world = len(res)
    classes = M.CLASSES if classed else M.CLASSES[:1]
    nc = len(classes)
    refs = [cref.CTokenBucket(N, c[0], fill_rate_per_second(c[1], c[2])) for c in classes]
    sdir = HostStringDirectory(N)
    for s in range(W.TB_STEPS):
        batches = [M.batch(r, s, shift) for r in range(world)]
        k, p, t = (np.concatenate([b[i] for b in batches]) for i in range(3))
        ids = sdir.assign([NAMES[i] for i in k.tolist()])
        g, rem = np.empty(k.size, np.uint8), np.empty(k.size, np.int32)
        for c, ref in enumerate(refs):
            sel = (k % np.uint64(nc)) == c
            g[sel], rem[sel] = ref.acquire_batch(ids[sel], p[sel], t[sel])
        for r in range(world):
            sl = slice(r * W.TB_N, (r + 1) * W.TB_N)
            assert np.array_equal(res[r][f"g{s}"], g[sl]), (s, r)
            assert np.array_equal(res[r][f"r{s}"], rem[sl]), (s, r)
    old, new = owners(world, seed)
    n_moved = int((old != new).sum())
    if moved is not None:
        assert n_moved == moved
    ref_id = sdir.lookup(NAMES).astype(np.int64)
    state = [ref.export_state() for ref in refs]
    seen = []
    for r in range(world):
        keys, ids = res[r]["dir_keys"].astype(np.int64), res[r]["dir_ids"].astype(np.int64)
        assert np.all(new[keys] == r)                        # the new owner's names only
        for c in range(nc):
            sel = keys % nc == c
            assert np.array_equal(res[r]["t"][ids[sel]], state[c][1][ref_id[keys[sel]]])
            assert np.array_equal(res[r]["v"][ids[sel]].view(np.int64), state[c][0][ref_id[keys[sel]]].view(np.int64))
        seen.append(keys)
        assert int(res[r]["dir_size"]) == int((new == r).sum())
        if device_path:
            assert int(res[r]["arena_used"]) == int(ROOM[new == r].sum())
    seen = np.concatenate(seen)
    assert seen.size == np.unique(seen).size == N          # every name once, none held twice
    sent, recv = sum(int(x["sent"]) for x in res), sum(int(x["recv"]) for x in res)
    assert sent == recv == (0 if shift else n_moved)
    if not shift:
        assert all(int(x["sent"]) > 0 and int(x["recv"]) > 0 for x in res)
    for ref in refs:
        ref.close()


def check_refused(res, device_path: bool = False):
    """Every rank raised, and nothing changed on any of them."""
    names = ("v", "t", "dir_keys", "dir_ids", "dir_size") + (("arena_used",) if device_path else ())
    for r, x in enumerate(res):
        assert int(x["raised"]) == 1, r
        for nm in names:
            a, b = x[f"before_{nm}"], x[f"after_{nm}"]
            assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a,
                                  b.view(np.int64) if b.dtype == np.float64 else b), (r, nm)


# ------------------------------------------------------------------ rank bodies
def _run(rank, world, out_dir, case, engine, directory, decide, route, dump, seed):
    """Steps 0-1 under the hash partition, migrate, steps 2-3 under map B (case "ok" or
    "lapse"); cases "tight" and "arena": steps 0-1, a migrate that every rank must refuse,
    dumps around it."""
    from distributedratelimiting.redis_amd import cluster
    from distributedratelimiting.redis_amd.strdir import pack_strings
    shift = M.LAPSE_SHIFT if case == "lapse" else 0
    mb = M.map_b(world)
    out = {}

    def step(s, omap):
        k, p, t = M.batch(rank, s, shift)
        buf, offs = pack_strings([NAMES[i] for i in k.tolist()])
        out[f"g{s}"], out[f"r{s}"] = route(buf, offs, p, t, omap)

    step(0, None)
    step(1, None)
    if case in ("tight", "arena"):
        before = dump()
        try:
            cluster.migrate(engine, directory, mb, M.migrate_ts(world), seed=seed)
            raised = 0
        except ValueError:
            raised = 1
        after = dump()
        out.update({f"before_{k}": x for k, x in before.items()})
        out.update({f"after_{k}": x for k, x in after.items()})
        out["raised"] = np.int64(raised)
    else:
        sent, recv = cluster.migrate(engine, directory, mb, M.migrate_ts(world, shift), seed=seed)
        out["sent"], out["recv"] = np.int64(sent), np.int64(recv)
        step(2, mb)
        step(3, mb)
        out.update(dump())
    return out


def _capacity(rank: int, world: int, case: str, seed: int) -> int:
    from distributedratelimiting.redis_amd import cluster
    if case == "tight":
        r, held = tight_rank(world, seed)
        if rank == r:
            return held          # room for what it holds, none for what map B adds
    return cluster.keys_per_rank(N, world)


def text_migrate_worker(rank: int, world: int, port: int, out_dir: str, case: str = "ok", classed: str = "plain",
                        seed: int = 0):
    """Oracle stand-in engines, HostStringDirectory, numpy batches over gloo."""
    dist = W._init(rank, world, port)
    from distributedratelimiting.redis_amd import cluster
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory
    seed = int(seed)
    cap = _capacity(rank, world, case, seed)
    engine = M.OracleEngine(cap, M.CLASSES if classed == "classed" else M.CLASSES[:1])
    directory = HostStringDirectory(cap)
    out = _run(rank, world, out_dir, case, engine, directory, *_host_calls(engine, directory, seed), seed)
    np.savez(os.path.join(out_dir, f"tmig_{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


def _host_calls(engine, directory, seed):
    """(decide, route, dump) of the host path: numpy batches and a HostStringDirectory."""
    from distributedratelimiting.redis_amd import cluster

    def decide(lk, lp, lt):
        if engine.classed and len(lk):
            text_of = {i: s for s, i in directory.ids.items()}
            engine.set_class(lk, np.array([_key_number(text_of[i]) % 3 for i in np.asarray(lk).tolist()], dtype=np.uint8))
        return engine.acquire_batch(lk, lp, lt)

    def route(buf, offs, p, t, omap):
        g, r = cluster.route_text_batch(decide, buf, offs, p, t, directory, owner_map=omap, seed=seed,
                                        n_bytes=int(offs[-1]))
        return np.asarray(g), np.asarray(r)

    def dump():
        engine.synchronize()
        v, t = engine.export_state()
        ids = directory.lookup(NAMES)
        have = ids != NO
        return {"v": np.asarray(v).copy(), "t": np.asarray(t).copy(), "dir_keys": np.flatnonzero(have),
                "dir_ids": ids[have], "dir_size": np.int64(directory.size())}

    return decide, route, dump


def text_migrate_worker_hip(rank: int, world: int, port: int, out_dir: str, path: str, case: str = "ok",
                            classed: str = "plain", seed: int = 0):
    """HIP engines on cuda:0; path "host": numpy batches, HostStringDirectory, host-buffer
    engine calls; path "device": CUDA tensors end to end with a StringDirectory."""
    dist = W._init(rank, world, port)
    torch, dev, stream = W._hip_setup()
    from distributedratelimiting.redis_amd import TokenBucketEngine, cluster
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory, StringDirectory, to_device
    seed = int(seed)
    cap = _capacity(rank, world, case, seed)
    c = classed == "classed"
    engine = TokenBucketEngine(cap, *M.CLASSES[0], device=0, classes=M.CLASSES[1:] if c else None)
    if path == "device":
        arena = 1 << 16
        if case == "arena":
            r, used = tight_arena_rank(world, seed)
            if rank == r:
                arena = used         # room for the text it holds, none for what map B adds
        directory = StringDirectory(cap, arena, device=0)
        all_names = to_device(NAMES, dev)
        cls_of_key = torch.arange(N, device=dev) % 3

        def decide(lk, lp, lt):
            if c and lk.numel():
                ids = directory.lookup(*all_names)
                tab = torch.zeros(cap, dtype=torch.int64, device=dev)
                tab[ids[ids >= 0]] = cls_of_key[ids >= 0]
                engine.set_class_device(lk, tab[lk].to(torch.uint8), stream=stream.cuda_stream)
            g = torch.empty(lk.numel(), dtype=torch.uint8, device=dev)
            r = torch.empty(lk.numel(), dtype=torch.int32, device=dev)
            engine.acquire_batch_device(lk, lp, lt, g, r, stream=stream.cuda_stream)
            return g, r

        def route(buf, offs, p, t, omap):
            g, r = cluster.route_text_batch(decide, torch.from_numpy(buf).to(dev),
                                            torch.from_numpy(offs.view(np.int64)).to(dev), torch.from_numpy(p).to(dev),
                                            torch.from_numpy(t).to(dev), directory, owner_map=omap, seed=seed,
                                            n_bytes=int(offs[-1]))
            return g.cpu().numpy(), r.cpu().numpy()

        def dump():
            engine.synchronize()
            v, t = engine.export_state()
            ids = directory.lookup(*all_names).cpu().numpy().view(np.uint64)
            have = ids != NO
            held, used, _ = directory.usage()      # raises if the directory is in an error state
            out = {"v": np.asarray(v).copy(), "t": np.asarray(t).copy(), "dir_keys": np.flatnonzero(have),
                   "dir_ids": ids[have], "dir_size": np.int64(held), "arena_used": np.int64(used)}
            # the text behind every held id, read back through the directory
            buf, offs = directory.text_of(torch.from_numpy(ids[have].view(np.int64)).to(dev))
            blob, o = buf.cpu().numpy().tobytes(), offs.cpu().numpy()
            assert [blob[o[j]:o[j + 1]] for j in range(o.size - 1)] == [NAMES[k] for k in np.flatnonzero(have)]
            return out

        out = _run(rank, world, out_dir, case, engine, directory, decide, route, dump, seed)
        if case in ("tight", "arena"):
            # the refused migration left the directory usable: a known name still resolves to its
            # id through assign, and no error state has been raised
            k = int(out["after_dir_keys"][0])
            got = directory.assign(*to_device([NAMES[k]], dev))
            assert int(got[0]) == int(out["after_dir_ids"][0])
            assert directory.size() == int(out["after_dir_size"])
    else:
        directory = HostStringDirectory(cap)
        out = _run(rank, world, out_dir, case, engine, directory, *_host_calls(engine, directory, seed), seed)
    np.savez(os.path.join(out_dir, f"tmig_{rank}.npz"), **out)
    engine.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    # python tests/_text_migrate_workers.py <worker> <rank> <world> <port> <out_dir> [args]
    fn = globals()[sys.argv[1]]
    fn(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), *sys.argv[5:])
