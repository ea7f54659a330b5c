"""Multi-GPU layer: one engine per GPU (one process per rank), keys hash-partitioned.

The reference distributes by letting many client processes share one Redis key space
(the bucket key is ``InstanceName + resourceID``, PTB:42).  Here every key
has exactly one owner GPU holding its bucket state:

    owner(key) = ((mix64(key) >> 32) * world) >> 32      (= mix64(key) >> (64 - log2 world))

or, with an owner map (every routing call takes ``owner_map=``), the map's entry for the
key's virtual node (the top 12 bits of mix64(key)): ``balanced_owner_map`` builds one from
observed per-virtual-node loads so that a Zipf stream's hot keys do not overload their
owners, and the owner's key directory (``tbe_dir_*``, device-resident and collision-free: it
stores whole keys) turns the keys it owns into dense bucket ids.  The token-bucket paths
need no collective when ingest is already partitioned (the benchmark's default mode).
Exchanges:

* ``route_requests`` / ``route_replies`` (``route_batch`` = both around a ``decide``):
  requests that arrive at any rank travel to their owner in one all-to-all (grouped by a
  stable partition, so a key's requests reach the owner in (source rank, arrival) order,
  a valid serial order of the reference) and the replies come back in a reverse
  all-to-all.  On GPUs everything stays in HBM (``tbe_route_*`` kernels + RCCL); only the
  world group sizes go through the host, as the all-to-all's split sizes.
* ``route_text_requests`` / ``route_text_batch``: the same for a batch keyed by text (the
  reference's own strings): the owner follows from a 64-bit routing key of the text
  (``text_route_keys``), every string travels with its bytes (a third all-to-all), and the
  owner's string directory resolves them byte for byte (DESIGN.md §7 "Routing text").
* ``route_cancel``: cancellations of queued requests travel to the key's owner the same
  way (one all-to-all each way).
* ``migrate`` / ``migrate_queueing``: a new owner map comes into force between two batches;
  the buckets whose owner changes travel to their new owners (one all-to-all of rows), and for
  a queueing engine their queued waits travel with them, in order and with their request ids
  (a second all-to-all of ring entries), which therefore must be unique across owners
  (DESIGN.md §7 "Migrating buckets", "Migrating queued waits").
* ``approx_epoch``: the ApproximateTokenBucket global tier.  Each rank is one client
  (A:9-599) holding a local tier for every shared key; at every refresh epoch the
  per-key consumed counts are exchanged -- all-gather for exact per-client prefix
  semantics (client r's sync call sees clients 0..r-1, SURVEY.md §8e option 2), or
  all-reduce when the node acts as ONE client (option 1) -- and every rank replays the
  same sync calls on its replica of the global tier.

Inputs as CUDA tensors take the device path (backend "nccl" = RCCL over xGMI); numpy
arrays take a host path with identical semantics (backend "gloo", the CPU tests).  The
device path also runs over a "gloo" group (its collectives then stage through host
memory): that is how two ranks sharing one GPU exercise the whole device path in the
tests (RCCL refuses two ranks on one device).

A directory holds the keys whose buckets are alive: ``reclaim`` removes the keys whose
bucket has expired (the Redis ``EXPIRE``, TB:232-235) and their ids are handed out again, so
a churning key space passes through a directory of the size of its live set.  A batch that
brings more new keys than there is room for raises ``TbeError(TBE_ERANGE)`` before any
decision is made; that state is sticky, so an owner reclaims from a timer well before it.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import numpy as np

GAMMA = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1
NO_ID = np.uint64(MASK64)


# ------------------------------------------------------------------ key partitioning
def _mix64(z: np.ndarray) -> np.ndarray:
    z = np.asarray(z, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def key_owner(keys, world: int, owner_map=None) -> np.ndarray:
    """Owner rank of each key (csrc/tbe_hash.hpp key_owner): ((mix64(key) >> 32) * world)
    >> 32, i.e. the top log2(world) bits of mix64(key) for a power-of-two world; with an
    owner map (include/tbe_cluster.h), owner_map[key_vnode(key)]."""
    if owner_map is not None:
        return np.asarray(check_owner_map(owner_map, world), dtype=np.int64)[key_vnode(keys)]
    h = _mix64(keys) >> np.uint64(32)
    with np.errstate(over="ignore"):
        return ((h * np.uint64(world)) >> np.uint64(32)).astype(np.int64)


# ------------------------------------------------------------------ owner maps
OWNER_MAP_BITS = 12                  # include/tbe_cluster.h TBE_OWNER_MAP_BITS
OWNER_MAP_SIZE = 1 << OWNER_MAP_BITS


def key_vnode(keys) -> np.ndarray:
    """Virtual node of each key: the top 12 bits of mix64(key) (tbe_key_vnode)."""
    return (_mix64(keys) >> np.uint64(64 - OWNER_MAP_BITS)).astype(np.int64)


def check_owner_map(owner_map, world: int):
    """Validate an owner map before any kernel reads it (include/tbe_cluster.h: a u8 array
    of exactly 4096 entries, each < world).  A CUDA tensor's shape and dtype are checked
    here; its values are not read back (that would synchronise every routed batch) -- the
    route kernels clamp an entry >= world to world - 1, so a bad device map misroutes but
    never writes out of bounds.  Returns the map unchanged; raises ValueError otherwise."""
    if _is_cuda(owner_map):
        import torch
        if owner_map.dtype != torch.uint8 or owner_map.numel() != OWNER_MAP_SIZE:
            raise ValueError(f"owner map must be {OWNER_MAP_SIZE} uint8 entries")
        return owner_map
    m = np.asarray(owner_map)
    if m.shape != (OWNER_MAP_SIZE,):
        raise ValueError(f"owner map must have exactly {OWNER_MAP_SIZE} entries, got shape {m.shape}")
    if m.dtype != np.uint8:
        if not np.issubdtype(m.dtype, np.integer) or m.min() < 0 or m.max() > 255:
            raise ValueError("owner map entries must be uint8 owner ranks")
    if int(m.max()) >= world:
        raise ValueError(f"owner map entry {int(m.max())} >= world ({world})")
    return m


def hash_owner_map(world: int) -> np.ndarray:
    """The owner map equal to the hash partition for a power-of-two world:
    v -> (v * world) >> 12."""
    if world & (world - 1) or not 1 <= world <= OWNER_MAP_SIZE:
        raise ValueError("the hash owner map needs a power-of-two world <= 4096")
    return ((np.arange(OWNER_MAP_SIZE, dtype=np.int64) * world) >> OWNER_MAP_BITS).astype(np.uint8)


# Keys one engine holds in its fastest layout: two 8-bit LSD passes over the bucket ids
# (2^11 keys per bucket) with room for the 1024 hot-key buckets, and packed 8-byte records.
# Past it the engine takes a third partition pass, and past 2^27 keys its records no longer
# pack (a 28-bit key field leaves under 32 bits for the time offset), which also turns off
# hot-key runs: on Zipf traffic that is a cliff, not a slope (DESIGN.md §7 "owner maps").
PACKED_KEYS_MAX = (65536 - 1024) << 11


def max_vnodes_per_owner(n_keys: int, world: int, slack: float = 0.01, limit: int = PACKED_KEYS_MAX) -> int:
    """The most virtual nodes one owner may take while its table (keys_per_rank) stays
    within `limit` keys; never fewer than the even share ceil(4096 / world)."""
    fair = -(-OWNER_MAP_SIZE // world)
    best = fair
    for m in range(fair + 1, OWNER_MAP_SIZE + 1):
        share = -(-n_keys * m // OWNER_MAP_SIZE)
        if min(n_keys, int(share * (1.0 + slack)) + 1024) > limit:
            break
        best = m
    return best


def balanced_owner_map(loads, world: int, n_keys: int | None = None) -> np.ndarray:
    """An owner map that evens out the owners' request loads (DESIGN.md §7 "owner maps").
    loads[v] = requests observed on virtual node v (e.g. all ranks' vnode counts of a
    batch, all-reduced so that every rank builds the same map).  Longest processing time
    first: virtual nodes by descending load (ties by index), each to the owner with the
    least load so far (ties to the lowest rank), virtual nodes without load spread so that
    every owner ends with about the same number of them (its share of the key space).
    n_keys (the global key space): no owner takes more than max_vnodes_per_owner virtual
    nodes, so every owner's table stays in the packed two-pass layout -- the owner of a
    very hot key then keeps more of the load than the others instead of pushing their
    tables over that limit.  Deterministic: the same loads give the same map on every rank."""
    loads = np.asarray(loads, dtype=np.int64).reshape(-1)
    if loads.size != OWNER_MAP_SIZE or world < 1 or world > 256:
        raise ValueError("loads must have 4096 entries and 1 <= world <= 256")
    order = np.lexsort((np.arange(OWNER_MAP_SIZE), -loads))
    out = np.empty(OWNER_MAP_SIZE, dtype=np.uint8)
    acc = np.zeros(world, dtype=np.int64)
    nv = np.zeros(world, dtype=np.int64)
    cap_v = -(-OWNER_MAP_SIZE // world)
    cap = OWNER_MAP_SIZE if n_keys is None else max_vnodes_per_owner(n_keys, world)
    big = np.iinfo(np.int64).max
    for v in order.tolist():
        if loads[v] > 0:
            r = int(np.argmin(np.where(nv < cap, acc, big)))
        else:   # no load seen: keep the owners' shares of the key space level
            r = int(np.argmin(np.where(nv < cap_v, nv, OWNER_MAP_SIZE + 1)))
        out[v] = r
        acc[r] += loads[v]
        nv[r] += 1
    return out


def _scramble_params(n: int):
    bits = max(1, int(n - 1).bit_length())
    return np.uint64((1 << bits) - 1), np.uint64(max(1, bits // 2))


def _scramble(x: np.ndarray, mask, sh) -> np.ndarray:
    with np.errstate(over="ignore"):
        for a, c in ((0x9E3779B97F4A7C15, 0x632BE59BD9B4E019),
                     (0xD1B54A32D192ED03, 0x8CB92BA72F3D8DD7),
                     (0xAEF17502108EF2D9, 0x2545F4914F6CDD1D)):
            x = (x * np.uint64(a) + np.uint64(c)) & mask
            x ^= x >> sh
    return x


def scramble_walk(x, n: int) -> np.ndarray:
    """The fixed bijection of [0, n) the directory applies to its counters
    (csrc/tbe_hash.hpp scramble_walk)."""
    mask, sh = _scramble_params(n)
    x = _scramble(np.asarray(x, dtype=np.uint64), mask, sh)
    bad = x >= np.uint64(n)
    while bad.any():
        x[bad] = _scramble(x[bad], mask, sh)
        bad = x >= np.uint64(n)
    return x


class HostIdPool:
    """Host model of the directories' id pool (csrc/tbe_idpool.hpp, DESIGN.md §7 "The id
    rule"): a stack of freed ids and a ``fresh`` counter.  Keys new to it, in order of first
    occurrence, each pop the stack; once it is empty they take id = scramble_walk(fresh++,
    capacity).  ``reclaim`` removes keys and pushes their ids in ascending order.  Never
    reclaimed, it hands out scramble_walk(0), (1), ..."""

    def __init__(self, capacity: int):
        self.capacity = int(capacity)
        self.ids = {}
        self.free = []
        self.fresh = 0
        self.overflow = False

    def _take(self, new) -> None:
        """Ids for `new`: keys not in ``ids``, distinct, in order of first occurrence."""
        room = len(self.free) + max(0, self.capacity - self.fresh)
        if len(new) > room:
            self.overflow = True
        new = new[:room]
        n_pop = min(len(new), len(self.free))
        for k in new[:n_pop]:
            self.ids[k] = self.free.pop()
        if new[n_pop:]:
            ctr = np.arange(self.fresh, self.fresh + len(new) - n_pop, dtype=np.uint64)
            self.fresh += len(new) - n_pop
            for k, i in zip(new[n_pop:], scramble_walk(ctr, self.capacity).tolist()):
                self.ids[k] = i

    def reclaim(self, dead_ids, keep_ids=()) -> int:
        """Remove every held key whose id is in dead_ids and not in keep_ids; their ids go
        onto the free stack in ascending order.  Returns the number removed."""
        gone = {int(i) for i in dead_ids} - {int(i) for i in keep_ids}
        victims = sorted((i, k) for k, i in self.ids.items() if i in gone)
        for i, k in victims:
            del self.ids[k]
            self.free.append(i)
        return len(victims)

    def size(self) -> int:
        return len(self.ids)


class HostDirectory(HostIdPool):
    """Host mirror of the device key directory (tbe_dir_*): a HostIdPool over u64 keys.
    Used by the gloo path and the tests."""

    def check(self) -> None:
        """Raise TbeError(TBE_ERANGE) once a batch has brought more new keys than ids remained."""
        if self.overflow:
            from . import _capi
            raise _capi.TbeError(_capi.TBE_ERANGE, f"key directory over capacity ({self.capacity} ids)")

    def assign(self, keys) -> np.ndarray:
        keys = np.asarray(keys, dtype=np.uint64)
        if keys.size == 0:
            return np.zeros(0, dtype=np.uint64)
        uniq, first = np.unique(keys, return_index=True)
        self._take([k for _, k in sorted((f, k) for k, f in zip(uniq.tolist(), first.tolist()) if k not in self.ids)])
        return self.lookup(keys)

    def lookup(self, keys) -> np.ndarray:
        get = self.ids.get
        return np.array([get(k, MASK64) for k in np.asarray(keys, dtype=np.uint64).tolist()], dtype=np.uint64)


class _DeviceReclaim:
    """reclaim_device / reclaim of a device directory: ``_RECLAIM_DEVICE`` and ``_RECLAIM``
    name its two C entry points (tbe_dir_* or tbe_sdir_*), ``_h`` is its handle."""

    def reclaim_device(self, d_dead, d_keep_ids=None):
        """The device-form reclaim on the current stream: d_dead is a uint8 device tensor of
        ``capacity`` flags indexed by id (``TokenBucketEngine.expired_device``), d_keep_ids
        an int64 device tensor of ids never to remove.  Returns a one-element int64 device
        tensor that receives the number of keys removed (nothing is synchronised)."""
        import torch
        from . import _capi
        if d_dead.numel() != self.capacity or d_dead.element_size() != 1:
            raise ValueError("d_dead must hold one byte per id of the directory's capacity")
        d_dead = d_dead.contiguous()
        n_keep = 0 if d_keep_ids is None else d_keep_ids.numel()
        if n_keep:
            d_keep_ids = d_keep_ids.contiguous()
        count = torch.zeros(1, dtype=torch.int64, device=d_dead.device)
        st = getattr(self._lib, self._RECLAIM_DEVICE)(self._h, d_dead.data_ptr(),
                                                      d_keep_ids.data_ptr() if n_keep else None, n_keep,
                                                      count.data_ptr(), device_stream(d_dead.device))
        if st != _capi.TBE_OK:
            raise _capi.TbeError(st, f"{self._RECLAIM_DEVICE} failed")
        return count

    def reclaim(self, engine, ts_us: int, keep_ids=None) -> int:
        """Drop every key whose bucket no longer exists in `engine` at ts_us (the Redis EXPIRE
        of idle buckets, TB:232-235); keep_ids: ids of an assign whose engine batch is not
        submitted yet.  Synchronous; returns the number of keys removed."""
        import ctypes
        from . import _capi
        keep = np.ascontiguousarray([] if keep_ids is None else keep_ids, dtype=np.uint64)
        n = ctypes.c_uint64()
        st = getattr(self._lib, self._RECLAIM)(self._h, engine.handle, int(ts_us),
                                               keep.ctypes.data if keep.size else None, keep.size, ctypes.byref(n))
        if st != _capi.TBE_OK:
            raise _capi.TbeError(st, f"{self._RECLAIM} failed")
        return n.value

    def reclaim_idle(self, engine, ts_us: int, keep_ids=None, d_idle=None):
        """Give back the ids of the keys an ``ApproximateEngine`` no longer needs at ts_us
        (DESIGN.md §2c): scan (``idle_device``), clear the flags of keep_ids (an int64 device
        tensor or a sequence: ids of an assign whose engine batch is not submitted yet),
        remove the flagged keys (``reclaim_device``) and reset the flagged ids to a new
        engine's state (``reset_device``) -- all on the current stream, nothing synchronised.
        d_idle: flags already scanned and agreed between the clients of a replicated tier
        (``approx_idle_epoch``); the scan is then skipped.  The engine must cover the
        directory's ids.  Ids no key holds are idle too and are reset with the rest (a sync
        replays every id and leaves an unheld one a row with a period estimate), so an id
        assigned after this call and before the next sync starts as a new limiter.  Returns (count, d_idle): a one-element int64 device tensor that
        receives the number of keys removed, and the flags used."""
        import torch
        if engine.n_keys < self.capacity:
            raise ValueError("the engine has fewer keys than the directory has ids")
        dev = torch.device("cuda", torch.cuda.current_device()) if d_idle is None else d_idle.device
        st = device_stream(dev)
        if d_idle is None:
            d_idle = torch.empty(self.capacity, dtype=torch.uint8, device=dev)
            engine.idle_device(ts_us, d_idle, stream=st)
        elif d_idle.numel() != self.capacity or d_idle.element_size() != 1:
            raise ValueError("d_idle must hold one byte per id of the directory's capacity")
        if keep_ids is not None:
            keep = keep_ids if torch.is_tensor(keep_ids) else torch.as_tensor(
                np.asarray(keep_ids, dtype=np.int64), device=dev)
            if keep.numel():
                d_idle.index_fill_(0, keep.to(device=dev, dtype=torch.int64), 0)
        count = self.reclaim_device(d_idle)
        engine.reset_device(d_idle, stream=st)
        return count, d_idle


class DeviceDirectory(_DeviceReclaim):
    """The owner's key directory in HBM (include/tbe_cluster.h tbe_dir_*).

    ``strict`` (default): ``check()`` raises TBE_ERANGE for the very batch that overflowed,
    before anything is decided -- near capacity that costs a device synchronisation per
    batch.  ``strict=False``: near capacity each check enqueues an asynchronous copy of the
    directory's state (tbe_dir_state_async) and inspects the previous one, so an overflow
    raises one batch later without synchronising; the overflowing batch itself is still
    refused, by the engine (its keys beyond capacity get UINT64_MAX ids, an invalid batch:
    TBE_EINVAL at the engine's next synchronisation, and that batch's reply buffers are left
    unwritten).  Once an overflow has been seen every later check() raises, as in strict mode.
    bench.py --route timed uses it, so no synchronisation sits inside a timed step."""

    def __init__(self, capacity: int, device: int = -1, strict: bool = True):
        import ctypes
        from . import _capi
        self._lib = _capi.load()
        h = ctypes.c_void_p()
        st = self._lib.tbe_dir_create(int(capacity), device, ctypes.byref(h))
        if st != _capi.TBE_OK:
            raise _capi.TbeError(st, f"tbe_dir_create({capacity}) failed")
        self._h = h
        self.capacity = int(capacity)
        # upper bound of the keys held (each key of an assign batch adds at most one, a
        # reclaim only removes): while it stays below capacity no batch can have overflowed,
        # so the exact count (a device synchronisation) is fetched only once the bound
        # reaches it
        self._bound = 0
        self.strict = strict
        self._pending = None     # (pinned state copy, event) of the last asynchronous check
        self._overflowed = False  # an asynchronous check saw the (sticky) overflow bit

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.tbe_dir_destroy(self._h)
            self._h = None

    def check(self) -> None:
        """Raise TbeError(TBE_ERANGE) if an assign batch overflowed the directory; free
        (no device synchronisation) while the assigned-id bound stays below capacity."""
        if self._bound < self.capacity:
            return
        if self.strict:
            self._bound = self.size()      # raises TBE_ERANGE on overflow
            return
        import torch
        from . import _capi
        if self._overflowed:   # the overflow bit is sticky: refuse every later batch too
            raise _capi.TbeError(_capi.TBE_ERANGE, f"key directory over capacity ({self.capacity} ids)")
        if self._pending is not None and self._pending[1].query():
            st = self._pending[0]
            self._pending = None
            if int(st[1]) != 0:
                self._overflowed = True
                raise _capi.TbeError(_capi.TBE_ERANGE, f"key directory over capacity ({self.capacity} ids)")
        if self._pending is None:
            dev = torch.device("cuda", torch.cuda.current_device())
            st = torch.zeros(2, dtype=torch.int64, pin_memory=True)
            rc = self._lib.tbe_dir_state_async(self._h, st.data_ptr(), device_stream(dev))
            if rc != _capi.TBE_OK:
                raise _capi.TbeError(rc, "tbe_dir_state_async failed")
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            self._pending = (st, ev)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _run(self, fn, d_keys):
        import torch
        from . import _capi
        if not _is_cuda(d_keys) or d_keys.dtype not in (torch.int64, torch.uint64):
            raise TypeError("DeviceDirectory takes an int64 (or uint64) CUDA tensor of keys")
        d_keys = d_keys.contiguous()
        ids = torch.empty(d_keys.numel(), dtype=torch.int64, device=d_keys.device)
        st = fn(self._h, d_keys.data_ptr(), d_keys.numel(), ids.data_ptr(), device_stream(d_keys.device))
        if st != _capi.TBE_OK:
            raise _capi.TbeError(st, "directory call failed")
        return ids

    def assign(self, d_keys):
        """int64 device tensor of keys -> int64 device tensor of ids (assigning new ones;
        keys beyond capacity get -1, and check() raises from then on)."""
        ids = self._run(self._lib.tbe_dir_assign_device, d_keys)
        self._bound += d_keys.numel()
        return ids

    def lookup(self, d_keys):
        """ids of known keys, -1 (UINT64_MAX) for others; assigns nothing."""
        return self._run(self._lib.tbe_dir_lookup_device, d_keys)

    def keys_of(self, d_ids):
        """int64 device tensor of ids -> int64 device tensor of the keys holding them, -1
        (UINT64_MAX) for an id no key holds (tbe_dir_keys_of_device)."""
        return self._run(self._lib.tbe_dir_keys_of_device, d_ids)

    def size(self) -> int:
        """Keys held (assigned and not reclaimed since); raises TBE_ERANGE after an overflow."""
        import ctypes
        from . import _capi
        n = ctypes.c_uint64()
        st = self._lib.tbe_dir_size(self._h, ctypes.byref(n))
        if st != _capi.TBE_OK:
            raise _capi.TbeError(st, "directory over capacity" if st == _capi.TBE_ERANGE else "tbe_dir_size failed")
        return n.value

    _RECLAIM_DEVICE, _RECLAIM = "tbe_dir_reclaim_device", "tbe_dir_reclaim"

    def reclaim(self, engine, ts_us: int, keep_ids=None) -> int:
        import ctypes
        from . import _capi
        n = super().reclaim(engine, ts_us, keep_ids)
        held = ctypes.c_uint64()
        st = self._lib.tbe_dir_size(self._h, ctypes.byref(held))
        # exact after a reclaim (reclaim_device leaves the bound valid: it only removes); an
        # overflowed directory keeps check() on its exact path
        self._bound = held.value if st == _capi.TBE_OK else self.capacity
        return n


def keys_per_rank(n_keys: int, world: int, slack: float = 0.01, owner_map=None) -> int:
    """Table capacity per rank for n_keys hash-partitioned keys: the expected share plus
    a margin far above the binomial spread of the owner counts.  With an owner map, the
    share of the owner with the most virtual nodes (each holds 1/4096 of the keys)."""
    if world == 1:
        return n_keys
    if owner_map is not None:
        most = int(np.bincount(np.asarray(owner_map, dtype=np.int64), minlength=world).max())
        share = -(-n_keys * most // OWNER_MAP_SIZE)
    else:
        share = -(-n_keys // world)
    return min(n_keys, int(share * (1.0 + slack)) + 1024)


def vnode_loads(d_keys):
    """Requests per virtual node of a device batch (tbe_vnode_count_device): int64 [4096]."""
    import torch
    from . import _capi
    lib = _capi.load()
    d_keys = _device_columns(d_keys)[0]
    out = torch.empty(OWNER_MAP_SIZE, dtype=torch.int64, device=d_keys.device)
    _check(lib.tbe_vnode_count_device(d_keys.data_ptr(), d_keys.numel(), out.data_ptr(), device_stream(d_keys.device)))
    return out


def _device_map(owner_map, dev, world: int):
    """The owner map as a u8 device tensor (NULL pointer for the hash partition), validated
    (check_owner_map) so that no route kernel sees an entry >= world."""
    if owner_map is None:
        return None
    import torch
    check_owner_map(owner_map, world)
    m = owner_map if _is_cuda(owner_map) else torch.from_numpy(np.ascontiguousarray(owner_map, dtype=np.uint8))
    return m.to(device=dev, dtype=torch.uint8).contiguous()


# ------------------------------------------------------------------ collectives
def _stages_through_host(t, group) -> bool:
    """A CUDA tensor on a gloo group: gloo's all-to-all / all-gather take host tensors."""
    import torch.distributed as dist
    return _is_cuda(t) and dist.get_backend(group) == "gloo"


def _all_to_all(out, inp, out_splits=None, in_splits=None, group=None) -> None:
    import torch.distributed as dist
    if _stages_through_host(inp, group):
        o = out.cpu()
        dist.all_to_all_single(o, inp.cpu(), output_split_sizes=out_splits, input_split_sizes=in_splits,
                               group=group)
        out.copy_(o)
        return
    dist.all_to_all_single(out, inp, output_split_sizes=out_splits, input_split_sizes=in_splits, group=group)


def _all_gather(out, inp, group=None) -> None:
    import torch.distributed as dist
    if _stages_through_host(inp, group):
        o = out.cpu()
        dist.all_gather_into_tensor(o, inp.cpu(), group=group)
        out.copy_(o)
        return
    dist.all_gather_into_tensor(out, inp, group=group)


def _all_reduce_sum(t, group=None) -> None:
    import torch.distributed as dist
    if _stages_through_host(t, group):
        h = t.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
        t.copy_(h)
        return
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)


# ------------------------------------------------------------------ all-to-all routing
class RoutePlan:
    """What route_replies needs to send replies back: the arrival -> grouped permutation
    and the all-to-all split sizes of both directions."""

    def __init__(self, order, send_counts, recv_counts, n, error=None):
        self.order, self.send_counts, self.recv_counts, self.n = order, send_counts, recv_counts, n
        # route_text_requests: this rank's batch was malformed and none of it was sent (n is 0
        # then); the rank still takes part in the reply exchange, and route_text_batch raises
        # this afterwards
        self.error = error


def _is_cuda(x) -> bool:
    return hasattr(x, "is_cuda") and x.is_cuda


def route_requests(keys, permits, ts_us, directory, group=None, owner_map=None):
    """Send this rank's requests to their owners.  Returns ((local ids, permits, ts) of
    the requests this rank owns, in (source rank, arrival) order, and the RoutePlan for
    route_replies).  CUDA tensors: device kernels + RCCL; numpy: host path + gloo.
    owner_map: table-driven ownership (balanced_owner_map), the same on every rank."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size(group)
    if _is_cuda(keys):
        dev = keys.device
        keys, permits, ts_us = _device_columns(keys, (permits, torch.int32), (ts_us, torch.int64))
        pos, sc_l, rc_l, recv = _route_device(keys, permits, ts_us, world, group, owner_map)
        local = directory.assign(recv[:, 0])
        directory.check()        # an over-capacity batch raises before anything is decided
        return (local, recv[:, 2].to(torch.int32), recv[:, 1].contiguous()), RoutePlan(pos, sc_l, rc_l, keys.numel())
    keys = np.asarray(keys, dtype=np.uint64)
    n = keys.shape[0]
    owner = key_owner(keys, world, owner_map)
    order = np.argsort(owner, kind="stable")
    send_counts = np.bincount(owner, minlength=world).astype(np.int64)
    sc = torch.from_numpy(send_counts)
    rc = torch.empty_like(sc)
    dist.all_to_all_single(rc, sc, group=group)
    recv_counts = rc.numpy()
    payload = np.stack([keys[order].view(np.int64), np.asarray(ts_us, dtype=np.int64)[order],
                        np.asarray(permits, dtype=np.int64)[order]], axis=1)
    recv = torch.empty((int(recv_counts.sum()), 3), dtype=torch.int64)
    dist.all_to_all_single(recv, torch.from_numpy(np.ascontiguousarray(payload)),
                           output_split_sizes=recv_counts.tolist(), input_split_sizes=send_counts.tolist(),
                           group=group)
    r = recv.numpy()
    local = directory.assign(r[:, 0].view(np.uint64))
    directory.check()
    return (local, r[:, 2].astype(np.int32), r[:, 1].copy()), RoutePlan(order, send_counts.tolist(),
                                                                        recv_counts.tolist(), n)


def _device_columns(keys, *cols):
    """The device path's input contract: keys int64 (uint64 is reinterpreted), the other
    columns converted to the dtype the route kernels read, all on the keys' device."""
    import torch
    if keys.dtype == torch.uint64:
        keys = keys.view(torch.int64)
    if keys.dtype != torch.int64:
        raise TypeError(f"keys must be an int64 or uint64 tensor, not {keys.dtype}")
    out = [keys.contiguous()]
    for c, dt in cols:
        if not _is_cuda(c) or c.device != keys.device:
            raise ValueError("every column of a device-path batch must be on the keys' device")
        if c.numel() != keys.numel():
            raise ValueError("columns differ in length")
        out.append(c.to(dt).contiguous())
    return tuple(out)


def _route_device(keys, permits, payload, world, group, owner_map=None):
    """Owner-grouped exchange of {key, payload i64, permits i32} records on the device:
    tbe_route_plan_map_device + tbe_route_pack_device, the split sizes by all-to-all, the
    records by all-to-all.  Returns (pos, send counts, recv counts, recv [m, 3] int64)."""
    import torch
    from . import _capi
    lib = _capi.load()
    dev = keys.device
    stream = device_stream(dev)
    n = keys.numel()
    pos = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    counts = torch.zeros(world, dtype=torch.int64, device=dev)
    work = torch.empty(max(1, lib.tbe_route_workspace_bytes(n, world)), dtype=torch.uint8, device=dev)
    dmap = _device_map(owner_map, dev, world)
    _check(lib.tbe_route_plan_map_device(keys.data_ptr(), n, world, dmap.data_ptr() if dmap is not None else None,
                                         work.data_ptr(), pos.data_ptr(), counts.data_ptr(), stream))
    send = torch.empty((n, 3), dtype=torch.int64, device=dev)
    _check(lib.tbe_route_pack_device(pos.data_ptr(), n, keys.data_ptr(), permits.data_ptr(),
                                     payload.data_ptr(), send.data_ptr(), stream))
    rc = torch.empty_like(counts)
    _all_to_all(rc, counts, group=group)
    sc_l, rc_l = counts.tolist(), rc.tolist()
    recv = torch.empty((sum(rc_l), 3), dtype=torch.int64, device=dev)
    _all_to_all(recv, send, rc_l, sc_l, group=group)
    return pos, sc_l, rc_l, recv


def route_replies(plan: RoutePlan, cols, group=None):
    """Send the owner's reply columns (one int64-convertible array/tensor per column, in
    route_requests' received order) back; returns them in this rank's arrival order."""
    import torch
    import torch.distributed as dist

    if cols and _is_cuda(cols[0]):
        from . import _capi
        lib = _capi.load()
        dev = cols[0].device
        reply = torch.stack([c.to(torch.int64) for c in cols], dim=1).contiguous()
        k = reply.shape[1]
        back = torch.empty((plan.n, k), dtype=torch.int64, device=dev)
        _all_to_all(back, reply, plan.send_counts, plan.recv_counts, group=group)
        out = torch.empty_like(back)
        _check(lib.tbe_route_gather_device(plan.order.data_ptr(), plan.n, back.data_ptr(), k, out.data_ptr(),
                                           device_stream(dev)))
        return tuple(out[:, c] for c in range(k))
    k = len(cols)
    m = sum(plan.recv_counts)
    reply = np.stack([np.asarray(c, dtype=np.int64).reshape(-1) for c in cols], axis=1) if m \
        else np.zeros((0, k), dtype=np.int64)
    back = torch.empty((plan.n, k), dtype=torch.int64)
    dist.all_to_all_single(back, torch.from_numpy(np.ascontiguousarray(reply)),
                           output_split_sizes=plan.send_counts, input_split_sizes=plan.recv_counts, group=group)
    b = back.numpy()
    out = np.empty_like(b)
    out[plan.order] = b
    return tuple(out[:, c] for c in range(k))


def route_batch(decide: Callable, keys, permits, ts_us, directory, group=None, owner_map=None):
    """Decide a batch whose requests arrived at this rank but may belong to any rank.

    ``decide(local_ids, permits, ts) -> (col0, col1[, ...])`` runs this rank's engine on
    the requests it owns (e.g. granted and remaining; a queueing engine adds the request
    ids it assigns, which a later ``route_cancel`` needs).  Returns the columns for this
    rank's own requests in their arrival order: granted/status as u8, remaining as i32,
    further columns as i64 (host path) or the int64 device tensors (device path)."""
    (lk, lp, lt), plan = route_requests(keys, permits, ts_us, directory, group, owner_map)
    cols = decide(lk, lp, lt)
    out = route_replies(plan, cols, group)
    if _is_cuda(out[0]):
        import torch
        return (out[0].to(torch.uint8), out[1].to(torch.int32)) + tuple(out[2:])
    return (out[0].astype(np.uint8), out[1].astype(np.int32)) + tuple(out[2:])


# ------------------------------------------------------------------ routing text
TEXT_MAX_LEN = 1 << 16               # a key's longest text (include/tbe_strdir.h)


def _text_spans(offs, n_bytes: int):
    """(start, length, malformed) of every string of an Arrow-style array, by the string
    directory's rules (sd_span): end < start, end > n_bytes or a length over 65536 is
    malformed, and such a string reads as the empty string at offset 0."""
    o = np.ascontiguousarray(offs)
    o = o.view(np.uint64) if o.dtype == np.int64 else o.astype(np.uint64)
    a, b = o[:-1], o[1:]
    with np.errstate(over="ignore"):
        ok = (b >= a) & (b <= np.uint64(n_bytes)) & (b - a <= np.uint64(TEXT_MAX_LEN))
        zero = np.uint64(0)
        return np.where(ok, a, zero).astype(np.int64), np.where(ok, b - a, zero).astype(np.int64), ~ok


def _as_u8(buf) -> np.ndarray:
    return np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else np.asarray(buf, dtype=np.uint8)


def text_route_keys(buf, offs, seed: int = 0, n_bytes: Optional[int] = None) -> np.ndarray:
    """The u64 routing key of every string (include/tbe_cluster.h "routing text";
    tbe_text_route_key, tbe_route_text_keys_device): h = mix64(seed ^ len * GAMMA), then h =
    mix64(h ^ w_k) over the little-endian 8-byte words of the text, the last one zero-padded.
    buf: uint8 array (or bytes), offs: n + 1 offsets, n_bytes: the bytes in use (default: all
    of buf).  The owner of a string is ``key_owner`` / ``key_vnode`` of this key.  A malformed
    string (``_text_spans``) hashes as the empty string."""
    buf = _as_u8(buf)
    nb = buf.shape[0] if n_bytes is None else int(n_bytes)
    start, length, _ = _text_spans(offs, nb)
    pad = np.zeros(nb + 8, dtype=np.uint8)
    pad[:nb] = buf[:nb]
    with np.errstate(over="ignore"):
        h = _mix64(np.uint64(seed & MASK64) ^ (length.astype(np.uint64) * np.uint64(GAMMA)))
    idx = np.flatnonzero(length > 0)
    k = 0
    while idx.size:
        p = start[idx] + 8 * k
        rem = length[idx] - 8 * k
        w = np.zeros(idx.size, dtype=np.uint64)
        for b in range(8):
            w |= np.where(b < rem, pad[np.minimum(p + b, nb)], 0).astype(np.uint64) << np.uint64(8 * b)
        h[idx] = _mix64(h[idx] ^ w)
        idx = idx[rem > 8]
        k += 1
    return h


def plan_text_route(buf, offs, world: int, owner_map=None, seed: int = 0, n_bytes: Optional[int] = None) -> dict:
    """What one rank sends when a batch keyed by text is routed: the rule of
    tbe_route_text_keys_device, tbe_route_plan_map_device, tbe_route_text_offsets_device and
    tbe_route_text_pack_device in numpy, their reference and the body of the host path.
    Returns keys (u64), n_bad, lens (int64, arrival order), order (grouped -> arrival), pos
    (arrival -> grouped), counts and byte_counts (int64 [world]), send_offs (int64 [n + 1]) and
    out_bytes (uint8 [send_offs[n]]: every owner's strings, arrival order, tightly packed)."""
    buf = _as_u8(buf)
    nb = buf.shape[0] if n_bytes is None else int(n_bytes)
    start, lens, bad = _text_spans(offs, nb)
    n = lens.shape[0]
    keys = text_route_keys(buf, offs, seed, nb)
    owner = key_owner(keys, world, owner_map) if n else np.zeros(0, dtype=np.int64)
    order = np.argsort(owner, kind="stable")
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n, dtype=np.int64)
    counts = np.bincount(owner, minlength=world).astype(np.int64)
    send_offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens[order], out=send_offs[1:])
    src = np.repeat(start[order] - send_offs[:-1], lens[order]) + np.arange(int(send_offs[-1]), dtype=np.int64)
    byte_counts = np.bincount(owner, weights=lens, minlength=world).astype(np.int64)
    return {"keys": keys, "n_bad": int(bad.sum()), "lens": lens, "order": order, "pos": pos, "counts": counts,
            "byte_counts": byte_counts, "send_offs": send_offs, "out_bytes": buf[src]}


def _malformed(n_bad: int) -> ValueError:
    return ValueError(f"route_text: {n_bad} strings of the batch have malformed offsets (end < start, end > n_bytes "
                      f"or longer than {TEXT_MAX_LEN} bytes); none of the batch was sent")


def route_text_requests(buf, offs, permits, ts_us, directory, group=None, owner_map=None, seed: int = 0,
                        n_bytes: Optional[int] = None):
    """``route_requests`` for a batch keyed by text (DESIGN.md §7 "Routing text"): an
    Arrow-style string array -- buf (uint8), offs (n + 1 offsets), n_bytes (default: all of
    buf) -- with permits and ts_us.  Each string goes to the owner of its routing key
    (``text_route_keys``; owner maps apply to that key as to any u64), carrying its text; the
    owner's string directory resolves the received strings byte for byte.  Returns what
    ``route_requests`` returns, and ``route_replies`` takes the plan as it is.

    CUDA tensors and a ``StringDirectory``: tbe_route_text_* kernels; text, offsets and records
    stay in HBM, only the per-owner row and byte counts cross to the host.  numpy arrays and a
    ``HostStringDirectory``: the same protocol on the host (gloo).  Three all-to-alls: the
    {rows, bytes} counts together, the {len, ts_us, permits} rows, the bytes.

    A batch with malformed offsets (``_text_spans``) is not sent: this rank announces zero
    counts, takes part in every exchange (it still decides what the other ranks send it), and
    the returned plan carries a ValueError in ``plan.error`` and describes an empty batch
    (``plan.n`` = 0, an empty ``order``, zero send counts), so ``route_replies`` on it returns
    empty columns on either path.  The other ranks are unaffected.

    The device path synchronises with the host three times per batch: the sender's counts, the
    received counts, and ``StringDirectory.size()`` after the assign (the directory's only
    overflow check)."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    if owner_map is not None and not _is_cuda(owner_map):
        check_owner_map(owner_map, world)
    if _is_cuda(buf):
        if not hasattr(directory, "text_of"):
            raise TypeError("route_text_requests with CUDA tensors needs a StringDirectory")
        return _route_text_device(buf, offs, permits, ts_us, directory, world, group, owner_map, seed, n_bytes)
    return _route_text_host(buf, offs, permits, ts_us, directory, world, group, owner_map, seed, n_bytes)


def _route_text_host(buf, offs, permits, ts_us, directory, world, group, owner_map, seed, n_bytes):
    import torch
    import torch.distributed as dist
    from . import _capi
    buf = _as_u8(buf)
    p = plan_text_route(buf, offs, world, owner_map, seed, n_bytes)
    n = p["lens"].shape[0]
    error = _malformed(p["n_bad"]) if p["n_bad"] else None
    order = p["order"]
    if error is None:
        sc2 = np.stack([p["counts"], p["byte_counts"]], axis=1)
        rows = np.stack([p["lens"][order], np.asarray(ts_us, dtype=np.int64)[order],
                         np.asarray(permits, dtype=np.int64)[order]], axis=1)
        out_bytes = p["out_bytes"]
    else:
        sc2 = np.zeros((world, 2), dtype=np.int64)
        rows, out_bytes = np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.uint8)
    sc = torch.from_numpy(np.ascontiguousarray(sc2).reshape(-1))
    rc = torch.empty_like(sc)
    dist.all_to_all_single(rc, sc, group=group)
    rc2 = rc.numpy().reshape(world, 2)
    sc_rows, sc_bytes = sc2[:, 0].tolist(), sc2[:, 1].tolist()
    rc_rows, rc_bytes = rc2[:, 0].tolist(), rc2[:, 1].tolist()
    recv = torch.empty((sum(rc_rows), 3), dtype=torch.int64)
    dist.all_to_all_single(recv, torch.from_numpy(np.ascontiguousarray(rows)), output_split_sizes=rc_rows,
                           input_split_sizes=sc_rows, group=group)
    recv_bytes = torch.empty(sum(rc_bytes), dtype=torch.uint8)
    dist.all_to_all_single(recv_bytes, torch.from_numpy(np.ascontiguousarray(out_bytes)), output_split_sizes=rc_bytes,
                           input_split_sizes=sc_bytes, group=group)
    r = recv.numpy()
    roffs = np.zeros(r.shape[0] + 1, dtype=np.int64)
    np.cumsum(r[:, 0], out=roffs[1:])
    blob = recv_bytes.numpy().tobytes()
    local = directory.assign([blob[roffs[j]:roffs[j + 1]] for j in range(r.shape[0])])
    if directory.overflow:
        raise _capi.TbeError(_capi.TBE_ERANGE, f"string directory over capacity ({directory.capacity} ids)")
    if error is not None:        # nothing was sent: the plan describes an empty batch
        order, n = order[:0], 0
    return (local, r[:, 2].astype(np.int32), r[:, 1].copy()), RoutePlan(order, sc_rows, rc_rows, n, error)


def _text_columns(buf, offs, n_bytes):
    """The device path's text contract: buf uint8, offs int64 (uint64 is reinterpreted) with
    n + 1 entries on buf's device, n_bytes within buf.  The kernels read the text in 8-byte
    words, so a buffer that does not start on an 8-byte boundary (a slice of a larger byte
    tensor) is copied to one that does."""
    import torch
    if buf.dtype != torch.uint8:
        raise TypeError(f"text bytes must be a uint8 tensor, not {buf.dtype}")
    if offs.dtype == torch.uint64:
        offs = offs.view(torch.int64)
    if offs.dtype != torch.int64 or not _is_cuda(offs) or offs.device != buf.device or offs.numel() < 1:
        raise TypeError("text offsets must be n + 1 int64 (or uint64) entries on the bytes' device")
    nb = buf.numel() if n_bytes is None else int(n_bytes)
    if not 0 <= nb <= buf.numel():
        raise ValueError("n_bytes exceeds the byte buffer")
    buf = buf.contiguous()
    if buf.data_ptr() % 8:
        buf = buf.clone()
    return buf, offs.contiguous(), nb


def _text_keys_device(lib, buf, offs, nb, seed, stream):
    """(int64 routing keys, one-element int64 count of malformed strings), both on the device."""
    import torch
    n = offs.numel() - 1
    keys = torch.empty(max(n, 1), dtype=torch.int64, device=buf.device)
    n_bad = torch.zeros(1, dtype=torch.int64, device=buf.device)
    _check(lib.tbe_route_text_keys_device(buf.data_ptr(), nb, offs.data_ptr(), n, int(seed) & MASK64, keys.data_ptr(),
                                          n_bad.data_ptr(), stream))
    return keys[:n], n_bad


def text_vnode_loads(d_bytes, d_offs, seed: int = 0, n_bytes: Optional[int] = None):
    """``vnode_loads`` of a device batch keyed by text: requests per virtual node of the
    strings' routing keys, int64 [4096] -- what ``balanced_owner_map`` builds a map for text
    traffic from."""
    from . import _capi
    lib = _capi.load()
    d_bytes, d_offs, nb = _text_columns(d_bytes, d_offs, n_bytes)
    keys, _ = _text_keys_device(lib, d_bytes, d_offs, nb, seed, device_stream(d_bytes.device))
    return vnode_loads(keys)


def _route_text_device(buf, offs, permits, ts_us, directory, world, group, owner_map, seed, n_bytes):
    """route_text_requests on the device: keys, plan, send offsets and pack (tbe_route_text_*),
    the counts, rows and bytes by all-to-all, the receiver's offsets, the directory."""
    import torch
    from . import _capi
    lib = _capi.load()
    buf, offs, nb = _text_columns(buf, offs, n_bytes)
    dev = buf.device
    stream = device_stream(dev)
    n = offs.numel() - 1
    cols = []
    for c, dt in ((permits, torch.int32), (ts_us, torch.int64)):
        if not _is_cuda(c) or c.device != dev:
            raise ValueError("every column of a device-path batch must be on the bytes' device")
        if c.numel() != n:
            raise ValueError("columns differ in length")
        cols.append(c.to(dt).contiguous())
    permits, ts_us = cols
    keys, n_bad = _text_keys_device(lib, buf, offs, nb, seed, stream)
    pos = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    counts = torch.zeros(world, dtype=torch.int64, device=dev)
    byte_counts = torch.zeros(world, dtype=torch.int64, device=dev)
    work = torch.empty(max(8, lib.tbe_route_workspace_bytes(n, world), lib.tbe_route_text_workspace_bytes(n)),
                       dtype=torch.uint8, device=dev)
    dmap = _device_map(owner_map, dev, world)
    _check(lib.tbe_route_plan_map_device(keys.data_ptr(), n, world, dmap.data_ptr() if dmap is not None else None,
                                         work.data_ptr(), pos.data_ptr(), counts.data_ptr(), stream))
    send_offs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    _check(lib.tbe_route_text_offsets_device(offs.data_ptr(), nb, n, pos.data_ptr(), counts.data_ptr(), world,
                                             work.data_ptr(), send_offs.data_ptr(), byte_counts.data_ptr(), stream))
    send_bytes = torch.empty((nb + 7) // 8 * 8 + 8, dtype=torch.uint8, device=dev)
    rows = torch.empty((n, 3), dtype=torch.int64, device=dev)
    _check(lib.tbe_route_text_pack_device(buf.data_ptr(), nb, offs.data_ptr(), n, pos.data_ptr(), send_offs.data_ptr(),
                                          permits.data_ptr(), ts_us.data_ptr(), send_bytes.data_ptr(),
                                          send_bytes.numel(), rows.data_ptr(), stream))
    head = torch.cat([torch.stack([counts, byte_counts], dim=1).reshape(-1), n_bad]).tolist()
    error = _malformed(head[-1]) if head[-1] else None
    sc2 = [0] * (2 * world) if error else head[:-1]
    sc = torch.tensor(sc2, dtype=torch.int64, device=dev)
    rc = torch.empty_like(sc)
    _all_to_all(rc, sc, group=group)
    rc2 = rc.tolist()
    sc_rows, sc_bytes, rc_rows, rc_bytes = sc2[0::2], sc2[1::2], rc2[0::2], rc2[1::2]
    recv = torch.empty((sum(rc_rows), 3), dtype=torch.int64, device=dev)
    _all_to_all(recv, rows[:sum(sc_rows)], rc_rows, sc_rows, group=group)
    mb = sum(rc_bytes)
    recv_bytes = torch.empty((mb + 7) // 8 * 8 + 8, dtype=torch.uint8, device=dev)
    recv_bytes[mb:] = 0
    _all_to_all(recv_bytes[:mb], send_bytes[:sum(sc_bytes)], rc_bytes, sc_bytes, group=group)
    m = recv.shape[0]
    roffs = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    rwork = torch.empty(max(8, lib.tbe_route_text_workspace_bytes(m)), dtype=torch.uint8, device=dev)
    _check(lib.tbe_route_text_recv_offsets_device(recv.data_ptr(), m, rwork.data_ptr(), roffs.data_ptr(), stream))
    local = directory.assign(recv_bytes, roffs, mb)
    directory.size()             # raises once a batch has overflowed the directory, before anything is decided
    if error is not None:        # nothing was sent: the plan describes an empty batch
        pos, n = pos[:0], 0
    return (local, recv[:, 2].to(torch.int32), recv[:, 1].contiguous()), RoutePlan(pos, sc_rows, rc_rows, n, error)


def route_text_batch(decide: Callable, buf, offs, permits, ts_us, directory, group=None, owner_map=None,
                     seed: int = 0, n_bytes: Optional[int] = None):
    """``route_batch`` for a batch keyed by text: ``route_text_requests``, ``decide`` on the
    requests this rank owns, ``route_replies``.  A rank whose batch is malformed still decides
    what it receives and takes part in the reply exchange, then raises ValueError with nothing
    of its own batch decided."""
    (lk, lp, lt), plan = route_text_requests(buf, offs, permits, ts_us, directory, group, owner_map, seed, n_bytes)
    cols = decide(lk, lp, lt)
    out = route_replies(plan, cols, group)
    if plan.error is not None:
        raise plan.error
    if _is_cuda(out[0]):
        import torch
        return (out[0].to(torch.uint8), out[1].to(torch.int32)) + tuple(out[2:])
    return (out[0].astype(np.uint8), out[1].astype(np.int32)) + tuple(out[2:])


def route_cancel(cancel: Callable, keys, request_ids, directory, group=None, owner_map=None):
    """Cancel queued requests (CancelQueueState.TrySetCanceled, Q:480-506 / A:531-557)
    that may be queued on any rank: ``keys`` are global keys, ``request_ids`` the ids
    their owners assigned (``route_batch``'s extra reply column).  ``cancel(local_ids,
    request_ids) -> u8`` runs on the owner; a key unknown to the owner's directory has
    nothing queued.  Returns the hits in this rank's order.  Per owner, the cancels apply
    by source rank, then call order."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size(group)
    if _is_cuda(keys):
        return _route_cancel_device(cancel, keys, request_ids, directory, world, group, owner_map)
    if isinstance(directory, DeviceDirectory):
        raise TypeError("route_cancel with a DeviceDirectory takes CUDA tensors of keys and request ids")
    keys = np.asarray(keys, dtype=np.uint64)
    n = keys.shape[0]
    owner = key_owner(keys, world, owner_map)
    order = np.argsort(owner, kind="stable")
    send_counts = np.bincount(owner, minlength=world).astype(np.int64)
    sc = torch.from_numpy(send_counts)
    rc = torch.empty_like(sc)
    dist.all_to_all_single(rc, sc, group=group)
    recv_counts = rc.numpy()
    payload = np.stack([keys[order].view(np.int64), np.asarray(request_ids, dtype=np.int64)[order]], axis=1)
    recv = torch.empty((int(recv_counts.sum()), 2), dtype=torch.int64)
    dist.all_to_all_single(recv, torch.from_numpy(np.ascontiguousarray(payload)),
                           output_split_sizes=recv_counts.tolist(), input_split_sizes=send_counts.tolist(),
                           group=group)
    r = recv.numpy()
    hit = np.zeros(r.shape[0], dtype=np.int64)
    if r.shape[0]:
        local = directory.lookup(r[:, 0].view(np.uint64))
        known = local != NO_ID
        if known.any():
            hit[known] = np.asarray(cancel(local[known], r[known, 1]), dtype=np.int64)
    back = torch.empty(n, dtype=torch.int64)
    dist.all_to_all_single(back, torch.from_numpy(hit), output_split_sizes=send_counts.tolist(),
                           input_split_sizes=recv_counts.tolist(), group=group)
    out = np.empty(n, dtype=np.uint8)
    out[order] = back.numpy()
    return out


def _route_cancel_device(cancel, keys, request_ids, directory, world, group, owner_map=None):
    """route_cancel's device path: (key, request id) pairs go to the owners through the
    route kernels (the id rides in the record's i64 payload), the owner's DeviceDirectory
    looks the keys up (a key it never assigned has nothing queued), ``cancel(local ids,
    request ids)`` gets the known pairs as int64 device tensors, and the hits come back
    through the reverse all-to-all.  Returns u8 hits (device tensor) in this rank's order."""
    import torch
    from . import _capi
    if not isinstance(directory, DeviceDirectory):
        raise TypeError("route_cancel with CUDA tensors needs a DeviceDirectory")
    keys, request_ids = _device_columns(keys, (request_ids, torch.int64))
    dev = keys.device
    zero = torch.zeros(keys.numel(), dtype=torch.int32, device=dev)
    pos, sc_l, rc_l, recv = _route_device(keys, zero, request_ids, world, group, owner_map)
    hit = torch.zeros(recv.shape[0], dtype=torch.int64, device=dev)
    if recv.shape[0]:
        local = directory.lookup(recv[:, 0])
        known = torch.nonzero(local != -1).flatten()
        if known.numel():
            h = cancel(local[known], recv[known, 1].contiguous())
            hit[known] = torch.as_tensor(np.asarray(h) if not _is_cuda(h) else h, device=dev).to(torch.int64)
    back = torch.empty((keys.numel(), 1), dtype=torch.int64, device=dev)
    _all_to_all(back, hit.view(-1, 1), sc_l, rc_l, group=group)
    out = torch.empty_like(back)
    lib = _capi.load()
    _check(lib.tbe_route_gather_device(pos.data_ptr(), keys.numel(), back.data_ptr(), 1, out.data_ptr(),
                                       device_stream(dev)))
    return out[:, 0].to(torch.uint8)


def device_stream(dev) -> int:
    """The current torch stream's handle for the device path.  The engine reads a NULL
    handle as "inputs complete at the call" (include/tbe.h), which the default stream's
    queued work is not, so the device path refuses it: run it inside
    torch.cuda.stream(torch.cuda.Stream(...))."""
    import torch
    h = torch.cuda.current_stream(dev).cuda_stream
    if not h:
        raise ValueError("cluster device path: set a non-default torch.cuda.Stream as current "
                         "(the default stream's NULL handle cannot order the engine's work)")
    return h


def _check(st: int) -> None:
    from . import _capi
    if st != _capi.TBE_OK:
        raise _capi.TbeError(st, "routing kernel launch failed")


# ------------------------------------------------------------------ live owner-map change
ABSENT = np.iinfo(np.int64).min          # t_us of a row never granted (tbe.h)
_CLASS_WORDS = 1 + 3 * 256               # the class table as int64 words: count, then three options each


def class_ttl_ms(token_limit: int, tokens_per_period: int, period_ticks: int) -> int:
    """EXPIRE of one limiter's buckets in ms (TB:234), as the engine computes it."""
    rate = np.float64(tokens_per_period) / (np.float64(period_ticks) / np.float64(1e7))
    q = min(max(np.float64(token_limit) / rate, 1.0), 31536000.0)
    return int(np.ceil(q)) * 1000


def rows_live(t_us, ts_us: int, ttl_ms) -> np.ndarray:
    """Which rows are live at ts_us, as a bool array: present and not lapsed
    (tbe_export_live_device's rule); ttl_ms a number or one per row; ts_us < 0 skips the
    lapse test."""
    t_us = np.asarray(t_us, dtype=np.int64)
    live = t_us != ABSENT
    if ts_us >= 0:
        live &= ~(t_us < 1000 * (int(ts_us) // 1000 - np.asarray(ttl_ms, dtype=np.int64)))
    return live


def plan_migration(keys_of_id, v, t_us, cls, live, owner_map, world: int, rank: int):
    """What one owner sends when `owner_map` (None: the hash partition) comes into force:
    tbe_migrate_out_device's rule in numpy, its reference and the body of ``migrate``'s host
    path.  keys_of_id[i]: the key holding id i, UINT64_MAX where none does; v, t_us, cls
    (None: class 0) and live (``rows_live``) describe row i.  An id is *leaving* when its key's
    new owner is not `rank`; a leaving id with a live row sends {key, bits of v, t_us, class},
    one with an absent or lapsed row sends nothing (its new owner starts it from a full
    bucket).  Returns (rows int64 [n, 4] grouped by destination ascending and by id inside
    one, counts int64 [world + 2]: rows per owner, leaving ids, orphans -- live rows whose id
    no key holds, never sent --, leaving uint8 [ids]).  A map entry >= world: ValueError."""
    return _plan_migration(keys_of_id, v, t_us, cls, live, owner_map, world, rank)[:3]


def _plan_migration(keys_of_id, v, t_us, cls, live, owner_map, world: int, rank: int):
    """``plan_migration`` and, fourth, the ids of the rows in send order (int64)."""
    keys = np.ascontiguousarray(keys_of_id, dtype=np.uint64)
    n = keys.shape[0]
    if not 1 <= world <= 256 or not 0 <= rank < world:
        raise ValueError("world in 1..256 and rank < world")
    if owner_map is not None:
        check_owner_map(owner_map, world)
    v = np.ascontiguousarray(v, dtype=np.float64)
    t_us = np.ascontiguousarray(t_us, dtype=np.int64)
    cls = np.zeros(n, dtype=np.uint8) if cls is None else np.asarray(cls, dtype=np.uint8)
    live = np.asarray(live, dtype=bool)
    if not (v.shape[0] == t_us.shape[0] == cls.shape[0] == live.shape[0] == n):
        raise ValueError("one entry per id in every column")
    held = keys != NO_ID
    dest = np.full(n, rank, dtype=np.int64)
    dest[held] = key_owner(keys[held], world, owner_map)
    leaving = held & (dest != rank)
    send = np.flatnonzero(leaving & live)
    send = send[np.argsort(dest[send], kind="stable")]
    rows = np.stack([keys[send].view(np.int64), v[send].view(np.int64), t_us[send], cls[send].astype(np.int64)],
                    axis=1).reshape(-1, 4)
    counts = np.zeros(world + 2, dtype=np.int64)
    counts[:world] = np.bincount(dest[send], minlength=world)
    counts[world] = int(leaving.sum())
    counts[world + 1] = int((live & ~held).sum())
    return rows, counts, leaving.astype(np.uint8), send.astype(np.int64)


def _arena_room(lens):
    """Arena bytes the string directory takes for texts of these lengths: each rounded up to 8."""
    return (lens + 7) & ~7


def plan_text_migration(text_of_id, v, t_us, cls, live, owner_map, world: int, rank: int, seed: int = 0) -> dict:
    """``plan_migration`` for an owner whose keys are text (DESIGN.md §7 "Migrating text-keyed
    buckets"): tbe_sdir_route_keys_device, tbe_migrate_out_ids_device and the text pack in
    numpy, their reference and the body of ``migrate``'s host path.  text_of_id[i]: the bytes
    id i holds, None where none does; the other arguments as in ``plan_migration``.  The key of
    an id is ``text_route_keys`` of its text under `seed` (a text whose key is UINT64_MAX reads
    as unheld, as on the device), and from there on the rule is ``plan_migration``'s.  Returns
    a dict: rows (column 0 = the routing key), counts and leaving as ``plan_migration``
    returns them; row_ids (int64, the id of every row, send order); lens (int64, the rows'
    text lengths); out_bytes (uint8, the rows' texts tightly packed in send order);
    byte_counts and arena_counts (int64 [world]: per destination, the text bytes and the arena
    bytes -- each length rounded up to 8 -- of its rows); arena_freed (the arena bytes of all
    leaving ids, those that send no row included)."""
    n = len(text_of_id)
    held = np.array([t is not None for t in text_of_id], dtype=bool)
    texts = [bytes(t) for t in text_of_id if t is not None]
    lens_all = np.zeros(n, dtype=np.int64)
    lens_all[held] = [len(t) for t in texts]
    keys = np.full(n, NO_ID, dtype=np.uint64)
    if texts:
        offs = np.zeros(len(texts) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(lens_all[held], dtype=np.uint64)
        blob = np.frombuffer(b"".join(texts), dtype=np.uint8)
        keys[held] = text_route_keys(blob, offs, seed, blob.shape[0])
    rows, counts, leaving, row_ids = _plan_migration(keys, v, t_us, cls, live, owner_map, world, rank)
    lens = lens_all[row_ids]
    out = b"".join(text_of_id[i] for i in row_ids.tolist())
    dest = np.repeat(np.arange(world, dtype=np.int64), counts[:world])
    return {"rows": rows, "counts": counts, "leaving": leaving, "row_ids": row_ids, "lens": lens,
            "out_bytes": np.frombuffer(out, dtype=np.uint8).copy(),
            "byte_counts": np.bincount(dest, weights=lens, minlength=world).astype(np.int64),
            "arena_counts": np.bincount(dest, weights=_arena_room(lens), minlength=world).astype(np.int64),
            "arena_freed": int(_arena_room(lens_all[leaving.astype(bool)]).sum())}


def _class_table(engine):
    """[(token_limit, tokens_per_period, period_ticks)], class 0 first."""
    if hasattr(engine, "classes"):
        return [tuple(int(x) for x in c) for c in engine.classes()]
    c = engine.config
    return [(int(c.token_limit), int(c.tokens_per_period), int(c.replenishment_period_ticks))]


def _preflight(local_error, classes, like, group) -> None:
    """Every rank raises ValueError when any rank has a `local_error` or the ranks' class
    tables differ; nothing has been changed anywhere yet.  `like`: a tensor on the device the
    exchanges run on (a CUDA tensor on the device path)."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    words = torch.zeros(_CLASS_WORDS, dtype=torch.int64)
    words[0] = len(classes)
    words[1:1 + 3 * len(classes)] = torch.tensor(classes, dtype=torch.int64).reshape(-1)
    words = words.to(like.device)
    allw = torch.empty(world * _CLASS_WORDS, dtype=torch.int64, device=like.device)
    _all_gather(allw, words, group=group)
    if local_error is None and not bool((allw.view(world, -1) == words).all().item()):
        local_error = "the ranks' engines hold different class tables"
    bad = torch.tensor([0 if local_error is None else 1], dtype=torch.int64, device=like.device)
    _all_reduce_sum(bad, group=group)
    if int(bad.item()):
        raise ValueError("cluster.migrate refused, nothing changed: "
                         + (local_error or "another rank failed its pre-flight check"))


def _room_error(engine_keys, directory, held, counts, incoming, world):
    if engine_keys < directory.capacity:
        return "the engine has fewer keys than the directory has ids"
    if counts[world + 1]:
        return f"{counts[world + 1]} live rows' ids are held by no key of the directory"
    if held - counts[world] + incoming > directory.capacity:
        return (f"the directory holds {held} keys, {counts[world]} leave and {incoming} arrive: "
                f"more than its {directory.capacity} ids")
    return None


def migrate(engine, directory, new_map, ts_us: int, group=None, seed: int = 0) -> Tuple[int, int]:
    """Bring a new owner map into force while the tables stay where they are (DESIGN.md §7
    "Migrating buckets").  A collective: every rank calls it between batches with the same
    `new_map` (None: the hash partition) and ts_us.  Each rank finds the keys it holds that
    the new map gives to another rank, sends their live bucket rows (with class byte) to the
    new owners in one all-to-all, clears those rows, drops the keys from its directory and
    installs the rows it receives behind its own directory.  Afterwards
    ``route_batch(..., owner_map=new_map)`` decides as if the new map had been in force from
    the start.  Returns (rows sent, rows received).

    With a ``DeviceDirectory`` everything stays in HBM (``migrate_out_device``,
    ``reclaim_device``, ``assign``, ``set_class_device``, ``import_rows``); only the world
    group sizes go through the host.  With a ``HostDirectory`` the same steps run on numpy
    arrays over ``export_state`` / ``import_state`` (and ``get_class`` / ``set_class`` on a
    classed engine).  Before anything changes every rank checks that no live row is an orphan,
    that its directory has room for what arrives, that its engine covers its directory and
    that all ranks hold the same class table; a failure on any rank raises ValueError on all
    of them.  Token bucket kind only; lease counters are not carried (the source zeroes
    them).

    Text-keyed buckets (DESIGN.md §7 "Migrating text-keyed buckets"): with a ``StringDirectory``
    (device path) or a ``HostStringDirectory`` (host path) a key's owner follows from the
    routing key of its text under `seed`, the seed the caller passes to ``route_text_batch``
    (the u64 paths ignore it); every row travels with its text, and afterwards
    ``route_text_batch(..., owner_map=new_map, seed=seed)`` decides as if the new map had been
    in force from the start.  The pre-flight of a ``StringDirectory`` also checks that its arena
    has room for the text that arrives, so a migration never puts it into TBE_ERANGE."""
    import torch.distributed as dist
    from . import _capi
    from .strdir import HostStringDirectory, StringDirectory
    kind = int(getattr(engine, "KIND", _capi.TBE_KIND_TOKEN_BUCKET))
    if kind == _capi.TBE_KIND_QUEUEING:
        raise ValueError("cluster.migrate: the queueing kind's rings and the host's request-id futures "
                         "would have to move too; it is not supported")
    if kind == _capi.TBE_KIND_APPROXIMATE:
        raise ValueError("cluster.migrate: the approximate kind's tier is replicated and its requests "
                         "are not routed, so there is nothing to move")
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    if new_map is not None and not _is_cuda(new_map):
        check_owner_map(new_map, world)
    if isinstance(directory, StringDirectory):
        return _migrate_text_device(engine, directory, new_map, int(ts_us), world, rank, group, int(seed))
    if isinstance(directory, HostStringDirectory):
        return _migrate_text_host(engine, directory, new_map, int(ts_us), world, rank, group, int(seed))
    if isinstance(directory, DeviceDirectory):
        return _migrate_device(engine, directory, new_map, int(ts_us), world, rank, group)
    return _migrate_host(engine, directory, new_map, int(ts_us), world, rank, group)


def _migrate_device(engine, directory, new_map, ts_us, world, rank, group):
    import torch
    from . import _capi
    dev = torch.device("cuda", engine.config.device if engine.config.device >= 0 else torch.cuda.current_device())
    st = device_stream(dev)
    cap = directory.capacity
    dmap = _device_map(new_map, dev, world)
    counts = torch.zeros(world + 2, dtype=torch.int64, device=dev)
    leaving = torch.zeros(cap, dtype=torch.uint8, device=dev)
    covered = engine.n_keys >= cap
    if covered:
        kof = directory.keys_of(torch.arange(cap, dtype=torch.int64, device=dev))
        engine.migrate_out_device(ts_us, kof, dmap, world, rank, None, counts, leaving, stream=st)
    rc = torch.empty(world, dtype=torch.int64, device=dev)
    _all_to_all(rc, counts[:world].contiguous(), group=group)
    sc_l, rc_l = counts.tolist(), rc.tolist()
    try:
        held = directory.size()
        err = _room_error(engine.n_keys, directory, held, sc_l, sum(rc_l), world)
    except _capi.TbeError as ex:
        err = str(ex)
    _preflight(err, _class_table(engine), counts, group)
    n_send = sum(sc_l[:world])
    rows = torch.empty((n_send, 4), dtype=torch.int64, device=dev)
    engine.migrate_out_device(ts_us, kof, dmap, world, rank, rows if n_send else None, counts, leaving, commit=True,
                              capacity=n_send, stream=st)
    directory.reclaim_device(leaving)
    recv = torch.empty((sum(rc_l), 4), dtype=torch.int64, device=dev)
    _all_to_all(recv, rows, rc_l, sc_l[:world], group=group)
    if recv.shape[0]:
        ids = directory.assign(recv[:, 0].contiguous())
        directory.check()
        if getattr(engine, "classed", False):   # first: a reused id still carries its previous key's class
            engine.set_class_device(ids, recv[:, 3].to(torch.uint8), stream=st)
        engine.import_rows(ids, recv[:, 1].contiguous().view(torch.float64), recv[:, 2].contiguous(), stream=st)
    return n_send, sum(rc_l)


def _migrate_host(engine, directory, new_map, ts_us, world, rank, group):
    import torch
    import torch.distributed as dist
    from . import _capi
    cap = directory.capacity
    classes = _class_table(engine)
    classed = bool(getattr(engine, "classed", False))
    v, t = engine.export_state()
    v, t = np.array(v, dtype=np.float64), np.array(t, dtype=np.int64)
    n_keys = int(getattr(engine, "n_keys", v.shape[0]))
    err = None
    if n_keys < cap or v.shape[0] < cap:
        err = "the engine has fewer keys than the directory has ids"
        rows, counts = np.zeros((0, 4), dtype=np.int64), np.zeros(world + 2, dtype=np.int64)
        leaving = np.zeros(cap, dtype=np.uint8)
    else:
        v, t = v[:cap], t[:cap]
        keys_of_id = np.full(cap, NO_ID, dtype=np.uint64)
        for k, i in directory.ids.items():
            keys_of_id[i] = k
        cls = engine.get_class(np.arange(cap, dtype=np.uint64)) if classed else np.zeros(cap, dtype=np.uint8)
        ttl = np.array([class_ttl_ms(*c) for c in classes], dtype=np.int64)[cls]
        rows, counts, leaving = plan_migration(keys_of_id, v, t, cls, rows_live(t, ts_us, ttl), new_map, world, rank)
    sc = torch.from_numpy(counts[:world].copy())
    rc = torch.empty_like(sc)
    dist.all_to_all_single(rc, sc, group=group)
    sc_l, rc_l = counts.tolist(), rc.tolist()
    if err is None:
        err = "the directory is over capacity" if directory.overflow else \
            _room_error(n_keys, directory, directory.size(), sc_l, sum(rc_l), world)
    _preflight(err, classes, sc, group)
    gone = np.flatnonzero(leaving)
    v[gone] = np.array([c[0] for c in classes], dtype=np.float64)[cls[gone]]
    t[gone] = ABSENT
    engine.import_state(v, t)
    directory.reclaim(gone)
    recv = torch.empty((sum(rc_l), 4), dtype=torch.int64)
    dist.all_to_all_single(recv, torch.from_numpy(np.ascontiguousarray(rows)), output_split_sizes=rc_l,
                           input_split_sizes=sc_l[:world], group=group)
    r = recv.numpy()
    if r.shape[0]:
        ids = directory.assign(r[:, 0].copy().view(np.uint64))
        directory.check()
        if classed:   # first: a reused id still carries its previous key's class
            engine.set_class(ids, r[:, 3].astype(np.uint8))
        v[ids.astype(np.int64)] = r[:, 1].copy().view(np.float64)
        t[ids.astype(np.int64)] = r[:, 2]
        engine.import_state(v, t)
    return int(rows.shape[0]), int(r.shape[0])


# ------------------------------------------------------------------ migrating queued waits
def plan_queue_migration(keys_of_id, v, t_us, cls, live, qcount, owner_map, world: int, rank: int):
    """``plan_migration`` for a queueing engine (tbe_queue_migrate_out_ids_device's rule in
    numpy, its reference and the body of ``migrate_queueing``'s host path).  qcount[i]: the
    entries queued on id i.  A leaving id sends a row when its bucket row is live OR its queue
    is not empty (a key with queued requests is never dead); such a row travels verbatim, a
    lapsed or absent t_us included, and its word 3 is ``class | qcount << 8``.  An orphan is an
    id no key holds whose row is live or whose queue is not empty.  Returns (rows, counts,
    leaving, row_ids): ``plan_migration``'s three and the rows' ids in send order (int64)."""
    qcount = np.asarray(qcount, dtype=np.int64)
    alive = np.asarray(live, dtype=bool) | (qcount > 0)
    rows, counts, leaving, row_ids = _plan_migration(keys_of_id, v, t_us, cls, alive, owner_map, world, rank)
    rows[:, 3] |= qcount[row_ids] << 8
    return rows, counts, leaving, row_ids


def _preflight_queue(local_error, classes, like, group) -> None:
    """``_preflight`` for ``migrate_queueing``: the class tables compared hold the five options
    of every queueing class."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    width = 5
    n_words = 1 + width * 256
    words = torch.zeros(n_words, dtype=torch.int64)
    words[0] = len(classes)
    words[1:1 + width * len(classes)] = torch.tensor(classes, dtype=torch.int64).reshape(-1)
    words = words.to(like.device)
    allw = torch.empty(world * n_words, dtype=torch.int64, device=like.device)
    _all_gather(allw, words, group=group)
    if local_error is None and not bool((allw.view(world, -1) == words).all().item()):
        local_error = "the ranks' engines hold different class tables"
    bad = torch.tensor([0 if local_error is None else 1], dtype=torch.int64, device=like.device)
    _all_reduce_sum(bad, group=group)
    if int(bad.item()):
        raise ValueError("cluster.migrate_queueing refused, nothing changed: "
                         + (local_error or "another rank failed its pre-flight check"))


def _queue_class_table(engine):
    """[(token_limit, tokens_per_period, period_ticks, queue_limit, order)], class 0 first."""
    return [tuple(int(x) for x in c) for c in engine.queue_classes()]


def migrate_queueing(engine, directory, new_map, ts_us: int, group=None) -> Tuple[int, int, int, int]:
    """``migrate`` for a queueing engine (TokenBucketWithQueue), plain or with queueing limit
    classes: a moved key keeps its bucket row, its class and its queued waits, in order and with
    their request ids, and the new owner's replenish tick grants them exactly as the old
    owner's would have (DESIGN.md §7 "Migrating queued waits").  A collective with ``migrate``'s
    calling convention; returns (rows sent, rows received, entries sent, entries received).

    A leaving key sends a row when its bucket row is live at ts_us or its queue is not empty
    (``plan_queue_migration``); word 3 of a row carries the class and the number of queued
    entries, and the entries themselves (``request_id << 16 | permits``, oldest first) follow
    in a second all-to-all whose splits both sides derive from the rows.  The receiver assigns
    ids, sets the classes (first: a class assignment requires an empty queue and resets the
    header), installs the rows and then the queues.  With a ``DeviceDirectory`` everything
    stays in HBM (``queue_migrate_out_device``, ``queue_export_ids_device(clear=True)``,
    ``reclaim_device``, ``assign``, ``set_class_device``, ``import_rows``,
    ``queue_import_ids_device``); with a ``HostDirectory`` the same steps run on numpy arrays
    over ``export_state`` / ``import_state`` and the host-buffer queue calls.  The pre-flight is
    ``migrate``'s; the class tables compared hold all five options of every class.

    Request ids travel verbatim, so after a migration a key's queue mixes ids minted by its
    old and its new owner: the owners must mint ids that are unique across owners, e.g.
    ``id_base = (rank << 40) + counter``, which stays below 2^47.  Afterwards
    ``route_batch(wait, ..., owner_map=new_map)`` and ``route_cancel(..., owner_map=new_map)``
    behave as if the new map had been in force from the start.  NewestFirst evictions of the
    last wait batch (``evicted()``) must be fetched before migrating.  Text-keyed directories,
    lease counters and the approximate kind are not covered."""
    import torch.distributed as dist
    from . import _capi
    from .strdir import HostStringDirectory, StringDirectory
    kind = int(getattr(engine, "KIND", _capi.TBE_KIND_TOKEN_BUCKET))
    if kind == _capi.TBE_KIND_TOKEN_BUCKET:
        raise ValueError("cluster.migrate_queueing: a token-bucket engine has no queues; use cluster.migrate")
    if kind == _capi.TBE_KIND_APPROXIMATE:
        raise ValueError("cluster.migrate_queueing: the approximate kind's tier is replicated and its requests "
                         "are not routed, so there is nothing to move")
    if isinstance(directory, (StringDirectory, HostStringDirectory)):
        raise ValueError("cluster.migrate_queueing: text-keyed queueing migration is out of scope")
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    if new_map is not None and not _is_cuda(new_map):
        check_owner_map(new_map, world)
    if isinstance(directory, DeviceDirectory):
        return _migrate_queue_device(engine, directory, new_map, int(ts_us), world, rank, group)
    return _migrate_queue_host(engine, directory, new_map, int(ts_us), world, rank, group)


def _migrate_queue_device(engine, directory, new_map, ts_us, world, rank, group):
    import torch
    from . import _capi
    dev = torch.device("cuda", engine.config.device if engine.config.device >= 0 else torch.cuda.current_device())
    st = device_stream(dev)
    cap = directory.capacity
    dmap = _device_map(new_map, dev, world)
    counts = torch.zeros(world + 2, dtype=torch.int64, device=dev)
    leaving = torch.zeros(cap, dtype=torch.uint8, device=dev)
    covered = engine.n_keys >= cap
    if covered:
        kof = directory.keys_of(torch.arange(cap, dtype=torch.int64, device=dev))
        engine.queue_migrate_out_device(ts_us, kof, dmap, world, rank, None, counts, leaving, stream=st)
    rc = torch.empty(world, dtype=torch.int64, device=dev)
    _all_to_all(rc, counts[:world].contiguous(), group=group)
    sc_l, rc_l = counts.tolist(), rc.tolist()
    try:
        held = directory.size()
        err = _room_error(engine.n_keys, directory, held, sc_l, sum(rc_l), world)
    except _capi.TbeError as ex:
        err = str(ex)
    _preflight_queue(err, _queue_class_table(engine), counts, group)
    n_send = sum(sc_l[:world])
    rows = torch.empty((n_send, 4), dtype=torch.int64, device=dev)
    row_ids = torch.empty(n_send, dtype=torch.int64, device=dev)
    engine.queue_migrate_out_device(ts_us, kof, dmap, world, rank, rows if n_send else None, counts, leaving,
                                    commit=True, capacity=n_send, stream=st, row_ids=row_ids if n_send else None)
    # the rows' queues, next and with nothing in between; the entry splits are the rows' counts
    # summed over each destination's group (the one host synchronisation of the source side)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    ends = torch.cumsum(torch.tensor(sc_l[:world], dtype=torch.int64, device=dev), 0)
    cum = torch.cat([zero, torch.cumsum(rows[:, 3] >> 8, 0)])
    es_l = torch.diff(cum[ends], prepend=zero).tolist()
    n_ent = sum(es_l)
    entries = torch.empty(n_ent, dtype=torch.int64, device=dev)
    if n_send:
        qcount = torch.empty(n_send, dtype=torch.int32, device=dev)
        n_out = torch.zeros(1, dtype=torch.int64, device=dev)
        engine.queue_export_ids_device(row_ids, qcount, None, entries if n_ent else None, n_out, clear=True,
                                       capacity=n_ent, stream=st)
    directory.reclaim_device(leaving)
    recv = torch.empty((sum(rc_l), 4), dtype=torch.int64, device=dev)
    _all_to_all(recv, rows, rc_l, sc_l[:world], group=group)
    rq = (recv[:, 3] >> 8).contiguous()
    rcum = torch.cat([zero, torch.cumsum(rq, 0)])
    er_l = torch.diff(rcum[torch.cumsum(torch.tensor(rc_l, dtype=torch.int64, device=dev), 0)], prepend=zero).tolist()
    rent = torch.empty(sum(er_l), dtype=torch.int64, device=dev)
    _all_to_all(rent, entries, er_l, es_l, group=group)
    if recv.shape[0]:
        ids = directory.assign(recv[:, 0].contiguous())
        directory.check()
        if getattr(engine, "classed", False):   # first: it requires an empty queue and resets the header
            engine.set_class_device(ids, (recv[:, 3] & 0xFF).to(torch.uint8), stream=st)
        engine.import_rows(ids, recv[:, 1].contiguous().view(torch.float64), recv[:, 2].contiguous(), stream=st)
        engine.queue_import_ids_device(ids.contiguous(), rq.to(torch.int32), rent if rent.numel() else None, stream=st)
    return n_send, sum(rc_l), n_ent, sum(er_l)


def _migrate_queue_host(engine, directory, new_map, ts_us, world, rank, group):
    import torch
    import torch.distributed as dist
    cap = directory.capacity
    classes = _queue_class_table(engine)
    classed = bool(getattr(engine, "classed", False))
    v, t = engine.export_state()
    v, t = np.array(v, dtype=np.float64), np.array(t, dtype=np.int64)
    n_keys = int(getattr(engine, "n_keys", v.shape[0]))
    err = None
    if n_keys < cap or v.shape[0] < cap:
        err = "the engine has fewer keys than the directory has ids"
        rows, counts = np.zeros((0, 4), dtype=np.int64), np.zeros(world + 2, dtype=np.int64)
        leaving, row_ids = np.zeros(cap, dtype=np.uint8), np.zeros(0, dtype=np.int64)
    else:
        v, t = v[:cap], t[:cap]
        keys_of_id = np.full(cap, NO_ID, dtype=np.uint64)
        for k, i in directory.ids.items():
            keys_of_id[i] = k
        all_ids = np.arange(cap, dtype=np.uint64)
        cls = engine.get_class(all_ids) if classed else np.zeros(cap, dtype=np.uint8)
        ttl = np.array([class_ttl_ms(*c[:3]) for c in classes], dtype=np.int64)[cls]
        qcount = engine.queue_export_ids(all_ids, capacity=0)[0]
        rows, counts, leaving, row_ids = plan_queue_migration(keys_of_id, v, t, cls, rows_live(t, ts_us, ttl), qcount,
                                                              new_map, world, rank)
    sc = torch.from_numpy(counts[:world].copy())
    rc = torch.empty_like(sc)
    dist.all_to_all_single(rc, sc, group=group)
    sc_l, rc_l = counts.tolist(), rc.tolist()
    if err is None:
        err = "the directory is over capacity" if directory.overflow else \
            _room_error(n_keys, directory, directory.size(), sc_l, sum(rc_l), world)
    _preflight_queue(err, classes, sc, group)
    gone = np.flatnonzero(leaving)
    v[gone] = np.array([c[0] for c in classes], dtype=np.float64)[cls[gone]]
    t[gone] = ABSENT
    engine.import_state(v, t)
    _, start, entries, _ = engine.queue_export_ids(row_ids.astype(np.uint64), clear=True)
    directory.reclaim(gone)
    recv = torch.empty((sum(rc_l), 4), dtype=torch.int64)
    dist.all_to_all_single(recv, torch.from_numpy(np.ascontiguousarray(rows)), output_split_sizes=rc_l,
                           input_split_sizes=sc_l[:world], group=group)
    r = recv.numpy()
    # rows are grouped by destination and entries follow row order: the entry splits are the
    # entry starts at the group boundaries; the receiver reads its own from the rows' word 3
    ends = np.cumsum(np.asarray(sc_l[:world], dtype=np.int64))
    es_l = np.diff(np.asarray(start, dtype=np.int64)[ends], prepend=0).tolist()
    rq = r[:, 3] >> 8
    rcum = np.concatenate([[0], np.cumsum(rq)])
    er_l = np.diff(rcum[np.cumsum(np.asarray(rc_l, dtype=np.int64))], prepend=0).tolist()
    rent = torch.empty(int(sum(er_l)), dtype=torch.int64)
    dist.all_to_all_single(rent, torch.from_numpy(np.ascontiguousarray(entries).view(np.int64).copy()),
                           output_split_sizes=er_l, input_split_sizes=es_l, group=group)
    if r.shape[0]:
        ids = directory.assign(r[:, 0].copy().view(np.uint64))
        directory.check()
        if classed:   # first: it requires an empty queue and resets the header
            engine.set_class(ids, (r[:, 3] & 0xFF).astype(np.uint8))
        v[ids.astype(np.int64)] = r[:, 1].copy().view(np.float64)
        t[ids.astype(np.int64)] = r[:, 2]
        engine.import_state(v, t)
        engine.queue_import_ids(ids, rq.astype(np.uint32), rent.numpy().view(np.uint64))
    return int(rows.shape[0]), int(r.shape[0]), int(sum(es_l)), int(sum(er_l))


# Text-keyed buckets.  The protocol of the u64 paths with three differences: the key-of-id
# table holds routing keys of the held text; the counts exchange carries {rows, text bytes,
# arena bytes} per destination; every row travels with a fifth column, its text length, and
# the texts themselves follow in a byte exchange whose splits are the byte counts (the layout
# _route_text_device uses for requests).
def _arena_error(used, freed, incoming, arena_bytes):
    if used - freed + incoming > arena_bytes:
        return (f"the directory's arena holds {used} bytes of key text, {freed} leave and {incoming} arrive: "
                f"more than its {arena_bytes} bytes")
    return None


def _migrate_text_device(engine, directory, new_map, ts_us, world, rank, group, seed):
    import torch
    from . import _capi
    lib = _capi.load()
    dev = torch.device("cuda", engine.config.device if engine.config.device >= 0 else torch.cuda.current_device())
    st = device_stream(dev)
    cap = directory.capacity
    dmap = _device_map(new_map, dev, world)
    counts = torch.zeros(world + 2, dtype=torch.int64, device=dev)
    leaving = torch.zeros(cap, dtype=torch.uint8, device=dev)
    covered = engine.n_keys >= cap
    sc_l = [0] * (world + 2)
    n_send = 0
    head = torch.zeros(3 * world + 1, dtype=torch.int64, device=dev)   # {rows, bytes, arena} per owner, then freed
    if covered:
        rk = directory.route_keys(seed)
        engine.migrate_out_device(ts_us, rk, dmap, world, rank, None, counts, leaving, stream=st)
        sc_l = counts.tolist()
        n_send = sum(sc_l[:world])
        rows = torch.empty((n_send, 4), dtype=torch.int64, device=dev)
        row_ids = torch.empty(n_send, dtype=torch.int64, device=dev)
        if n_send:
            engine.migrate_out_device(ts_us, rk, dmap, world, rank, rows, counts, None, capacity=n_send, stream=st,
                                      row_ids=row_ids)
        # the rows' text lengths and offsets; per destination (the rows are grouped by it) the
        # differences of the byte and arena-byte prefix sums at the group boundaries
        lens = torch.empty(n_send, dtype=torch.int64, device=dev)
        _check(lib.tbe_sdir_text_lengths_device(directory._h, row_ids.data_ptr(), n_send, lens.data_ptr(), None, st))
        offs = torch.zeros(n_send + 1, dtype=torch.int64, device=dev)
        aoffs = torch.zeros(n_send + 1, dtype=torch.int64, device=dev)
        if n_send:
            torch.cumsum(lens, 0, out=offs[1:])
            torch.cumsum(_arena_room(lens), 0, out=aoffs[1:])
        bounds = torch.tensor(np.concatenate([[0], np.cumsum(sc_l[:world])]), dtype=torch.int64, device=dev)
        all_ids = torch.arange(cap, dtype=torch.int64, device=dev)
        lens_all = torch.empty(cap, dtype=torch.int64, device=dev)
        _check(lib.tbe_sdir_text_lengths_device(directory._h, all_ids.data_ptr(), cap, lens_all.data_ptr(), None, st))
        head[0:3 * world:3] = counts[:world]
        head[1:3 * world:3] = offs[bounds].diff()
        head[2:3 * world:3] = aoffs[bounds].diff()
        head[3 * world] = (_arena_room(lens_all) * leaving).sum()
    head_l = head.tolist()
    freed = head_l[3 * world]
    sc3 = head[:3 * world].contiguous()
    rc3 = torch.empty_like(sc3)
    _all_to_all(rc3, sc3, group=group)
    rc_l = rc3.tolist()
    sc_rows, sc_bytes = head_l[0:3 * world:3], head_l[1:3 * world:3]
    rc_rows, rc_bytes, rc_arena = rc_l[0::3], rc_l[1::3], rc_l[2::3]
    try:
        held, used, arena_bytes = directory.usage()
        err = _room_error(engine.n_keys, directory, held, sc_l, sum(rc_rows), world) or \
            _arena_error(used, freed, sum(rc_arena), arena_bytes)
    except _capi.TbeError as ex:
        err = str(ex)
    _preflight(err, _class_table(engine), counts, group)
    # the text is packed before the reclaim, which compacts the arena and forgets the ids
    nb = sum(sc_bytes)
    send_bytes = torch.zeros((nb + 7) // 8 * 8 + 8, dtype=torch.uint8, device=dev)
    _check(lib.tbe_sdir_text_device(directory._h, row_ids.data_ptr(), n_send, offs.data_ptr(), send_bytes.data_ptr(), st))
    engine.migrate_out_device(ts_us, rk, dmap, world, rank, rows if n_send else None, counts, leaving, commit=True,
                              capacity=n_send, stream=st)
    directory.reclaim_device(leaving)
    m = sum(rc_rows)
    recv = torch.empty((m, 5), dtype=torch.int64, device=dev)
    _all_to_all(recv, torch.cat([rows, lens.view(-1, 1)], dim=1), rc_rows, sc_rows, group=group)
    mb = sum(rc_bytes)
    recv_bytes = torch.empty((mb + 7) // 8 * 8 + 8, dtype=torch.uint8, device=dev)
    recv_bytes[mb:] = 0
    _all_to_all(recv_bytes[:mb], send_bytes[:nb], rc_bytes, sc_bytes, group=group)
    if m:
        roffs = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        torch.cumsum(recv[:, 4], 0, out=roffs[1:])
        ids = directory.assign(recv_bytes, roffs, mb)
        directory.size()         # raises on an overflow, which the pre-flight has made impossible
        if getattr(engine, "classed", False):   # first: a reused id still carries its previous key's class
            engine.set_class_device(ids, recv[:, 3].to(torch.uint8), stream=st)
        engine.import_rows(ids, recv[:, 1].contiguous().view(torch.float64), recv[:, 2].contiguous(), stream=st)
    return n_send, m


def _migrate_text_host(engine, directory, new_map, ts_us, world, rank, group, seed):
    import torch
    import torch.distributed as dist
    cap = directory.capacity
    classes = _class_table(engine)
    classed = bool(getattr(engine, "classed", False))
    v, t = engine.export_state()
    v, t = np.array(v, dtype=np.float64), np.array(t, dtype=np.int64)
    n_keys = int(getattr(engine, "n_keys", v.shape[0]))
    err = None
    if n_keys < cap or v.shape[0] < cap:
        err = "the engine has fewer keys than the directory has ids"
        p = plan_text_migration([None] * cap, np.zeros(cap), np.full(cap, ABSENT), None, np.zeros(cap, dtype=bool),
                                new_map, world, rank, seed)
    else:
        v, t = v[:cap], t[:cap]
        text_of_id = [None] * cap
        for k, i in directory.ids.items():
            text_of_id[i] = k
        cls = engine.get_class(np.arange(cap, dtype=np.uint64)) if classed else np.zeros(cap, dtype=np.uint8)
        ttl = np.array([class_ttl_ms(*c) for c in classes], dtype=np.int64)[cls]
        p = plan_text_migration(text_of_id, v, t, cls, rows_live(t, ts_us, ttl), new_map, world, rank, seed)
    rows, counts, leaving = p["rows"], p["counts"], p["leaving"]
    sc3 = torch.from_numpy(np.stack([counts[:world], p["byte_counts"], p["arena_counts"]], axis=1).reshape(-1).copy())
    rc3 = torch.empty_like(sc3)
    dist.all_to_all_single(rc3, sc3, group=group)
    rc = rc3.numpy().reshape(world, 3)
    sc_l, rc_rows, rc_bytes = counts.tolist(), rc[:, 0].tolist(), rc[:, 1].tolist()
    if err is None:     # a HostStringDirectory has no arena: the arena bytes travel unchecked
        err = "the directory is over capacity" if directory.overflow else \
            _room_error(n_keys, directory, directory.size(), sc_l, sum(rc_rows), world)
    _preflight(err, classes, sc3, group)
    gone = np.flatnonzero(leaving)
    v[gone] = np.array([c[0] for c in classes], dtype=np.float64)[cls[gone]]
    t[gone] = ABSENT
    engine.import_state(v, t)
    directory.reclaim(gone)
    recv = torch.empty((sum(rc_rows), 5), dtype=torch.int64)
    send = np.concatenate([rows, p["lens"].reshape(-1, 1)], axis=1)
    dist.all_to_all_single(recv, torch.from_numpy(np.ascontiguousarray(send)), output_split_sizes=rc_rows,
                           input_split_sizes=sc_l[:world], group=group)
    recv_bytes = torch.empty(sum(rc_bytes), dtype=torch.uint8)
    dist.all_to_all_single(recv_bytes, torch.from_numpy(p["out_bytes"]), output_split_sizes=rc_bytes,
                           input_split_sizes=p["byte_counts"].tolist(), group=group)
    r = recv.numpy()
    if r.shape[0]:
        roffs = np.zeros(r.shape[0] + 1, dtype=np.int64)
        np.cumsum(r[:, 4], out=roffs[1:])
        blob = recv_bytes.numpy().tobytes()
        ids = directory.assign([blob[roffs[j]:roffs[j + 1]] for j in range(r.shape[0])])
        if directory.overflow:
            from . import _capi
            raise _capi.TbeError(_capi.TBE_ERANGE, f"string directory over capacity ({directory.capacity} ids)")
        if classed:   # first: a reused id still carries its previous key's class
            engine.set_class(ids, r[:, 3].astype(np.uint8))
        v[ids.astype(np.int64)] = r[:, 1].copy().view(np.float64)
        t[ids.astype(np.int64)] = r[:, 2]
        engine.import_state(v, t)
    return int(rows.shape[0]), int(r.shape[0])


# ------------------------------------------------------------------ approximate global tier
def approx_epoch(engine, counts, ts_us: int, stagger_us: int, mode: str = "clients",
                 group=None):
    """One refresh epoch of the ApproximateTokenBucket across ranks.

    ``engine`` exposes ``collect(counts)`` (A:430-435) and
    ``sync(all_counts, n_clients, my_client, ts_us, stagger_us)`` (A:439-508);
    ``counts`` is an int32 tensor [n_keys] on the engine's device.  Returns the drain
    log of this rank's queues."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    engine.collect(counts)
    if world == 1:
        return engine.sync(counts, 1, 0, ts_us, stagger_us, **_after_collective(counts))
    if mode == "clients":       # every rank is a client: exact prefix semantics
        allc = torch.empty(world * counts.numel(), dtype=counts.dtype, device=counts.device)
        _all_gather(allc, counts, group=group)
        return engine.sync(allc, world, rank, ts_us, stagger_us, **_after_collective(counts))
    if mode == "node":          # the node is one client: sum of the ranks' counts
        _all_reduce_sum(counts, group=group)
        return engine.sync(counts, 1, 0, ts_us, stagger_us, **_after_collective(counts))
    raise ValueError(f"unknown mode {mode!r}")


def approx_idle_epoch(engine, ts_us: int, d_idle, group=None):
    """Which keys every client of a replicated tier agrees are idle at ts_us.  Each rank scans
    its own engine into the uint8 tensor ``d_idle`` (``idle_device``); the "not idle" flags
    are summed over the ranks as int32, and a key stays flagged only where the sum is 0: a
    key one client still queues on or has consumed from is kept by all.  Every rank then
    reclaims and resets the same ids (``reclaim_idle(..., d_idle=d_idle)``), so replicas and
    directories stay identical.  Returns d_idle."""
    import torch
    import torch.distributed as dist

    engine.idle_device(ts_us, d_idle, **_after_collective(d_idle))
    if dist.is_initialized() and dist.get_world_size(group) > 1:
        busy = (d_idle == 0).to(torch.int32)
        _all_reduce_sum(busy, group=group)
        d_idle.copy_((busy == 0).to(torch.uint8))
    return d_idle


def _after_collective(t) -> dict:
    """The engine's sync replay reads the exchanged counts on its own stream: order it after
    the collective on the current stream (tbe_approx_sync_stream: an event, no host wait)."""
    if not _is_cuda(t):
        return {}
    import torch
    cur = torch.cuda.current_stream(t.device)
    if not cur.cuda_stream:     # the legacy default stream: no handle to order after
        cur.synchronize()
        return {}
    return {"stream": cur.cuda_stream}
