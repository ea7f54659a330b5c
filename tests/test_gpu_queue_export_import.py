"""tbe_queue_export_ids(_device) / tbe_queue_import_ids(_device) (include/tbe.h; DESIGN.md §7
"Migrating queued waits").  Every expected queue comes from oracle.cref.CQueueingTokenBucket,
never from the engine under test; every comparison is exact.

Sizes.  The kernels work on tiles of 2,048 listed ids (256 lanes x 8 consecutive ids): 6,000
ids are two full tiles and a partial one.  QueueLimit 8 stores 32-bit headers, QueueLimit
2,000 stores 64-bit ones and makes queues of more than 64 and more than 256 entries, so one
queue spans several rounds of the expansion loop.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ABSENT = np.iinfo(np.int64).min
FAILED, GRANTED, QUEUED, REJECTED = 0, 1, 2, 3
T0 = 1_760_000_000_000_000
SENT = 0x7EADBEEF7EADBEEF
TILE = 2_048


def _engine(n_keys, opts, classes=None, **kw):
    from distributedratelimiting.redis_amd import QueueingTokenBucketEngine
    return QueueingTokenBucketEngine(n_keys, *opts, device=0, classes=classes, **kw)


def _ref(n_keys, opts):
    from distributedratelimiting.redis_amd import fill_rate
    from oracle import cref
    return cref.CQueueingTokenBucket(n_keys, opts[0], fill_rate(opts[1], opts[2]), opts[3], opts[4])


def _words(queue):
    return [(i << 16) | p for i, p in queue]


def _want(queue_of, ids):
    """(qcount, entry_start, entries) of the listed ids from an oracle's queue_of."""
    qs = [_words(queue_of(int(k))) for k in ids]
    qcount = np.array([len(q) for q in qs], dtype=np.uint32)
    start = np.zeros(len(ids) + 1, dtype=np.uint64)
    start[1:] = np.cumsum(qcount, dtype=np.uint64)
    ent = np.array([w for q in qs for w in q], dtype=np.uint64)
    return qcount, start, ent


def _dev(a, gpu):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(gpu)


def _export_device(eng, gpu, ids, capacity, clear=False, pad=4):
    """One device call into sentinel-filled buffers; returns numpy (qcount, start, entries
    buffer [capacity + pad], total)."""
    import torch
    n = len(ids)
    d_ids = _dev(np.asarray(ids, dtype=np.uint64), gpu)
    d_q = torch.full((n,), -3, dtype=torch.int32, device=gpu)
    d_s = torch.full((n + 1,), SENT, dtype=torch.int64, device=gpu)
    d_e = torch.full((capacity + pad,), SENT, dtype=torch.int64, device=gpu)
    d_n = torch.full((1,), SENT, dtype=torch.int64, device=gpu)
    torch.cuda.synchronize()                                   # the buffers are filled before the engine's stream runs
    eng.queue_export_ids_device(d_ids, d_q, d_s, d_e if capacity else None, d_n, clear=clear, capacity=capacity)
    torch.cuda.synchronize()
    return (d_q.cpu().numpy().view(np.uint32), d_s.cpu().numpy().view(np.uint64), d_e.cpu().numpy().view(np.uint64),
            int(d_n.item()))


def _snapshot(eng):
    """Everything the new calls may change, as numpy arrays."""
    v, t = eng.export_state()
    q, s, e, tot = eng.queue_export_ids(np.arange(eng.n_keys, dtype=np.uint64))
    return v.view(np.int64).copy(), t.copy(), q, s, e


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _drive(eng, ref, rng, n_keys, steps, per_key, permits_of, id_base=0, t0=T0, gap=2_000_000, keymap=None,
           pool=None):
    """`steps` wait batches with a tick after each, on engine and oracle alike (eng None: the
    oracle alone); returns the number of requests ever QUEUED per key (from the oracle) and the
    next id base.  pool: the keys that get requests (default: all)."""
    queued = np.zeros(n_keys, dtype=np.int64)
    pool = np.arange(n_keys, dtype=np.uint64) if pool is None else pool
    for s in range(steps):
        n = len(pool) * per_key
        keys = pool[rng.integers(0, len(pool), n)]
        permits = permits_of(rng, n)
        ts = t0 + s * gap + np.sort(rng.integers(0, 1000, n)).astype(np.int64)
        ek = keys if keymap is None else keymap[keys.astype(np.int64)]
        st_ref, rem_ref, ec_ref, ei_ref = ref.acquire_batch(keys, permits, ts, id_base)
        if eng is not None:
            st, rem, (ec, ei) = eng.wait_batch(ek, permits, ts, id_base)
            assert np.array_equal(st, st_ref) and np.array_equal(rem, rem_ref), f"step {s}"
            assert np.array_equal(ec, ec_ref) and np.array_equal(ei, ei_ref), f"evictions, step {s}"
        queued += np.bincount(keys[st_ref == QUEUED].astype(np.int64), minlength=n_keys)
        id_base += n
        tick = t0 + s * gap + gap // 2
        lk_ref, li_ref, lr_ref = ref.refresh(tick)
        if eng is None:
            continue
        lk, li, lr = eng.refresh(tick)
        if keymap is not None:
            inv = np.empty(n_keys, dtype=np.int64)
            inv[keymap.astype(np.int64)] = np.arange(n_keys)
            lk = inv[lk.astype(np.int64)].astype(np.uint64)
            o = np.argsort(lk, kind="stable")
            lk, li, lr = lk[o], li[o], lr[o]
        assert np.array_equal(lk, lk_ref) and np.array_equal(li, li_ref) and np.array_equal(lr, lr_ref), f"tick {s}"
    return queued, id_base


def _small_permits(rng, n):
    return rng.choice(np.array([1, 1, 2, 3], dtype=np.int32), n)


# ---------------------------------------------------------------- 1. export equals the oracle
@pytest.mark.parametrize("order", [0, 1], ids=["oldest", "newest"])
def test_export_equals_the_oracles_queues(engine_lib, oracle_lib, gpu, order):
    from distributedratelimiting.redis_amd import TbeError
    n_keys, ql = 6_000, 8
    opts = (4, 1, 10_000_000, ql, order)
    rng = np.random.default_rng(11 + order)
    eng, ref = _engine(n_keys, opts), _ref(n_keys, opts)
    pool = np.flatnonzero(np.arange(n_keys) % 4 != 3).astype(np.uint64)   # every fourth key never gets a request
    queued, _ = _drive(eng, ref, rng, n_keys, 8, 4, _small_permits, pool=pool)
    ids = rng.permutation(n_keys).astype(np.uint64)            # every id, the empty ones left in
    qcount, start, ent = _want(ref.queue_of, ids)
    total = int(start[-1])
    # the walk really wraps: non-empty keys that enqueued more than their ring holds
    wrapped = int(((qcount > 0) & (queued[ids.astype(np.int64)] > ql)).sum())
    print("non-empty", int((qcount > 0).sum()), "wrapped", wrapped, "entries", total)
    assert wrapped >= 50 and (qcount == 0).any()

    q, s, e, tot = eng.queue_export_ids(ids)
    assert tot == total and np.array_equal(q, qcount) and np.array_equal(s, start) and np.array_equal(e, ent)
    q, s, e, tot = _export_device(eng, gpu, ids, total)
    assert tot == total and np.array_equal(q, qcount) and np.array_equal(s, start)
    assert np.array_equal(e[:total], ent) and np.all(e[total:] == SENT)
    # capacity 0 only counts
    q, s, e, tot = _export_device(eng, gpu, ids, 0)
    assert tot == total and np.array_equal(q, qcount) and np.array_equal(s, start) and np.all(e == SENT)
    # one short: nothing at or past capacity is written
    q, s, e, tot = _export_device(eng, gpu, ids, total - 1)
    assert tot == total and np.array_equal(q, qcount)
    assert np.array_equal(e[:total - 1], ent[:-1]) and np.all(e[total - 1:] == SENT)
    eng.synchronize()                                          # none of these was refused
    # one short and clearing: refused as a unit
    before = _snapshot(eng)
    q, s, e, tot = _export_device(eng, gpu, ids, total - 1, clear=True)
    with pytest.raises(TbeError):
        eng.synchronize()
    assert _same(before, _snapshot(eng))
    with pytest.raises(TbeError):
        eng.queue_export_ids(ids, clear=True, capacity=total - 1)
    eng.synchronize()                                          # the host form leaves the sticky flag alone
    assert _same(before, _snapshot(eng))
    # an id out of range: nothing is written
    bad = ids.copy()
    bad[TILE + 5] = n_keys
    q, s, e, tot = _export_device(eng, gpu, bad, total)
    assert np.all(q.view(np.int32) == -3) and np.all(s == SENT) and np.all(e == SENT) and tot == SENT
    with pytest.raises(TbeError):
        eng.synchronize()
    with pytest.raises(TbeError):
        eng.queue_export_ids(bad)
    assert _same(before, _snapshot(eng))
    # clearing with room: every listed queue is empty afterwards, the rows stay
    q, s, e, tot = _export_device(eng, gpu, ids, total, clear=True)
    assert np.array_equal(e[:total], ent)
    eng.synchronize()
    after = _snapshot(eng)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    assert not after[2].any() and len(after[4]) == 0
    assert all(eng.queue_of(int(k)) == [] for k in ids[:50])
    eng.close()


# ---------------------------------------------------------------- 2. wide headers, long queues
def test_wide_headers_and_long_queues_round_trip(engine_lib, oracle_lib, gpu):
    n_keys, ql = 300, 2_000
    opts = (4, 1, 10_000_000, ql, 0)
    rng = np.random.default_rng(5)
    eng, ref = _engine(n_keys, opts), _ref(n_keys, opts)
    base = 0
    for s, hot in enumerate([{299: 2_100, 7: 200, 100: 40}, {299: 300, 7: 150, 100: 40}]):
        keys = np.concatenate([np.full(c, k) for k, c in hot.items()] + [rng.integers(0, n_keys, 900)]).astype(np.uint64)
        keys = rng.permutation(keys)
        n = len(keys)
        permits = np.ones(n, dtype=np.int32)
        ts = T0 + s * 5_000_000 + np.arange(n, dtype=np.int64)
        st, rem, _ = eng.wait_batch(keys, permits, ts, base)
        st_ref, rem_ref, _, _ = ref.acquire_batch(keys, permits, ts, base)
        assert np.array_equal(st, st_ref) and np.array_equal(rem, rem_ref)
        base += n
        lk, li, lr = eng.refresh(T0 + s * 5_000_000 + 3_000_000)        # heads advance
        lk_ref, li_ref, lr_ref = ref.refresh(T0 + s * 5_000_000 + 3_000_000)
        assert np.array_equal(lk, lk_ref) and np.array_equal(li, li_ref)
    ids = rng.permutation(n_keys).astype(np.uint64)
    qcount, start, ent = _want(ref.queue_of, ids)
    by_key = dict(zip(ids.tolist(), qcount.tolist()))
    print("entries", int(start[-1]), "key 299:", by_key[299], "key 7:", by_key[7], "key 100:", by_key[100])
    assert by_key[299] > 1_900 and by_key[7] > 256 and 64 < by_key[100] <= 256
    total = int(start[-1])
    q, s_, e, tot = _export_device(eng, gpu, ids, total)
    assert tot == total and np.array_equal(q, qcount) and np.array_equal(s_, start)
    assert np.array_equal(e[:total], ent) and np.all(e[total:] == SENT)
    # clear, then import every queue onto another id
    q, s_, e, tot = eng.queue_export_ids(ids, clear=True)
    assert np.array_equal(e, ent)
    assert eng.queue_export_ids(ids)[3] == 0
    to = np.roll(ids, 17)                                      # id i's queue goes to to[i]
    import torch
    d_to, d_qc, d_en = _dev(to, gpu), _dev(qcount, gpu), _dev(ent, gpu)
    torch.cuda.synchronize()
    eng.queue_import_ids_device(d_to, d_qc, d_en)
    torch.cuda.synchronize()
    eng.synchronize()
    q2, s2, e2, tot2 = eng.queue_export_ids(to)
    assert tot2 == total and np.array_equal(q2, qcount) and np.array_equal(e2, ent)
    for src, dst in list(zip(ids.tolist(), to.tolist()))[:40] + [(k, int(to[np.flatnonzero(ids == k)[0]])) for k in (299, 7, 100)]:
        assert eng.queue_of(dst) == ref.queue_of(src)
    eng.close()


# ---------------------------------------------------------------- 3. classed engine
QC = [(4, 1, 10_000_000, 1, 0), (3, 1, 10_000_000, 5, 1), (6, 2, 10_000_000, 40, 0)]


def test_classed_engine_wraps_and_imports_by_class(engine_lib, oracle_lib, gpu):
    """Class of key k = k % 3.  Every batch holds the keys of one class, so that the class's
    own oracle numbers its requests as the engine does."""
    from distributedratelimiting.redis_amd import TbeError
    n_keys = 2_500
    rng = np.random.default_rng(3)
    eng = _engine(n_keys, QC[0], classes=QC[1:])
    refs = [_ref(n_keys, c) for c in QC]
    cls = (np.arange(n_keys) % 3).astype(np.uint8)
    eng.set_class(np.arange(n_keys, dtype=np.uint64), cls)
    base = 0
    queued = np.zeros(n_keys, dtype=np.int64)
    for s in range(5):
        for c, ref in enumerate(refs):
            n = 6_000
            keys = (rng.integers(0, n_keys // 3, n) * 3 + c).astype(np.uint64)
            if c == 2:                                         # thirty busy keys of class 2: long queues
                keys[: n // 2] = (rng.integers(0, 30, n // 2) * 3 + 2).astype(np.uint64)
            permits = rng.choice(np.array([1, 1, 2, 3], dtype=np.int32), n)
            if c == 2:
                permits[: n // 2] = 1                          # forty entries fill their ring of forty
            ts = T0 + s * 2_000_000 + c * 1000 + np.sort(rng.integers(0, 1000, n)).astype(np.int64)
            st, rem, (ec, ei) = eng.wait_batch(keys, permits, ts, base)
            st_ref, rem_ref, ec_ref, ei_ref = ref.acquire_batch(keys, permits, ts, base)
            assert np.array_equal(st, st_ref) and np.array_equal(rem, rem_ref) and np.array_equal(ei, ei_ref), (s, c)
            queued += np.bincount(keys[st_ref == QUEUED].astype(np.int64), minlength=n_keys)
            base += n
        tick = T0 + s * 2_000_000 + 1_000_000
        lk, li, lr = eng.refresh(tick)
        logs = [r.refresh(tick) for r in refs]
        k_ref = np.concatenate([x[0] for x in logs])
        o = np.argsort(k_ref, kind="stable")
        assert np.array_equal(lk, k_ref[o]) and np.array_equal(li, np.concatenate([x[1] for x in logs])[o])
    queue_of = lambda k: refs[k % 3].queue_of(k)
    ids = rng.permutation(n_keys).astype(np.uint64)
    qcount, start, ent = _want(queue_of, ids)
    total = int(start[-1])
    ring = np.array([max(1, c[3]) for c in QC])[cls[ids.astype(np.int64)]]
    wrapped = [int(((qcount > 0) & (queued[ids.astype(np.int64)] > ring) & (cls[ids.astype(np.int64)] == c)).sum())
               for c in range(3)]
    print("wrapped keys per class", wrapped, "longest queue", int(qcount.max()), "entries", total)
    assert min(wrapped) >= 20 and qcount.max() > 8
    q, s_, e, tot = _export_device(eng, gpu, ids, total)
    assert tot == total and np.array_equal(q, qcount) and np.array_equal(s_, start) and np.array_equal(e[:total], ent)
    # clear everything, then import under the classes' limits
    eng.queue_export_ids(ids, clear=True)
    empty = _snapshot(eng)
    w = lambda i, p: (i << 16) | p
    refusals = {
        "longer than class 0's ring": ([0], [2], [w(1, 1), w(2, 1)]),
        "permits above class 1's TokenLimit": ([1], [1], [w(1, 4)]),
        "permits above class 1's QueueLimit": ([1], [2], [w(1, 3), w(2, 3)]),
        "longer than class 1's ring": ([1], [6], [w(i, 1) for i in range(6)]),
        "permits above class 2's QueueLimit": ([2], [7], [w(i, 6) for i in range(7)]),
    }
    for why, (k, c, ents) in refusals.items():
        with pytest.raises(TbeError):
            eng.queue_import_ids(k, c, ents)
        assert _same(empty, _snapshot(eng)), why
    # the same shapes inside the limits are taken
    eng.queue_import_ids([0, 1, 2], [1, 5, 7], [w(9, 1)] + [w(i, 1) for i in range(5)] + [w(i, 5) for i in range(6)] + [w(77, 6)])
    assert eng.queue_of(0) == [(9, 1)] and eng.queue_of(1) == [(i, 1) for i in range(5)]
    assert eng.queue_of(2) == [(i, 5) for i in range(6)] + [(77, 6)]
    eng.queue_export_ids([0, 1, 2], clear=True)
    # and the oracle's queues go back, each onto another id of its class
    to = (ids + np.uint64(3)) % np.uint64(2_499)               # 2,499 = 3 * 833: the class is kept
    assert np.array_equal(cls[to.astype(np.int64)], cls[ids.astype(np.int64)]) and len(set(to.tolist())) == n_keys - 1
    keep = ids != np.uint64(2_499)                             # (id 2,499 would collide with id 0's target)
    qc2, st2, en2 = _want(queue_of, ids[keep])
    eng.queue_import_ids(to[keep], qc2, en2)
    q2, s2, e2, tot2 = eng.queue_export_ids(to[keep])
    assert np.array_equal(q2, qc2) and np.array_equal(e2, en2)
    eng.close()


# ---------------------------------------------------------------- 4. a round trip decides identically
@pytest.mark.parametrize("order", [0, 1], ids=["oldest", "newest"])
def test_round_trip_onto_permuted_ids_decides_identically(engine_lib, oracle_lib, gpu, order):
    """Engine A runs steps 0-1; rows and queues move onto engine B at permuted ids; B and the
    oracle run steps 2-3 with a cancel of an entry queued before the move."""
    n_keys = 5_000
    opts = (4, 1, 10_000_000, 8, order)
    rng = np.random.default_rng(21 + order)
    a, b, ref = _engine(n_keys, opts), _engine(n_keys, opts), _ref(n_keys, opts)
    _, base = _drive(a, ref, rng, n_keys, 2, 4, _small_permits)
    perm = rng.permutation(n_keys).astype(np.uint64)           # key k lives at id perm[k] of B
    ids = np.arange(n_keys, dtype=np.uint64)
    v, t = a.export_state()
    vb, tb = np.empty_like(v), np.empty_like(t)
    vb[perm.astype(np.int64)], tb[perm.astype(np.int64)] = v, t
    b.import_state(vb, tb)
    qcount, start, ent, total = a.queue_export_ids(ids, clear=True)
    want = _want(ref.queue_of, ids)
    assert np.array_equal(qcount, want[0]) and np.array_equal(ent, want[2]) and total >= 1_000
    b.queue_import_ids(perm, qcount, ent)
    assert b.refresh_bound() >= min(total, n_keys * 4)         # a tick grants at most TokenLimit per key
    # cancel entries that were queued before the move
    ck = np.flatnonzero(qcount > 1)[:300].astype(np.uint64)
    cid = np.array([ref.queue_of(int(k))[1][0] for k in ck], dtype=np.int64)
    hit = b.cancel(perm[ck.astype(np.int64)], cid)
    assert np.array_equal(hit, ref.cancel(ck, cid)) and hit.all()
    _drive(b, ref, rng, n_keys, 2, 4, _small_permits, id_base=base, t0=T0 + 2 * 2_000_000, keymap=perm)
    for k in rng.integers(0, n_keys, 400).tolist():
        assert b.queue_of(int(perm[k])) == ref.queue_of(k)
    qb = b.queue_export_ids(perm)
    wb = _want(ref.queue_of, ids)
    assert np.array_equal(qb[0], wb[0]) and np.array_equal(qb[2], wb[2])
    a.close()
    b.close()


# ---------------------------------------------------------------- 5. import refusals
def test_import_refusals_change_nothing(engine_lib, oracle_lib, gpu):
    """One case per rule of the header, device form (sticky, raises at synchronize) and host
    form (TBE_EINVAL); the mutated position lies in the second tile of the id list."""
    import torch
    from distributedratelimiting.redis_amd import TbeError
    n_keys = 4_000
    opts = (4, 1, 10_000_000, 8, 0)
    rng = np.random.default_rng(9)
    eng, ref = _engine(n_keys, opts), _ref(n_keys, opts)
    _drive(eng, ref, rng, n_keys, 1, 4, _small_permits, pool=np.arange(0, n_keys, 4, dtype=np.uint64))
    have = np.array([len(ref.queue_of(k)) for k in range(n_keys)])
    free, busy = np.flatnonzero(have == 0), np.flatnonzero(have > 0)
    print("keys with an empty queue", len(free), "with entries", len(busy))
    assert len(free) >= TILE + 200 and len(busy) >= 100
    ids = rng.permutation(free).astype(np.uint64)
    n = len(ids)
    qcount = rng.integers(0, 4, n).astype(np.uint32)
    qcount[TILE + 7] = 3
    ne = int(qcount.sum())
    ent = ((np.arange(ne, dtype=np.uint64) + np.uint64(1 << 30)) << np.uint64(16)) | rng.integers(1, 3, ne).astype(np.uint64)
    at = int(qcount[: TILE + 7].sum())                         # first entry of the mutated id
    before = _snapshot(eng)

    def case(why, ids=ids, qcount=qcount, ent=ent, n_entries=None):
        d_ids, d_q = _dev(np.asarray(ids, dtype=np.uint64), gpu), _dev(np.asarray(qcount, dtype=np.uint32), gpu)
        d_e = _dev(np.asarray(ent, dtype=np.uint64), gpu)
        torch.cuda.synchronize()
        eng.queue_import_ids_device(d_ids, d_q, d_e, n_entries=n_entries)
        torch.cuda.synchronize()
        with pytest.raises(TbeError):
            eng.synchronize()
        assert _same(before, _snapshot(eng)), why + " (device form)"
        if n_entries is None:                                  # (the host form takes the entries' own length)
            with pytest.raises(TbeError):
                eng.queue_import_ids(ids, qcount, ent)
            eng.synchronize()
            assert _same(before, _snapshot(eng)), why + " (host form)"

    def mutated(a, i, x):
        a = a.copy()
        a[i] = x
        return a

    case("id >= n_keys", ids=mutated(ids, TILE + 7, n_keys))
    case("target queue not empty", ids=mutated(ids, TILE + 7, busy[0]))
    case("count above the ring length", qcount=mutated(qcount, TILE + 7, 9),
         ent=np.concatenate([ent[:at], np.full(6, (5 << 16) | 1, dtype=np.uint64), ent[at:]]))
    case("permits < 1", ent=mutated(ent, at + 1, np.uint64(7 << 16)))
    case("permits above TokenLimit", ent=mutated(ent, at + 1, np.uint64((7 << 16) | 5)))
    case("permits above QueueLimit", ent=np.concatenate([ent[:at], np.full(3, (5 << 16) | 3, dtype=np.uint64), ent[at + 3:]]))
    case("request id >= 2^47", ent=mutated(ent, at + 2, np.uint64((1 << 63) | 1)))
    case("counts sum below n_entries", ent=np.concatenate([ent, ent[:1]]))
    case("counts sum above n_entries", ent=ent[:-1])
    case("n_entries one more than the counts", ent=np.concatenate([ent, ent[:1]]), n_entries=ne + 1)
    case("n_entries one less than the counts", n_entries=ne - 1)
    # the unmutated call is taken
    eng.queue_import_ids(ids, qcount, ent)
    q, s, e, tot = eng.queue_export_ids(ids)
    assert np.array_equal(q, qcount) and np.array_equal(e, ent)
    after = _snapshot(eng)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])   # rows untouched
    for k in busy[:50].tolist():
        assert eng.queue_of(k) == ref.queue_of(k)
    eng.close()


# ---------------------------------------------------------------- 6. the drain bound
def test_bound_and_host_refresh_cover_imported_entries(engine_lib, gpu):
    """A fresh engine: every bucket is full, so a tick grants an imported entry of p <=
    TokenLimit permits and a second one while their sum stays <= TokenLimit."""
    n_keys = 1_000
    eng = _engine(n_keys, (4, 1, 10_000_000, 8, 0))
    assert eng.refresh_bound() == 0
    ids = np.arange(0, n_keys, 2, dtype=np.uint64)             # 500 keys, two entries each: 3 + 2 permits
    qcount = np.full(len(ids), 2, dtype=np.uint32)
    rid = np.arange(2 * len(ids), dtype=np.uint64) + np.uint64(1 << 40)
    ent = (rid << np.uint64(16)) | np.tile(np.array([3, 2], dtype=np.uint64), len(ids))
    eng.queue_import_ids(ids, qcount, ent)
    assert eng.refresh_bound() >= len(ent)
    lk, li, lr = eng.refresh(T0)
    assert np.array_equal(lk, ids) and np.array_equal(li, rid[0::2].astype(np.int64)) and np.all(lr == 1)
    assert eng.refresh_bound() >= len(ids)
    lk, li, lr = eng.refresh(T0 + 1_000_000)                   # one more token: 1 + 1 = 2 permits
    assert np.array_equal(lk, ids) and np.array_equal(li, rid[1::2].astype(np.int64)) and np.all(lr == 0)
    assert eng.queue_export_ids(np.arange(n_keys, dtype=np.uint64))[3] == 0
    eng.close()


# ---------------------------------------------------------------- 7. other kinds refuse
def test_other_kinds_refuse(engine_lib, gpu):
    import ctypes
    import torch
    from distributedratelimiting.redis_amd import ApproximateEngine, TbeError, TokenBucketEngine, _capi
    ap = ApproximateEngine(100, 4, 1, 10_000_000, 8, device=0)
    d_ids = torch.arange(4, dtype=torch.int64, device=gpu)
    d_q = torch.zeros(4, dtype=torch.int32, device=gpu)
    d_n = torch.zeros(1, dtype=torch.int64, device=gpu)
    d_c = torch.zeros(4, dtype=torch.int64, device=gpu)
    calls = [lambda: ap.queue_export_ids([0, 1]),
             lambda: ap.queue_export_ids_device(d_ids, d_q, None, None, d_n),
             lambda: ap.queue_import_ids([0], [0], []),
             lambda: ap.queue_import_ids_device(d_ids, d_q, None),
             lambda: ap.queue_migrate_out(T0, np.zeros(4, dtype=np.uint64), None, 2, 0),
             lambda: ap.queue_migrate_out_device(T0, d_ids, None, 2, 0, None, d_c)]
    for f in calls:
        with pytest.raises(TbeError) as ex:
            f()
        assert ex.value.status == _capi.TBE_EINVAL
    ap.close()
    tb = TokenBucketEngine(100, 4, 1, 10_000_000, device=0)
    lib, h = _capi.load(), tb.handle
    n = ctypes.c_uint64()
    p = lambda t: t.data_ptr()
    assert lib.tbe_queue_export_ids_device(h, p(d_ids), 4, p(d_q), None, None, 0, p(d_n), 0, None) == _capi.TBE_EINVAL
    assert lib.tbe_queue_export_ids(h, None, 0, None, None, None, 0, ctypes.byref(n), 0) == _capi.TBE_EINVAL
    assert lib.tbe_queue_import_ids_device(h, p(d_ids), p(d_q), 4, None, 0, None) == _capi.TBE_EINVAL
    assert lib.tbe_queue_import_ids(h, None, None, 0, None, 0) == _capi.TBE_EINVAL
    kof = np.zeros(4, dtype=np.uint64)
    cnt = np.zeros(4, dtype=np.uint64)
    assert lib.tbe_queue_migrate_out_ids(h, T0, 0, 4, kof.ctypes.data, None, 2, 0, None, 0, cnt.ctypes.data, None, 0,
                                         None) == _capi.TBE_EINVAL
    assert lib.tbe_queue_migrate_out_ids_device(h, T0, 0, 4, p(d_ids), None, 2, 0, None, 0, p(d_c), None, 0, None,
                                                None) == _capi.TBE_EINVAL
    tb.synchronize()
    tb.close()
