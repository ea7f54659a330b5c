"""Lease statistics (TBE_FLAG_STATS; tbe_stats_* in include/tbe.h): per-key
ok / failed counters and the engine totals, counted on the device behind every batch, and the
batched query {ok, failed, available, queued}.

Expected counts come from the oracles (oracle/semantics.py), never from the engine's own
replies: the oracle decides every request, its decisions are counted per key with numpy, and
the engine's replies are compared with the oracle's on the way.  Every comparison is exact.

T is k_stats_batch's tile in requests and S the slot count of its LDS table
(csrc/tbe_stats.hpp), as the binding states them."""
import ctypes

import numpy as np
import pytest

from oracle import semantics as sem

pytestmark = pytest.mark.gpu

ABSENT = np.iinfo(np.int64).min
T0 = 1_760_000_000_000_000
LIMIT = (10, 1, 10_000_000)         # TokenLimit 10, one token per second: TTL 10 s


def _ts():
    from distributedratelimiting.redis_amd import _capi
    return _capi.STATS_TILE, _capi.STATS_SLOTS


def _tb(n_keys, stats=True, **kw):
    from distributedratelimiting.redis_amd import TokenBucketEngine
    return TokenBucketEngine(n_keys, *LIMIT, device=0, stats=stats, **kw)


def _table(opts=LIMIT):
    return sem.TokenBucketTable(sem.TokenBucketConfig.from_options(*opts))


class _Want:
    """The counters the oracle's decisions add up to."""

    def __init__(self, n_keys):
        self.ok = np.zeros(n_keys, np.uint64)
        self.failed = np.zeros(n_keys, np.uint64)
        self.tot = [0, 0]

    def count(self, keys, status):
        keys = np.asarray(keys, np.int64)
        status = np.asarray(status)
        np.add.at(self.ok, keys[status == 1], np.uint64(1))
        np.add.at(self.failed, keys[status == 0], np.uint64(1))
        self.tot[0] += int((status == 1).sum())
        self.tot[1] += int((status == 0).sum())

    def add(self, which, key, m=1):
        (self.ok if which == 0 else self.failed)[key] += np.uint64(m)
        self.tot[which] += m

    def check(self, eng, totals=True):
        ok, failed = eng.stats_export()
        bad = np.flatnonzero((ok != self.ok) | (failed != self.failed))
        assert bad.size == 0, (bad[:8], ok[bad[:8]], self.ok[bad[:8]], failed[bad[:8]], self.failed[bad[:8]])
        if totals:   # (case 14: the totals are the sums wherever nothing was zeroed)
            assert eng.stats_totals() == (int(ok.sum()), int(failed.sum())) == tuple(self.tot)


def _decide(table, keys, permits, ts):
    g, r = table.acquire_batch(keys, permits, ts)
    return np.asarray(g, np.uint8), np.asarray(r, np.int32)


def _batch(rng, n_keys, n, t_start, permits=(0, 1, 1, 2, 4)):
    keys = rng.integers(0, n_keys, n).astype(np.uint64)
    p = rng.choice(permits, n).astype(np.int32)
    ts = t_start + np.cumsum(rng.integers(0, 40, n)).astype(np.int64)
    return keys, p, ts


def _dev(a, gpu):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(gpu)


# ---------------------------------------------------------------- 1. sizes
def test_sizes(engine_lib, gpu):
    T, _ = _ts()
    n_keys = 1_000
    rng = np.random.default_rng(1)
    eng, table, want = _tb(n_keys), _table(), _Want(n_keys)
    t = T0
    for n in (1, 63, 64, T - 1, T, T + 1, 3 * T + 17):
        keys, p, ts = _batch(rng, n_keys, n, t)
        t = int(ts[-1]) + 1_000
        g_ref, r_ref = _decide(table, keys, p, ts)
        g, r = eng.acquire_batch(keys, p, ts)
        assert np.array_equal(g, g_ref) and np.array_equal(r, r_ref), n
        want.count(keys, g_ref)
        want.check(eng)
    assert want.tot[0] > 1_000 and want.tot[1] > 1_000       # grants and denies both
    # the batched query reads the same counters, keys repeated
    q = rng.integers(0, n_keys, 5_000).astype(np.uint64)
    ok, failed, _, queued = eng.statistics(q, t)
    assert np.array_equal(ok, want.ok[q.astype(np.int64)]) and np.array_equal(failed, want.failed[q.astype(np.int64)])
    assert not queued.any()
    eng.close()


# ---------------------------------------------------------------- 2. one key
def test_one_key(engine_lib, gpu):
    T, _ = _ts()
    n_keys, n = 1_000, 3 * T + 5
    rng = np.random.default_rng(2)
    eng, table, want = _tb(n_keys), _table(), _Want(n_keys)
    keys = np.full(n, 7, np.uint64)
    p = rng.choice([0, 1, 2], n).astype(np.int32)           # zero-permit requests are always granted
    ts = T0 + np.cumsum(rng.integers(0, 900, n)).astype(np.int64)
    g_ref, r_ref = _decide(table, keys, p, ts)
    g, r = eng.acquire_batch(keys, p, ts)
    assert np.array_equal(g, g_ref) and np.array_equal(r, r_ref)
    want.count(keys, g_ref)
    assert min(want.tot) > T
    want.check(eng)
    eng.close()


# ---------------------------------------------------------------- 3. table overflow
def test_table_overflow(engine_lib, gpu):
    _, S = _ts()
    n_keys = 4 * S
    rng = np.random.default_rng(3)
    eng, table, want = _tb(n_keys), _table(), _Want(n_keys)
    keys = rng.permutation(n_keys).astype(np.uint64)        # every tile: 4096 distinct keys, 2048 slots
    p = rng.choice([1, 11], n_keys).astype(np.int32)        # 11 > TokenLimit: denied
    ts = np.full(n_keys, T0, np.int64)
    g_ref, r_ref = _decide(table, keys, p, ts)
    g, r = eng.acquire_batch(keys, p, ts)
    assert np.array_equal(g, g_ref) and np.array_equal(r, r_ref)
    want.count(keys, g_ref)
    want.check(eng)
    assert set((want.ok + want.failed).tolist()) == {1}
    eng.close()


# ---------------------------------------------------------------- 4. accumulation on the fast path
def test_back_to_back_on_the_fast_path(engine_lib, gpu):
    """Five device batches with no synchronise between them on a packed, pipelined engine; key
    4242 takes 4,096 requests of every batch (kHotMin is 2,048), so it has a run of its own
    from the third batch.  n_keys = 10,000 is the smoke shape: the smallest table the suite
    runs packed with hot runs and two passes; 16,384 requests make every batch dense."""
    import torch
    n_keys, n, nb = 10_000, 16_384, 5
    rng = np.random.default_rng(4)
    eng, table, want = _tb(n_keys), _table(), _Want(n_keys)
    a, b, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    assert eng._lib.tbe_layout(eng.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
    assert c.value & 7 == 7, c.value                        # packed records, hot-key runs, pipelined
    assert not eng.batch_format(n)["sparse"]
    host, ins, outs = [], [], []
    t = T0
    for _ in range(nb):
        keys, p, ts = _batch(rng, n_keys, n, t, permits=(0, 1, 1, 2))
        keys[rng.choice(n, 4_096, replace=False)] = 4242
        t = int(ts[-1]) + 2_000_000
        host.append((keys, p, ts))
        ins.append((_dev(keys, gpu), _dev(p, gpu), _dev(ts, gpu)))
        outs.append((torch.empty(n, dtype=torch.uint8, device=gpu), torch.empty(n, dtype=torch.int32, device=gpu)))
    torch.cuda.synchronize()
    for i in range(nb):
        eng.acquire_batch_device(*ins[i], *outs[i])
    eng.synchronize()
    for i in range(nb):
        g_ref, r_ref = _decide(table, *host[i])
        assert np.array_equal(outs[i][0].cpu().numpy(), g_ref), i
        assert np.array_equal(outs[i][1].cpu().numpy(), r_ref), i
        want.count(host[i][0], g_ref)
    assert int(want.ok[4242] + want.failed[4242]) >= nb * 4_096
    want.check(eng)
    eng.close()


# ---------------------------------------------------------------- 5. other layouts
CLASSES = [(10, 1, 10_000_000), (3, 1, 30_000_000), (100, 50, 1_000_000), (5, 10, 10_000_000)]


def _classed(n_keys, rng, stats=True):
    """A classed engine and the shared-state model of tests/test_gpu_classes.py: one
    TokenBucketTable per class over one state dict."""
    from distributedratelimiting.redis_amd import TokenBucketEngine
    eng = TokenBucketEngine(n_keys, *CLASSES[0], device=0, classes=CLASSES[1:], stats=stats)
    cls = rng.integers(0, 4, n_keys).astype(np.uint8)
    eng.set_class(np.arange(n_keys, dtype=np.uint64), cls)
    tables = [_table(c) for c in CLASSES]
    for t in tables[1:]:
        t.state = tables[0].state
    return eng, cls, tables


def _decide_classed(tables, cls, keys, permits, ts):
    g = np.empty(len(keys), np.uint8)
    r = np.empty(len(keys), np.int32)
    for i, (k, p, t) in enumerate(zip(keys.tolist(), permits.tolist(), ts.tolist())):
        ok, rem = tables[cls[k]].acquire(k, p, t)
        g[i], r[i] = ok, rem
    return g, r


def test_classed_engine(engine_lib, gpu):
    n_keys, n = 3_000, 20_000
    rng = np.random.default_rng(5)
    eng, cls, tables = _classed(n_keys, rng)
    assert not eng.layout()["packed"]                       # the wide path
    want = _Want(n_keys)
    t = T0
    for _ in range(2):
        keys, p, ts = _batch(rng, n_keys, n, t, permits=(0, 1, 2, 4, 6))
        t = int(ts[-1]) + 1_500_000
        g_ref, r_ref = _decide_classed(tables, cls, keys, p, ts)
        g, r = eng.acquire_batch(keys, p, ts)
        assert np.array_equal(g, g_ref) and np.array_equal(r, r_ref)
        want.count(keys, g_ref)
        want.check(eng)
    eng.close()


def test_sparse_batch(engine_lib, gpu):
    n_keys, n = 1_000_000, 5_000                            # R = 1024: fewer than R/8 requests per bucket
    rng = np.random.default_rng(6)
    eng, table, want = _tb(n_keys), _table(), _Want(n_keys)
    out = (ctypes.c_uint32 * 9)()
    assert eng._lib.tbe_batch_format(eng.handle, n, out, 9) == 0 and out[8] == 1
    t = T0
    for _ in range(2):
        keys, p, ts = _batch(rng, n_keys, n, t, permits=(1, 4, 11))
        keys[:600] = 31_337                                 # one dense bucket among the sparse ones
        t = int(ts[-1]) + 1_000
        g_ref, r_ref = _decide(table, keys, p, ts)
        g, r = eng.acquire_batch(keys, p, ts)
        assert np.array_equal(g, g_ref) and np.array_equal(r, r_ref)
        want.count(keys, g_ref)
        want.check(eng)
    eng.close()


# ---------------------------------------------------------------- 6. invalid batch
def test_invalid_batch_counts_nowhere(engine_lib, gpu):
    import torch
    from distributedratelimiting.redis_amd import TbeError
    n_keys, n = 10_000, 9_000
    rng = np.random.default_rng(7)
    eng, table, want = _tb(n_keys), _table(), _Want(n_keys)
    host, ins, outs = [], [], []
    for i in range(3):
        keys, p, ts = _batch(rng, n_keys, n, T0 + i * 1_000_000)
        if i == 1:
            keys[777] = n_keys                              # out of range: the whole batch is skipped
        host.append((keys, p, ts))
        ins.append((_dev(keys, gpu), _dev(p, gpu), _dev(ts, gpu)))
        outs.append((torch.empty(n, dtype=torch.uint8, device=gpu), torch.empty(n, dtype=torch.int32, device=gpu)))
    torch.cuda.synchronize()
    for i in range(3):
        eng.acquire_batch_device(*ins[i], *outs[i])
    with pytest.raises(TbeError) as ei:
        eng.synchronize()
    assert ei.value.status == 1
    for i in (0, 2):
        g_ref, _ = _decide(table, *host[i])
        assert np.array_equal(outs[i][0].cpu().numpy(), g_ref)
        want.count(host[i][0], g_ref)
    want.check(eng)
    # the query's own invalid call writes nothing and surfaces at synchronize
    d_ok = torch.full((4,), -5, dtype=torch.int64, device=gpu)
    d_keys = _dev(np.array([1, 2, n_keys, 3], np.uint64), gpu)
    torch.cuda.synchronize()
    eng.statistics_device(d_keys, T0, d_ok=d_ok)
    with pytest.raises(TbeError):
        eng.synchronize()
    assert d_ok.cpu().tolist() == [-5] * 4
    with pytest.raises(TbeError):
        eng.statistics(np.array([n_keys], np.uint64), T0)
    with pytest.raises(TbeError):
        eng.statistics(np.array([1], np.uint64), -1)        # ts_us < 0 on a clocked kind
    eng.synchronize()
    eng.close()


# ---------------------------------------------------------------- 7. host-buffer call
def test_host_call_from_pinned_buffers(engine_lib, gpu):
    """Pageable and page-locked buffers through the unchunked host call.  (The chunked path
    starts at 2 x 4M requests with no knob below that: tests/test_gpu_pinned.py reaches it
    with 16M-request batches, a workload-sized case this file does not repeat.)"""
    from distributedratelimiting.redis_amd.engine import PinnedArray
    T, _ = _ts()
    n_keys, n = 2_000, 2 * T + 9
    rng = np.random.default_rng(8)
    eng, table, want = _tb(n_keys), _table(), _Want(n_keys)
    bufs = [PinnedArray(n, d) for d in (np.uint64, np.int32, np.int64, np.uint8, np.int32)]
    bk, bp, bt, bg, br = (b.array for b in bufs)
    for i in range(2):
        keys, p, ts = _batch(rng, n_keys, n, T0 + i * 3_000_000)
        g_ref, r_ref = _decide(table, keys, p, ts)
        if i == 0:
            g, r = eng.acquire_batch(keys, p, ts)
        else:
            bk[:], bp[:], bt[:] = keys, p, ts
            g, r = eng.acquire_batch(bk, bp, bt, bg, br)
        assert np.array_equal(g, g_ref) and np.array_equal(r, r_ref)
        want.count(keys, g_ref)
        want.check(eng)
    for b in bufs:
        b.free()
    eng.close()


# ---------------------------------------------------------------- 8. queueing kind
@pytest.mark.parametrize("order", [sem.OLDEST_FIRST, sem.NEWEST_FIRST], ids=["oldest", "newest"])
def test_queueing_kind(engine_lib, gpu, order):
    import torch
    from distributedratelimiting.redis_amd import QueueingTokenBucketEngine
    n_keys, qlimit, n = 64, 4, 4_096
    opts = (5, 1, 10_000_000)                               # TokenLimit 5, one token per second
    rng = np.random.default_rng(80 + order)
    eng = QueueingTokenBucketEngine(n_keys, *opts, qlimit, order, device=0, stats=True)
    ref = sem.QueueingTokenBucketTable(sem.TokenBucketConfig.from_options(*opts), qlimit, order)
    want = _Want(n_keys)
    requests = np.zeros(n_keys, np.int64)                   # non-rejected requests per key
    cancelled = np.zeros(n_keys, np.int64)
    evictions = 0
    rid, t = 0, T0

    def gen():
        keys = rng.integers(0, n_keys, n).astype(np.uint64)
        p = rng.choice([0, 1, 1, 2, 3, 6], n).astype(np.int32)   # 6 > TokenLimit: REJECTED
        ts = t + np.sort(rng.integers(0, 900_000, n)).astype(np.int64)
        return keys, p, ts

    def wait_oracle(keys, p, ts, base):
        nonlocal evictions
        st = np.empty(n, np.uint8)
        for i, (k, pp, tt) in enumerate(zip(keys.tolist(), p.tolist(), ts.tolist())):
            status, _, ev = ref.acquire(k, pp, tt, base + i)
            st[i] = status
            if ev:                                          # the evicted entries' key is the causing request's
                want.add(1, k, len(ev))
                evictions += len(ev)
        want.count(keys, st)
        np.add.at(requests, keys.astype(np.int64)[st != sem.ST_REJECTED], 1)
        return st

    def drain_oracle(ts_us):
        log = ref.refresh(ts_us)
        for k, _, _ in log:
            want.add(0, k)
        return log

    for rnd in range(4):
        # a wait batch from host buffers
        keys, p, ts = gen()
        st_ref = wait_oracle(keys, p, ts, rid)
        st, _, _ = eng.wait_batch(keys, p, ts, rid)
        assert np.array_equal(st, st_ref), rnd
        rid += n
        want.check(eng)
        # an attempt batch: lease or fail
        t += 1_000_000
        keys, p, ts = gen()
        st_ref = np.array([ref.attempt(k, pp, tt)[0] for k, pp, tt in zip(keys.tolist(), p.tolist(), ts.tolist())],
                          np.uint8)
        want.count(keys, st_ref)
        np.add.at(requests, keys.astype(np.int64)[st_ref != sem.ST_REJECTED], 1)
        st, _ = eng.attempt_batch(keys, p, ts)
        assert np.array_equal(st, st_ref), rnd
        want.check(eng)
        # a replenish tick
        t += 2_000_000
        log = drain_oracle(t)
        k_log, id_log, _ = eng.refresh(t)
        assert list(zip(k_log.tolist(), id_log.tolist())) == [(k, i) for k, i, _ in log]
        want.check(eng)
        # a device wait batch with a fused tick
        t += 1_000_000
        keys, p, ts = gen()
        st_ref = wait_oracle(keys, p, ts, rid)
        tick = int(ts[-1]) + 1_500_000
        log = drain_oracle(tick)
        cap = n + n_keys * qlimit
        d_st = torch.empty(n, dtype=torch.uint8, device=gpu)
        d_rem = torch.empty(n, dtype=torch.int32, device=gpu)
        d_ks = torch.empty(cap, dtype=torch.int64, device=gpu)
        d_id = torch.empty(cap, dtype=torch.int64, device=gpu)
        d_lr = torch.empty(cap, dtype=torch.int32, device=gpu)
        d_cnt = torch.zeros(1, dtype=torch.int32, device=gpu)
        d_in = (_dev(keys, gpu), _dev(p, gpu), _dev(ts, gpu))
        torch.cuda.synchronize()
        eng.wait_batch_tick_device(*d_in, d_st, d_rem, rid, tick, d_ks, d_id, d_lr, d_cnt)
        eng.synchronize()
        assert np.array_equal(d_st.cpu().numpy(), st_ref), rnd
        assert int(d_cnt.item()) == len(log)
        rid += n
        t = tick + 500_000
        want.check(eng)
        # cancel some of what is queued (and one id that is not)
        held = [(k, i) for k in range(n_keys) for i, _ in ref.queue_of(k)]
        pick = held[::3] + [(0, rid + 99)]
        exp = np.array([ref.cancel(k, i) for k, i in pick], np.uint8)
        got = eng.cancel(np.array([k for k, _ in pick], np.uint64), np.array([i for _, i in pick], np.int64))
        assert np.array_equal(got, exp) and exp[:-1].all() and not exp[-1]
        np.add.at(cancelled, np.array([k for k, _ in pick[:-1]], np.int64), 1)
        want.check(eng)                                     # a cancelled wait is no lease
        # queued permits, and the per-key identity
        all_keys = np.arange(n_keys, dtype=np.uint64)
        ok, failed, _, queued = eng.statistics(all_keys, t)
        assert queued.tolist() == [ref.qsum.get(k, 0) for k in range(n_keys)]
        entries = np.array([len(ref.queue_of(k)) for k in range(n_keys)], np.int64)
        assert np.array_equal(ok.astype(np.int64) + failed.astype(np.int64) + entries + cancelled, requests)
    assert want.tot[0] and want.tot[1] and cancelled.sum() and entries.sum()
    assert (evictions > 0) == (order == sem.NEWEST_FIRST)
    eng.close()


# ---------------------------------------------------------------- 9. approximate kind
@pytest.mark.parametrize("n_clients", [2, 1], ids=["sync2", "refresh"])
@pytest.mark.parametrize("order", [sem.OLDEST_FIRST, sem.NEWEST_FIRST], ids=["oldest", "newest"])
def test_approximate_kind(engine_lib, gpu, order, n_clients):
    """wait = 0 and wait = 1 batches with zero-permit waits, the plain and the _retry form
    alternating; each epoch ends with tbe_approx_sync between 2 clients, or with
    tbe_approx_refresh of an only client."""
    import torch
    from distributedratelimiting.redis_amd import ApproximateEngine
    n_keys, n, limit, tokens, ticks, qlimit = 200, 3_000, 20, 10, 10_000_000, 6
    rng = np.random.default_rng(90 + order + 2 * n_clients)
    engines = [ApproximateEngine(n_keys, limit, tokens, ticks, qlimit, order, device=0, stats=True)
               for _ in range(n_clients)]
    clients = [sem.ApproxClient(limit, tokens, ticks, qlimit, order) for _ in range(n_clients)]
    table = sem.ApproxGlobalTable(clients[0].decay_rate)
    wants = [_Want(n_keys) for _ in range(n_clients)]
    counts = [torch.zeros(n_keys, dtype=torch.int32, device=gpu) for _ in range(n_clients)]
    torch.cuda.synchronize()
    rid = evictions = drained = 0
    all_keys = np.arange(n_keys, dtype=np.uint64)
    for epoch in range(3):
        for r in range(n_clients):
            for wait in (False, True):
                keys = rng.integers(0, n_keys, n).astype(np.uint64)
                p = rng.choice([0, 0, 1, 2, 3, 25], n).astype(np.int32)   # zero-permit waits; 25: REJECTED
                st_ref = np.empty(n, np.uint8)
                for i, (k, pp) in enumerate(zip(keys.tolist(), p.tolist())):
                    if wait:
                        st_ref[i], ev = clients[r].wait(k, pp, rid + i)
                        if ev:
                            wants[r].add(1, k, len(ev))
                            evictions += len(ev)
                    else:
                        st_ref[i] = clients[r].acquire(k, pp)
                wants[r].count(keys, st_ref)
                st = engines[r].acquire_batch(keys, p, wait=wait, id_base=rid, retry_after=bool(epoch % 2))[0]
                assert np.array_equal(st, st_ref), (epoch, r, wait)
                rid += n
                wants[r].check(engines[r])
        ts = T0 + epoch * 1_000_000
        if n_clients == 2:
            for r in range(2):
                engines[r].collect(counts[r])
            allc = torch.cat(counts)
            torch.cuda.synchronize()
            logs = [engines[r].sync(allc, 2, r, ts, 500_000) for r in range(2)]
        else:
            logs = [engines[0].refresh(ts)]
        exp_logs = sem.approx_refresh_all(clients, table, ts, 500_000 if n_clients == 2 else 0, range(n_keys))
        for r in range(n_clients):
            assert list(zip(logs[r][0].tolist(), logs[r][1].tolist())) == exp_logs[r]
            for k, _ in exp_logs[r]:
                wants[r].add(0, k)
            drained += len(exp_logs[r])
            wants[r].check(engines[r])
            _, _, avail, queued = engines[r].statistics(all_keys)
            assert avail.tolist() == [engines[r].local_state(k)[3] for k in range(n_keys)]
            assert avail.tolist() == [clients[r].available(clients[r].st(k)) for k in range(n_keys)]
            assert queued.tolist() == [clients[r].st(k).qcount for k in range(n_keys)]
    assert drained > 0 and (evictions > 0) == (order == sem.NEWEST_FIRST)
    for e in engines:
        e.close()


# ---------------------------------------------------------------- 10. available on the clocked kinds
def _avail_case(rng, classed, stats):
    """Rows absent, live and lapsed at the query time; (engine, expected available at tq, tq)."""
    n_keys, n = 2_000, 6_000
    if classed:
        eng, cls, tables = _classed(n_keys, rng, stats=stats)
    else:
        eng, cls, tables = _tb(n_keys, stats=stats), np.zeros(n_keys, np.uint8), [_table()]
    # keys 900..999: one early request each, lapsed by every class's TTL at the query time;
    # keys 0..899: requests up to 1.5 s before it; the upper half of the table stays absent
    keys = np.concatenate([np.arange(900, 1_000), rng.integers(0, 900, n - 100)]).astype(np.uint64)
    p = rng.choice([1, 2, 3], n).astype(np.int32)
    ts = T0 + np.concatenate([np.sort(rng.integers(0, 400_000, 100)),
                              np.sort(rng.integers(500_000, 9_000_000, n - 100))]).astype(np.int64)
    g_ref, r_ref = _decide_classed(tables, cls, keys, p, ts)
    g, r = eng.acquire_batch(keys, p, ts)
    assert np.array_equal(g, g_ref) and np.array_equal(r, r_ref)
    tq = T0 + 10_500_000     # class TTLs 10 s, 9 s, 1 s, 1 s: rows last granted early have lapsed
    want = []
    for k in range(n_keys):
        # (refill drops a lapsed row from the model as Redis does on access; the engine leaves it)
        _, x, prev = tables[cls[k]].refill(k, tq)
        want.append((int(x), prev is not None))
    return eng, cls, np.array([w[0] for w in want], np.int32), np.array([w[1] for w in want]), tq


@pytest.mark.parametrize("classed", [False, True], ids=["plain", "classed"])
def test_available(engine_lib, gpu, classed):
    rng = np.random.default_rng(100 + classed)
    eng, cls, want, live, tq = _avail_case(rng, classed, True)
    v0, t0 = eng.export_state()
    touched = t0 != ABSENT
    assert (~touched).any() and live.any() and (touched & ~live).any()      # absent, live, lapsed
    q = np.concatenate([np.arange(eng.n_keys), rng.integers(0, eng.n_keys, 500)]).astype(np.uint64)
    _, _, avail, queued = eng.statistics(q, tq)
    assert np.array_equal(avail, want[q.astype(np.int64)])
    cap = np.array([c[0] for c in CLASSES], np.int32)[cls] if classed else np.full(eng.n_keys, LIMIT[0], np.int32)
    assert np.array_equal(avail[: eng.n_keys][~live], cap[~live])       # absent or lapsed: the class's TokenLimit
    assert not queued.any()
    v1, t1 = eng.export_state()
    assert np.array_equal(t0, t1) and np.array_equal(v0.view(np.uint64), v1.view(np.uint64))   # nothing written
    eng.close()


# ---------------------------------------------------------------- 11. 64-bit carry
def test_carry_past_32_bits(engine_lib, gpu):
    n_keys = 1_000
    eng, table, want = _tb(n_keys), _table(), _Want(n_keys)
    want.ok[5] = np.uint64(2**32 - 3)
    want.failed[6] = np.uint64(2**32 - 1)
    want.tot = [2**32 - 3, 2**32 - 1]
    eng.stats_import(want.ok, want.failed)
    want.check(eng)                                          # the import moved the totals by the difference
    keys = np.array([5] * 12 + [6] * 12, np.uint64)
    p = np.array([1] * 8 + [11] * 4 + [1] * 2 + [11] * 10, np.int32)
    ts = np.full(24, T0, np.int64)
    g_ref, _ = _decide(table, keys, p, ts)
    assert g_ref[:12].sum() >= 5
    g, _ = eng.acquire_batch(keys, p, ts)
    assert np.array_equal(g, g_ref)
    want.count(keys, g_ref)
    assert int(want.ok[5]) > 2**32 and int(want.failed[6]) > 2**32
    want.check(eng)
    eng.stats_import(np.zeros(1, np.uint64), np.zeros(1, np.uint64), first=5)
    want.tot[0] -= int(want.ok[5])
    want.tot[1] -= int(want.failed[5])
    want.ok[5] = want.failed[5] = 0
    want.check(eng)
    eng.close()


# ---------------------------------------------------------------- 12. reclaim
def test_expired_zeroes_the_flagged_keys(engine_lib, gpu):
    import torch
    n_keys = 3_000
    rng = np.random.default_rng(12)
    eng, table, want = _tb(n_keys), _table(), _Want(n_keys)
    # keys 1500..1999 only in the first second (lapsed at the scan, TTL 10 s), keys 0..1499
    # after it, keys >= 2000 never
    keys = np.concatenate([rng.integers(1_500, 2_000, 3_000), rng.integers(0, 1_500, 6_000)]).astype(np.uint64)
    p = rng.choice([1, 4, 11], 9_000).astype(np.int32)
    ts = T0 + np.concatenate([np.sort(rng.integers(0, 1_000_000, 3_000)),
                              np.sort(rng.integers(1_000_000, 12_000_000, 6_000))]).astype(np.int64)
    g_ref, _ = _decide(table, keys, p, ts)
    g, _ = eng.acquire_batch(keys, p, ts)
    assert np.array_equal(g, g_ref)
    want.count(keys, g_ref)
    tq = int(ts[-1]) + 1_000_000
    d_dead = torch.zeros(n_keys, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    eng.expired_device(tq, d_dead, clear=False)
    eng.synchronize()
    dead = d_dead.cpu().numpy().astype(bool)
    gone = np.array([table.load(k, tq) is None for k in range(n_keys)])
    assert np.array_equal(dead, gone)
    busy_dead = dead & ((want.ok + want.failed) > 0)
    assert busy_dead.any() and (~dead).any()
    want.check(eng)                                          # clear == 0 zeroes none
    eng.expired_device(tq, d_dead, clear=True)
    eng.synchronize()
    tot = tuple(want.tot)
    want.ok[dead] = 0
    want.failed[dead] = 0
    want.check(eng, totals=False)                            # exactly the flagged keys
    assert eng.stats_totals() == tot                         # zeroing leaves the totals
    eng.close()


def test_approx_reset_zeroes_the_flagged_keys(engine_lib, gpu):
    import torch
    from distributedratelimiting.redis_amd import ApproximateEngine
    n_keys, n = 300, 4_000
    rng = np.random.default_rng(13)
    eng = ApproximateEngine(n_keys, 20, 10, 10_000_000, 4, 0, device=0, stats=True)
    cli = sem.ApproxClient(20, 10, 10_000_000, 4, 0)
    want = _Want(n_keys)
    keys = rng.integers(0, n_keys, n).astype(np.uint64)
    p = rng.choice([1, 2, 9], n).astype(np.int32)
    st_ref = np.array([cli.acquire(k, pp) for k, pp in zip(keys.tolist(), p.tolist())], np.uint8)
    st = eng.acquire_batch(keys, p, wait=False)[0]
    assert np.array_equal(st, st_ref)
    want.count(keys, st_ref)
    want.check(eng)
    flags = (np.arange(n_keys) % 3 == 0)
    d_flags = torch.from_numpy(flags.astype(np.uint8)).to(gpu)
    torch.cuda.synchronize()
    eng.reset_device(d_flags)
    eng.synchronize()
    tot = tuple(want.tot)
    want.ok[flags] = 0
    want.failed[flags] = 0
    want.check(eng, totals=False)
    assert eng.stats_totals() == tot
    eng.close()


def test_directory_reclaim_hands_on_a_zeroed_id(engine_lib, gpu):
    import torch
    from distributedratelimiting.redis_amd import TokenBucketEngine
    from distributedratelimiting.redis_amd.cluster import DeviceDirectory
    cap = 256
    with torch.cuda.stream(torch.cuda.Stream(gpu)):
        d = DeviceDirectory(cap, device=0)
        eng = TokenBucketEngine(cap, 5, 2, 10_000_000, device=0, stats=True)     # TTL 3 s
        table = _table((5, 2, 10_000_000))
        s = torch.cuda.current_stream(gpu).cuda_stream
        old = np.arange(1_000, 1_040, dtype=np.uint64)
        ids = d.assign(_dev(old, gpu))
        keys = np.repeat(ids.cpu().numpy().view(np.uint64), 4)
        p = np.tile(np.array([1, 2, 2, 6], np.int32), 40)
        ts = np.full(160, T0, np.int64)
        g_ref, _ = _decide(table, keys, p, ts)
        g = torch.empty(160, dtype=torch.uint8, device=gpu)
        r = torch.empty(160, dtype=torch.int32, device=gpu)
        eng.acquire_batch_device(_dev(keys, gpu), _dev(p, gpu), _dev(ts, gpu), g, r, stream=s)
        assert np.array_equal(g.cpu().numpy(), g_ref)
        ok, failed, _, _ = eng.statistics(keys[::4], T0)
        assert ok.tolist() == [3] * 40 and failed.tolist() == [1] * 40
        assert d.reclaim(eng, T0 + 4_000_000) == 40          # every bucket has lapsed
        new = np.arange(5_000, 5_040, dtype=np.uint64)
        ids2 = d.assign(_dev(new, gpu)).cpu().numpy().view(np.uint64)
        assert set(ids2.tolist()) == set(keys[::4].tolist())  # the ids are reused
        ok, failed, _, _ = eng.statistics(ids2, T0 + 4_000_000)
        assert not ok.any() and not failed.any()
        assert eng.stats_totals() == (120, 40)
        eng.close()
        d.close()


# ---------------------------------------------------------------- 13. flag off
def test_flag_off(engine_lib, gpu):
    from distributedratelimiting.redis_amd import TbeError, _capi
    rng = np.random.default_rng(101)                        # case 10's plain trace
    on, _, want, _, tq = _avail_case(rng, False, True)
    rng = np.random.default_rng(101)
    off, _, want_off, _, _ = _avail_case(rng, False, False)
    assert np.array_equal(want, want_off)
    q = np.arange(off.n_keys, dtype=np.uint64)
    ok, failed, avail, queued = off.statistics(q, tq)
    assert ok is None and failed is None and np.array_equal(avail, want) and not queued.any()
    assert np.array_equal(on.statistics(q, tq)[2], want)
    buf = np.zeros(off.n_keys, np.uint64)
    lib, h = off._lib, off.handle
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.tbe_stats_batch(h, q.ctypes.data, 4, tq, buf.ctypes.data, None, None, None) == _capi.TBE_EINVAL
    assert lib.tbe_stats_batch(h, q.ctypes.data, 4, tq, None, buf.ctypes.data, None, None) == _capi.TBE_EINVAL
    assert lib.tbe_stats_batch_device(h, 1, 4, tq, 1, None, None, None, None) == _capi.TBE_EINVAL   # (before any use)
    assert lib.tbe_stats_totals(h, ctypes.byref(a), ctypes.byref(b)) == _capi.TBE_EINVAL
    assert lib.tbe_stats_export(h, 0, 4, buf.ctypes.data, buf.ctypes.data) == _capi.TBE_EINVAL
    assert lib.tbe_stats_import(h, 0, 4, buf.ctypes.data, buf.ctypes.data) == _capi.TBE_EINVAL
    with pytest.raises(TbeError):
        off.stats_totals()
    # statistics decide nothing: same layout, same replies, same table on one more batch
    assert on.layout() == off.layout()
    keys, p, ts = _batch(rng, on.n_keys, 9_000, tq)
    g1, r1 = on.acquire_batch(keys, p, ts)
    g0, r0 = off.acquire_batch(keys, p, ts)
    assert np.array_equal(g1, g0) and np.array_equal(r1, r0)
    (v1, t1), (v0, t0) = on.export_state(), off.export_state()
    assert np.array_equal(t1, t0) and np.array_equal(v1.view(np.uint64), v0.view(np.uint64))
    on.close()
    off.close()


