"""RetryAfter of the approximate kind's failed leases, decided on the device per request
(tbe_approx_acquire_batch_retry / _retry_device; A:390-395):

    deficit    = Math.Max(0, ConsumedTokens + permitCount + _queueCount - TokenLimit)   // unchecked int32
    RetryAfter = TimeSpan.FromSeconds(deficit * FillRatePerSecond)

on the key's state at the request's own turn in arrival order.  Expected values: the oracle
client (oracle/semantics.py ApproxClient) driven request by request; whenever it answers
AP_FAILED the formula is evaluated on client.st(key) right after the call (a failure modifies
nothing, so that is the state at the decision).  The Python statement of the formula lives
here (retry_ticks), not in the oracle."""
import functools
from collections import namedtuple

import numpy as np
import pytest

from oracle.semantics import (AP_FAILED, AP_REJECTED, NEWEST_FIRST, OLDEST_FIRST, ApproxClient,
                              ApproxGlobalTable, approx_refresh_all, wrap32)

pytestmark = pytest.mark.gpu

S_US = 1_760_572_800 * 1_000_000
RETRY_NONE, RETRY_OVERFLOW = -1, 2 ** 63 - 1
TOKENS, TICKS = 10, 10_000_000


def retry_ticks(client, key, p):
    """.NET ticks of A:390-395 on the key's current state (int32 wrap, two f64 multiplies,
    truncation; TBE_RETRY_OVERFLOW where TimeSpan.FromSeconds throws)."""
    s = client.st(key)
    deficit = max(0, wrap32(s.global_ + s.local + p + s.qcount - client.token_limit))
    seconds = float(deficit) * client.decay_rate
    t = seconds * 1e7
    return RETRY_OVERFLOW if t >= 2.0 ** 63 else int(t)


def decide(client, wait, key, p, rid):
    """One request through the oracle: (status, available, evicted ids, ticks, changed,
    global) -- changed: the request moved the key's local score or queue count; global: the
    global score in a FAILED request's deficit."""
    s = client.st(key)
    before = (s.local, s.qcount)
    if wait:
        status, ev = client.wait(key, p, rid)
    else:
        status, ev = client.acquire(key, p), []
    avail = -1 if status == AP_REJECTED else client.available(s)
    ticks = retry_ticks(client, key, p) if status == AP_FAILED else RETRY_NONE
    return status, avail, ev, ticks, (s.local, s.qcount) != before, s.global_ if status == AP_FAILED else 0


# ----------------------------------------------------------------------------- the case list
# shape: "small"  300 keys, 4,000 requests: one pass, 16-row dense buckets, every key repeats
#                 inside a 2,048-request chunk (many owner rounds)
#        "two"    50,000 keys, 4,000 requests: two passes (fold records when packed), the reply
#                 position is not the arrival index; 70% of the requests go to 200 keys spread
#                 over the key space so that keys repeat and throttle
#        "large"  3,000,000 keys: buckets of 2,048 rows; 200,000 requests over a pool of 100,000
#                 keys (about 136 per bucket, below R/8: rows are gathered), and in the last
#                 epoch one more batch of 6,000 requests on the keys of three buckets (dense,
#                 three chunks each, keys repeating across the chunks)
# min_distinct: the common threshold is 100 distinct non-zero tick values.  With TokenLimit 20
# a case cannot reach it by construction: ticks = deficit * rate * 1e7 is one value per
# deficit, and deficit = global + local + p + qcount - 20 <= 20 * n_clients + 20 + QueueLimit
# - 20 while grants need global < 20 (every client adds at most its cap, <= 20, per epoch, and
# the tier decays).  Those cases state their own threshold: half of that bound's range that a
# run can be expected to visit -- 10 * n_clients + QueueLimit / 2 + 5.
Case = namedtuple("Case", "shape n_clients order qlimit wait pack limit epochs kw")


def case(shape, n_clients, order, qlimit, wait, pack, limit, epochs=None, **kw):
    if epochs is None:
        epochs = {"small": 4, "two": 3, "large": 2}[shape]
    return Case(shape, n_clients, order, qlimit, wait, pack, limit, epochs, tuple(sorted(kw.items())))


CASES = [
    case("small", 3, OLDEST_FIRST, 16, True, True, 20),
    case("small", 3, NEWEST_FIRST, 4, True, True, 20),
    case("small", 1, OLDEST_FIRST, 4, True, True, 20),
    case("small", 1, NEWEST_FIRST, 0, False, True, 20),
    case("small", 3, NEWEST_FIRST, 4, True, False, 20),
    case("small", 1, OLDEST_FIRST, 0, False, False, 20),
    case("small", 3, OLDEST_FIRST, 16, True, True, 16382),
    case("small", 1, NEWEST_FIRST, 4, True, True, 16383),
    case("small", 3, OLDEST_FIRST, 0, False, True, 16382),
    case("small", 1, NEWEST_FIRST, 16, False, True, 16383),
    case("small", 3, OLDEST_FIRST, 0, True, False, 16383),
    case("two", 3, NEWEST_FIRST, 4, True, True, 20),
    case("two", 1, OLDEST_FIRST, 16, True, True, 16383),
    case("two", 1, OLDEST_FIRST, 0, False, True, 20),
    case("two", 3, OLDEST_FIRST, 4, False, True, 16382),
    # two passes without fold records: an intermediate un-partition carries the deficits
    case("two", 3, NEWEST_FIRST, 4, True, False, 20),
    case("two", 1, NEWEST_FIRST, 16, True, True, 16382, fold_records=False),
    case("two", 1, OLDEST_FIRST, 4, True, True, 16383, fold_records=False),
    # the re-ranking final un-partition (TBE_FLAG_RERANK), both reply widths
    case("two", 1, NEWEST_FIRST, 4, True, True, 20, rerank=True),
    case("two", 3, OLDEST_FIRST, 0, False, True, 16383, rerank=True),
    case("large", 1, NEWEST_FIRST, 4, True, True, 20),
    # (TokenLimit 16382 over 3,000,000 keys leaves no room for packed records: SoA passes)
    case("large", 1, OLDEST_FIRST, 0, False, False, 16382),
]


def case_id(c):
    return "-".join([c.shape, f"c{c.n_clients}", "new" if c.order == NEWEST_FIRST else "old", f"q{c.qlimit}",
                     "wait" if c.wait else "try", "pack" if c.pack else "soa", f"L{c.limit}"] +
                    [k for k, v in c.kw])


def min_distinct(c):
    return 100 if c.limit > 20 else 10 * c.n_clients + c.qlimit // 2 + 5


Shape = namedtuple("Shape", "n_keys n pool hot dense")


def make_shape(c, rng):
    if c.shape == "small":
        return Shape(300, 4000, None, None, None)
    if c.shape == "two":
        return Shape(50_000, 4000, None, rng.choice(50_000, 200, replace=False), None)
    n_keys = 3_000_000
    pool = rng.choice(n_keys, 100_000, replace=False)
    buckets = rng.choice(n_keys // 2048, 3, replace=False)
    dense = (buckets[:, None] * 2048 + np.arange(2048)[None, :]).ravel()
    return Shape(n_keys, 200_000, np.union1d(pool, dense), None, dense)


def draw_keys(c, sh, rng, n):
    if sh.hot is not None:
        return np.where(rng.random(n) < 0.7, rng.choice(sh.hot, n), rng.integers(0, sh.n_keys, n)).astype(np.uint64)
    if sh.pool is not None:
        return rng.choice(sh.pool, n).astype(np.uint64)
    return rng.integers(0, sh.n_keys, n).astype(np.uint64)


def permit_choices(limit):
    # 0, TokenLimit and TokenLimit + 1 (REJECTED) in every mix
    if limit <= 100:
        return [0, 1, 1, 2, 3, 5, 8, limit, limit + 1]
    return [0, 1, 2, 3, 25, 1000, limit // 7, limit // 3, limit // 2, limit - 1, limit, limit + 1]


Batch = namedtuple("Batch", "client keys permits id_base status avail evicted ticks")
Run = namedtuple("Run", "shape epochs failed_share distinct moved_after with_global")


@functools.lru_cache(maxsize=4)
def expected_run(c):
    """The whole run of a case through the oracle, once: per epoch the batches (inputs and
    expected outputs) and the sync's (ts, stagger, expected drain logs).  Never modified."""
    rng = np.random.default_rng(1000 + CASES.index(c))
    sh = make_shape(c, rng)
    clients = [ApproxClient(c.limit, TOKENS, TICKS, c.qlimit, c.order) for _ in range(c.n_clients)]
    table = ApproxGlobalTable(clients[0].decay_rate)
    sync_keys = range(sh.n_keys) if sh.pool is None else sh.pool.tolist()
    choices = permit_choices(c.limit)
    epochs, rid = [], 0
    n_req = n_failed = moved_after = with_global = 0
    distinct = set()
    for epoch in range(c.epochs):
        batches = []
        for r in range(c.n_clients):
            todo = [draw_keys(c, sh, rng, sh.n)]
            if sh.dense is not None and epoch == c.epochs - 1:
                todo.append(rng.choice(sh.dense, 6000).astype(np.uint64))
            for keys in todo:
                n = keys.size
                permits = rng.choice(choices, n).astype(np.int32)
                out = [decide(clients[r], c.wait, k, p, rid + i)
                       for i, (k, p) in enumerate(zip(keys.tolist(), permits.tolist()))]
                status = np.array([o[0] for o in out], np.uint8)
                ticks = np.array([o[3] for o in out], np.int64)
                batches.append(Batch(r, keys, permits, rid, status, np.array([o[1] for o in out], np.int32),
                                     [(i, x) for i, o in enumerate(out) for x in o[2]], ticks))
                rid += n
                n_req += n
                n_failed += int((status == AP_FAILED).sum())
                with_global += sum(1 for o in out if o[5] != 0)
                distinct.update(ticks[(status == AP_FAILED) & (ticks > 0)].tolist())
                # FAILED requests followed, in this batch and on their key, by a request that
                # changes local or qcount: walk backwards, remembering the keys changed later
                changed_later = set()
                for (k, o) in zip(reversed(keys.tolist()), reversed(out)):
                    if o[0] == AP_FAILED and k in changed_later:
                        moved_after += 1
                    if o[4]:
                        changed_later.add(k)
        ts = S_US + epoch * 1_000_000 + int(rng.integers(0, 300_000))
        stagger = 1_000_000 // c.n_clients
        logs = approx_refresh_all(clients, table, ts, stagger, sync_keys)
        epochs.append((batches, ts, stagger, logs))
    return Run(sh, epochs, n_failed / n_req, len(distinct), moved_after, with_global)


def check_not_vacuous(c, run):
    """On the oracle's output alone, before anything is compared with the engine."""
    assert run.failed_share >= 0.15, run.failed_share
    assert run.distinct >= min_distinct(c), run.distinct
    assert run.moved_after >= 50, run.moved_after
    # after the first epoch's sync the deficits include a non-zero global score
    assert run.with_global >= 50, run.with_global


def make_engines(c, sh, n=None):
    from distributedratelimiting.redis_amd import ApproximateEngine
    engines = [ApproximateEngine(sh.n_keys, c.limit, TOKENS, TICKS, c.qlimit, c.order, device=0, pack=c.pack,
                                 **dict(c.kw)) for _ in range(n or c.n_clients)]
    lay = engines[0].layout()
    assert lay["packed"] == c.pack and lay["medium"] == (c.limit <= 16382)
    assert lay["passes"] == (1 if c.shape == "small" else 2)
    assert lay["fold_records"] == (c.pack and c.shape != "small" and dict(c.kw).get("fold_records", True))
    return engines


def sync_all(engines, counts, ts, stagger):
    import torch
    for e, cn in zip(engines, counts):
        e.collect(cn)
    allc = torch.cat(counts)
    torch.cuda.synchronize()   # the engines' sync replay reads allc on their own streams
    return [e.sync(allc, len(engines), r, ts, stagger) for r, e in enumerate(engines)]


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_retry_after_matches_oracle(engine_lib, gpu, c):
    """Status, available, evictions and retry_after_ticks of every request equal the oracle's,
    over several epochs with syncs between them (3 clients: global != 0, est > 1 and the client
    view is written; 1 client: the view is lazy and the entry point materialises it)."""
    import torch
    run = expected_run(c)
    check_not_vacuous(c, run)
    engines = make_engines(c, run.shape)
    counts = [torch.zeros(run.shape.n_keys, dtype=torch.int32, device=gpu) for _ in engines]
    torch.cuda.synchronize()
    for epoch, (batches, ts, stagger, exp_logs) in enumerate(run.epochs):
        for b in batches:
            st, av, (cause, ids), ticks = engines[b.client].acquire_batch(b.keys, b.permits, wait=c.wait,
                                                                          id_base=b.id_base, retry_after=True)
            assert ticks.dtype == np.int64
            assert np.array_equal(st, b.status), epoch
            assert np.array_equal(av, b.avail), epoch
            assert list(zip(cause.tolist(), ids.tolist())) == b.evicted, epoch
            bad = np.flatnonzero(ticks != b.ticks)
            assert bad.size == 0, (epoch, bad[:5], ticks[bad[:5]], b.ticks[bad[:5]], b.status[bad[:5]])
        logs = sync_all(engines, counts, ts, stagger)
        for (k, i, _), want in zip(logs, exp_logs):
            assert list(zip(k.tolist(), i.tolist())) == want


# (the first is the last case of the test above: its oracle run is still cached)
@pytest.mark.parametrize("c", [CASES[20], CASES[1], CASES[2], CASES[11], CASES[16], CASES[18]], ids=case_id)
def test_device_form_equals_host_form(engine_lib, gpu, c):
    """tbe_approx_acquire_batch_retry_device on a non-default stream, with no host
    synchronisation between the enqueue and the next batch, against the host form on twin
    engines (and so, by the test above, against the oracle); and the old entry points, given
    the same batches on a third set of twins, still return the same status, available and
    evictions."""
    import torch
    run = expected_run(c)
    sh = run.shape
    dev, host, old = make_engines(c, sh), make_engines(c, sh), make_engines(c, sh)
    counts = [[torch.zeros(sh.n_keys, dtype=torch.int32, device=gpu) for _ in dev] for _ in range(3)]
    side = torch.cuda.Stream(gpu)
    torch.cuda.synchronize()
    for batches, ts, stagger, exp_logs in run.epochs:
        outs = []
        for b in batches:   # enqueue only: nothing synchronises the host inside this loop
            with torch.cuda.stream(side):
                dk = torch.from_numpy(b.keys.view(np.int64)).to(gpu, non_blocking=True)
                dp = torch.from_numpy(b.permits).to(gpu, non_blocking=True)
                ds = torch.empty(b.keys.size, dtype=torch.uint8, device=gpu)
                da = torch.empty(b.keys.size, dtype=torch.int32, device=gpu)
                dt = torch.full((b.keys.size,), -7, dtype=torch.int64, device=gpu)
            dev[b.client].acquire_batch_device(dk, dp, ds, da, wait=c.wait, id_base=b.id_base,
                                               stream=side.cuda_stream, d_retry_after=dt)
            outs.append((dk, dp, ds, da, dt))
        side.synchronize()
        for b, (_, _, ds, da, dt) in zip(batches, outs):
            st, av, ev, ticks = host[b.client].acquire_batch(b.keys, b.permits, wait=c.wait, id_base=b.id_base,
                                                             retry_after=True)
            assert np.array_equal(ds.cpu().numpy(), st) and np.array_equal(st, b.status)
            assert np.array_equal(da.cpu().numpy(), av)
            assert np.array_equal(dt.cpu().numpy(), ticks) and np.array_equal(ticks, b.ticks)
            st0, av0, ev0 = old[b.client].acquire_batch(b.keys, b.permits, wait=c.wait, id_base=b.id_base)
            assert np.array_equal(st0, st) and np.array_equal(av0, av)
            assert np.array_equal(ev0[0], ev[0]) and np.array_equal(ev0[1], ev[1])
        for engs, cs in zip((dev, host, old), counts):
            logs = sync_all(engs, cs, ts, stagger)
            for (k, i, _), want in zip(logs, exp_logs):
                assert list(zip(k.tolist(), i.tolist())) == want


def test_chunked_host_path_equals_device_form(engine_lib, gpu):
    """Page-locked buffers of 2^22 + 5,000 requests over 50,000 keys take status_chunked
    (chunks of 2^22): status, available and ticks equal the same batch through the device
    form on a twin engine.  An equality of two engine paths (the oracle comparison is the
    tests above); one sync first, so the deficits carry a global score."""
    import torch
    from distributedratelimiting.redis_amd import ApproximateEngine
    from distributedratelimiting.redis_amd.engine import PinnedArray
    n_keys, n = 50_000, (1 << 22) + 5000
    rng = np.random.default_rng(77)
    a, b = (ApproximateEngine(n_keys, 20, TOKENS, TICKS, 4, NEWEST_FIRST, device=0) for _ in range(2))
    bufs = [PinnedArray(n, d) for d in (np.uint64, np.int32, np.uint8, np.int32, np.int64)]
    keys, permits, st, av, ticks = (x.array for x in bufs)
    counts = torch.zeros(n_keys, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    for epoch in range(2):
        keys[:] = rng.integers(0, n_keys, n)
        permits[:] = rng.choice([0, 1, 2, 3, 5, 20, 21], n)
        ticks[:] = -7
        _, _, (cause, ids), _ = a.acquire_batch(keys, permits, wait=True, id_base=epoch * n, status=st,
                                                available=av, retry_after=ticks)
        dk = torch.from_numpy(keys.view(np.int64).copy()).to(gpu)
        dp = torch.from_numpy(permits.copy()).to(gpu)
        ds = torch.empty(n, dtype=torch.uint8, device=gpu)
        da = torch.empty(n, dtype=torch.int32, device=gpu)
        dt = torch.empty(n, dtype=torch.int64, device=gpu)
        torch.cuda.synchronize()
        b.acquire_batch_device(dk, dp, ds, da, wait=True, id_base=epoch * n, d_retry_after=dt)
        b.synchronize()
        assert np.array_equal(ds.cpu().numpy(), st)
        assert np.array_equal(da.cpu().numpy(), av)
        assert np.array_equal(dt.cpu().numpy(), ticks)
        failed = st == AP_FAILED
        assert failed.mean() > 0.15 and (ticks[failed] >= 0).all() and (ticks[~failed] == RETRY_NONE).all()
        # not vacuous: on a throttled key the mix's five non-zero permit counts that can fail
        # (1, 2, 3, 5, 20) have five different deficits
        assert np.unique(ticks[failed]).size >= 5
        for e in (a, b):
            e.collect(counts)
            e.sync(counts, 1, 0, S_US + epoch * 1_000_000, 0)
    for x in bufs:
        x.free()


# ----------------------------------------------------------------------------- crafted cases
RATE = TOKENS / (TICKS / 1e7)          # 10 tokens per second
T1 = int(1.0 * RATE * 1e7)             # ticks of a deficit of 1


def one_batch(eng, reqs, wait, id_base=0):
    keys = np.array([k for k, _ in reqs], np.uint64)
    ps = np.array([p for _, p in reqs], np.int32)
    st, av, ev, ticks = eng.acquire_batch(keys, ps, wait=wait, id_base=id_base, retry_after=True)
    return st.tolist(), av.tolist(), list(zip(ev[0].tolist(), ev[1].tolist())), ticks.tolist()


def oracle_batch(cli, reqs, wait, id_base=0):
    out = [decide(cli, wait, k, p, id_base + i) for i, (k, p) in enumerate(reqs)]
    return ([o[0] for o in out], [o[1] for o in out], [(i, x) for i, o in enumerate(out) for x in o[2]],
            [o[3] for o in out])


def test_state_moves_after_the_failure(engine_lib, gpu):
    """On one key in one batch: p = 5 fails at AvailableTokens 3, then p = 3 is granted.  The
    first request's ticks use `local` before the grant (the host's per-key query after the
    batch saw local 20 and answered 5 * T1 instead of 2 * T1)."""
    from distributedratelimiting.redis_amd import ApproximateEngine
    eng = ApproximateEngine(8, 20, TOKENS, TICKS, 0, OLDEST_FIRST, device=0)
    reqs = [(3, 17), (3, 5), (3, 3), (3, 1)]
    st, av, ev, ticks = one_batch(eng, reqs, wait=False)
    assert st == [1, 0, 1, 0] and av == [3, 3, 0, 0]
    # local 17: 17 + 5 - 20 = 2; after the grant local 20: 20 + 1 - 20 = 1
    assert ticks == [RETRY_NONE, 2 * T1, RETRY_NONE, 1 * T1]
    assert (st, av, ev, ticks) == oracle_batch(ApproxClient(20, TOKENS, TICKS, 0, OLDEST_FIRST), reqs, False)


def test_wait_queues_after_the_failure(engine_lib, gpu):
    """OldestFirst, QueueLimit 4: p = 5 cannot queue (FAILED, qcount 0), then p = 4 queues.
    The failure's ticks carry qcount 0, not the 4 queued after it."""
    from distributedratelimiting.redis_amd import ApproximateEngine
    eng = ApproximateEngine(8, 20, TOKENS, TICKS, 4, OLDEST_FIRST, device=0)
    reqs = [(5, 18), (5, 5), (5, 4), (5, 1)]
    st, av, ev, ticks = one_batch(eng, reqs, wait=True)
    assert st == [1, 0, 2, 0]
    # 18 + 5 + 0 - 20 = 3; then qcount 4: 18 + 1 + 4 - 20 = 3 (p = 1 fails behind the queue, A:202)
    assert ticks == [RETRY_NONE, 3 * T1, RETRY_NONE, 3 * T1]
    assert (st, av, ev, ticks) == oracle_batch(ApproxClient(20, TOKENS, TICKS, 4, OLDEST_FIRST), reqs, True)


def test_eviction_after_the_failure(engine_lib, gpu):
    """NewestFirst, QueueLimit 4: two waits fill the queue (qcount 4), p = 5 > QueueLimit fails
    with qcount 4 in its deficit, then p = 3 evicts both (qcount 3)."""
    from distributedratelimiting.redis_amd import ApproximateEngine
    eng = ApproximateEngine(8, 20, TOKENS, TICKS, 4, NEWEST_FIRST, device=0)
    reqs = [(2, 19), (2, 2), (2, 2), (2, 5), (2, 3), (2, 5)]
    st, av, ev, ticks = one_batch(eng, reqs, wait=True, id_base=10)
    assert st == [1, 2, 2, 0, 2, 0] and ev == [(4, 11), (4, 12)]
    # 19 + 5 + 4 - 20 = 8; after the eviction qcount 3: 19 + 5 + 3 - 20 = 7
    assert ticks == [RETRY_NONE, RETRY_NONE, RETRY_NONE, 8 * T1, RETRY_NONE, 7 * T1]
    assert (st, av, ev, ticks) == oracle_batch(ApproxClient(20, TOKENS, TICKS, 4, NEWEST_FIRST), reqs, True, 10)


def test_deficit_zero_is_zero_ticks(engine_lib, gpu):
    """OldestFirst with a non-empty queue: an AcquireCore that the tokens would cover fails
    because of the queue (A:202).  TokenLimit 10, QueueLimit 4: p = 8 is granted, a wait of 3
    queues behind AvailableTokens 2; the collect of a refresh (A:430-435) then takes the local
    score, so 10 tokens are available with 3 still queued.  p = 2 and p = 7 fail with deficits
    0 + 2 + 3 - 10 < 0 and 0 + 7 + 3 - 10 = 0: 0 ticks, not TBE_RETRY_NONE; p = 8 with 1."""
    import torch
    from distributedratelimiting.redis_amd import ApproximateEngine
    eng = ApproximateEngine(8, 10, TOKENS, TICKS, 4, OLDEST_FIRST, device=0)
    cli = ApproxClient(10, TOKENS, TICKS, 4, OLDEST_FIRST)
    w = [(5, 8), (5, 3)]
    st, av, ev, ticks = one_batch(eng, w, wait=True)
    assert st == [1, 2] and (st, av, ev, ticks) == oracle_batch(cli, w, True)
    counts = torch.zeros(8, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    eng.collect(counts)
    cli.collect()
    a = [(5, 2), (5, 7), (5, 8)]
    st, av, ev, ticks = one_batch(eng, a, wait=False)
    assert (st, av, ev, ticks) == oracle_batch(cli, a, False)
    assert st == [0, 0, 0] and av == [10, 10, 10] and ticks == [0, 0, 1 * T1]


def test_zero_permit_failures(engine_lib, gpu):
    """A zero-permit AcquireCore on a throttled key (A:99-102) and a zero-permit wait beyond
    zero_wait_slots (this engine's own departure): the formula with p = 0."""
    from distributedratelimiting.redis_amd import ApproximateEngine
    eng = ApproximateEngine(4, 2, 2, TICKS, 2, OLDEST_FIRST, device=0, zero_wait_slots=2)
    cli = ApproxClient(2, 2, TICKS, 2, OLDEST_FIRST, zero_slots=2)
    t1 = int(1.0 * cli.decay_rate * 1e7)
    a = [(1, 2), (1, 0), (1, 1)]
    st, av, ev, ticks = one_batch(eng, a, wait=False)
    assert (st, av, ev, ticks) == oracle_batch(cli, a, False)
    assert st == [1, 0, 0] and ticks == [RETRY_NONE, 0, 1 * t1]       # 2 + 0 - 2 = 0; 2 + 1 - 2 = 1
    w = [(1, 0), (1, 0), (1, 2), (1, 0), (1, 1)]
    st, av, ev, ticks = one_batch(eng, w, wait=True, id_base=100)
    assert (st, av, ev, ticks) == oracle_batch(cli, w, True, 100)
    # two zero waits queue, p = 2 queues (qcount 2), the third zero wait finds no slot:
    # 2 + 0 + 2 - 2 = 2; p = 1 does not fit the queue: 2 + 1 + 2 - 2 = 3
    assert st == [2, 2, 2, 0, 0] and ticks == [RETRY_NONE, RETRY_NONE, RETRY_NONE, 2 * t1, 3 * t1]


def test_overflow(engine_lib, gpu):
    """replenishment_period_ticks = 1 and tokens_per_period = 2^31 - 1: the fill rate is
    2.1e16 per second, so a deficit of 1 is 2.1e23 ticks: TBE_RETRY_OVERFLOW where
    TimeSpan.FromSeconds throws; a deficit of 0 is still 0 ticks."""
    from distributedratelimiting.redis_amd import ApproximateEngine
    eng = ApproximateEngine(4, 5, 2 ** 31 - 1, 1, 0, OLDEST_FIRST, device=0)
    cli = ApproxClient(5, 2 ** 31 - 1, 1, 0, OLDEST_FIRST)
    a = [(0, 5), (0, 0), (0, 1), (0, 5), (1, 6)]
    st, av, ev, ticks = one_batch(eng, a, wait=False)
    assert (st, av, ev, ticks) == oracle_batch(cli, a, False)
    assert st == [1, 0, 0, 0, 3]
    assert ticks == [RETRY_NONE, 0, RETRY_OVERFLOW, RETRY_OVERFLOW, RETRY_NONE]


def test_null_retry_buffer_is_einval(engine_lib, gpu):
    """A null retry_after_ticks with n > 0 is TBE_EINVAL and applies nothing."""
    from distributedratelimiting.redis_amd import ApproximateEngine, _capi
    import ctypes
    eng = ApproximateEngine(4, 5, TOKENS, TICKS, 0, OLDEST_FIRST, device=0)
    keys, ps = np.zeros(3, np.uint64), np.full(3, 2, np.int32)
    st, av = np.empty(3, np.uint8), np.empty(3, np.int32)
    nev = ctypes.c_uint64()
    lib = _capi.load()
    rc = lib.tbe_approx_acquire_batch_retry(eng.handle, keys.ctypes.data, ps.ctypes.data, 3, 0, 0, st.ctypes.data,
                                            av.ctypes.data, None, ctypes.byref(nev))
    assert rc == _capi.TBE_EINVAL
    rc = lib.tbe_approx_acquire_batch_retry_device(eng.handle, keys.ctypes.data, ps.ctypes.data, 3, 0, 0,
                                                   st.ctypes.data, av.ctypes.data, None, None)
    assert rc == _capi.TBE_EINVAL
    assert eng.local_state(0)[0] == 0          # nothing applied
    assert one_batch(eng, [(0, 2), (0, 2), (0, 2)], wait=False)[0] == [1, 1, 0]
