"""tbe_migrate_out_device / tbe_migrate_out (include/tbe.h) against cluster.plan_migration:
rows, counts and flags identical, and the table after the call identical.

Sizes.  The kernels work on the export's tiles of 2,048 ids (256 lanes x 8): the counts lie
around a wave (64) and around a tile, and 3 * 2048 + 5 spans four tiles.  Tables are
populated through import_state with random v bit patterns, never through decisions.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ABSENT = np.iinfo(np.int64).min
NO = np.uint64(0xFFFFFFFFFFFFFFFF)
TS = 1_760_000_100_000_123
TILE = 2_048
COUNTS = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
OWNERS = [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (8, 0), (8, 4), (8, 7), (256, 0), (256, 128), (256, 255)]
MAPS = ["stay", "leave", "B", None]
MIXES = ["all", "none", "alternate", "unheld", "lapse"]
FIRST = 3                                   # the range starts at id 3 of a larger table
OPTS = (5, 2, 10_000_000)                   # TTL ceil(2.5) s
EXTRA = [(9, 1, 10_000_000), (100, 50, 10_000_000)]   # TTLs 9 s and 2 s
SENT = -0x0123456789ABCDEF                  # what the row buffer holds before a call


def _ttl(classes):
    from distributedratelimiting.redis_amd import cluster
    return np.array([cluster.class_ttl_ms(*c) for c in classes], dtype=np.int64)


def _stream(gpu):
    import torch
    return torch.cuda.stream(torch.cuda.Stream(gpu))


def _owner_map(kind, n, me):
    if kind is None:
        return None
    if kind == "stay":
        return np.full(4096, me, dtype=np.uint8)
    if kind == "leave":
        return np.full(4096, (me + 1) % n, dtype=np.uint8)
    m = (np.arange(4096, dtype=np.int64) * n) >> 12        # map B: odd virtual nodes to the next owner
    m[1::2] = (m[1::2] + 1) % n
    return m.astype(np.uint8)


def _table(count, mix, seed=0):
    """(key_of_id, v, t_us) of `count` ids.  v: random finite bit patterns."""
    rng = np.random.default_rng(1234 + count + seed)
    keys = rng.integers(0, 1 << 63, count, dtype=np.int64).astype(np.uint64)
    v = rng.integers(0, 0x7FE0 << 48, count, dtype=np.int64).view(np.float64).copy()
    t = TS - rng.integers(0, 2_000_000, count)             # every row live at TS (TTL >= 2 s, see "lapse")
    if mix == "none":
        t[:] = ABSENT
    elif mix == "alternate":
        t[1::2] = ABSENT
    elif mix == "unheld":                                  # unheld ids interleaved, their rows absent
        gone = rng.random(count) < 0.4
        keys[gone] = NO
        t[gone] = ABSENT
        t[rng.random(count) < 0.2] = ABSENT
    elif mix == "lapse":                                   # last grant 6 s before TS: lapsed for every class
        t[:] = TS - 6_000_000 - rng.integers(0, 1_000_000, count)
    return keys, v, t.astype(np.int64)


def _call(eng, gpu, ts, kof, omap, n, me, capacity, commit=False, first=0, pad=4):
    """One device call; returns (row buffer [capacity + pad, 4], counts, leaving)."""
    import torch
    cur = torch.cuda.current_stream(gpu).cuda_stream
    d_k = torch.from_numpy(kof.view(np.int64).copy()).to(gpu)
    d_m = None if omap is None else torch.from_numpy(omap.copy()).to(gpu)
    d_rows = torch.full((capacity + pad, 4), SENT, dtype=torch.int64, device=gpu)
    d_counts = torch.full((n + 2,), -1, dtype=torch.int64, device=gpu)
    d_leave = torch.full((kof.shape[0],), 7, dtype=torch.uint8, device=gpu)
    eng.migrate_out_device(ts, d_k, d_m, n, me, d_rows if capacity else None, d_counts, d_leave, commit=commit,
                           first=first, capacity=capacity, stream=cur)
    torch.cuda.synchronize()
    return d_rows.cpu().numpy(), d_counts.cpu().numpy(), d_leave.cpu().numpy()


def _want(kof, v, t, cls, ts, ttl, omap, n, me):
    from distributedratelimiting.redis_amd import cluster
    cls = np.zeros(kof.shape[0], dtype=np.uint8) if cls is None else cls
    return cluster.plan_migration(kof, v, t, cls, cluster.rows_live(t, ts, ttl[cls]), omap, n, me)


def _same_table(eng, v, t):
    v1, t1 = eng.export_state()
    assert np.array_equal(t1, t) and np.array_equal(v1.view(np.int64), v.view(np.int64))


@pytest.mark.parametrize("count", COUNTS)
def test_rows_counts_and_flags_against_the_plan(engine_lib, gpu, count):
    """Every owner count and position, every map and every row mix, read-only, over a range
    that does not start at id 0."""
    from distributedratelimiting.redis_amd import TokenBucketEngine
    ttl = _ttl([OPTS])
    with _stream(gpu):
        eng = TokenBucketEngine(FIRST + count + 2, *OPTS, device=0)
        sent_any = False
        for mix in MIXES:
            kof, v, t = _table(count, mix)
            eng.import_state(v, t, first=FIRST)
            v0, t0 = eng.export_state()
            for n, me in OWNERS:
                for kind in MAPS:
                    omap = _owner_map(kind, n, me)
                    for ts in ((TS, -1) if mix == "lapse" else (TS,)):
                        rows, counts, leaving = _want(kof, v, t, None, ts, ttl, omap, n, me)
                        got = _call(eng, gpu, ts, kof, omap, n, me, count, first=FIRST)
                        m = rows.shape[0]
                        assert np.array_equal(got[1], counts), (mix, n, me, kind, ts)
                        assert np.array_equal(got[2], leaving), (mix, n, me, kind, ts)
                        assert np.array_equal(got[0][:m], rows), (mix, n, me, kind, ts)
                        assert np.all(got[0][m:] == SENT)
                        if kind == "stay" or n == 1:
                            assert m == 0 and not leaving.any()
                        if kind == "leave" and n > 1 and mix == "all":
                            assert m == count and leaving.all()
                        if mix == "lapse" and kind == "leave" and n > 1:
                            assert m == (count if ts < 0 else 0) and leaving.all()
                        sent_any |= m > 0
            _same_table(eng, v0, t0)                       # commit == 0 reads only
        assert sent_any
        eng.synchronize()                                  # no call was refused
        eng.close()


@pytest.mark.parametrize("count", [65, TILE + 1, 3 * TILE + 5])
def test_capacity_zero_counts_and_short_capacity_stops_at_it(engine_lib, gpu, count):
    from distributedratelimiting.redis_amd import TokenBucketEngine
    ttl = _ttl([OPTS])
    kof, v, t = _table(count, "all")
    n, me = 3, 1
    omap = _owner_map("B", n, me)
    rows, counts, leaving = _want(kof, v, t, None, TS, ttl, omap, n, me)
    total = rows.shape[0]
    assert total > 8
    with _stream(gpu):
        eng = TokenBucketEngine(count, *OPTS, device=0)
        eng.import_state(v, t)
        got = _call(eng, gpu, TS, kof, omap, n, me, 0)
        assert np.array_equal(got[1], counts) and np.array_equal(got[2], leaving) and np.all(got[0] == SENT)
        got = _call(eng, gpu, TS, kof, omap, n, me, total - 1)
        assert np.array_equal(got[1], counts)              # counts are complete whatever the capacity
        assert np.array_equal(got[0][:total - 1], rows[:total - 1])
        assert np.all(got[0][total - 1:] == SENT)          # nothing at or past capacity
        _same_table(eng, v, t)
        eng.synchronize()
        eng.close()


@pytest.mark.parametrize("count", [64, TILE + 1, 3 * TILE + 5])
@pytest.mark.parametrize("mix", ["all", "unheld", "lapse"])
def test_commit_clears_leaving_rows_only(engine_lib, gpu, count, mix):
    from distributedratelimiting.redis_amd import TokenBucketEngine
    ttl = _ttl([OPTS])
    kof, v, t = _table(count, mix)
    n, me = 8, 4
    omap = _owner_map("B", n, me)
    rows, counts, leaving = _want(kof, v, t, None, TS, ttl, omap, n, me)
    assert 0 < leaving.sum() < (kof != NO).sum()
    with _stream(gpu):
        eng = TokenBucketEngine(FIRST + count, *OPTS, device=0)
        eng.import_state(v, t, first=FIRST)
        v0, t0 = eng.export_state()
        got = _call(eng, gpu, TS, kof, omap, n, me, rows.shape[0], commit=True, first=FIRST)
        eng.synchronize()
        assert np.array_equal(got[0][:rows.shape[0]], rows) and np.array_equal(got[1], counts)
        assert np.array_equal(got[2], leaving)
        gone = FIRST + np.flatnonzero(leaving)
        v0[gone], t0[gone] = float(OPTS[0]), ABSENT        # leaving rows absent, every other row untouched
        _same_table(eng, v0, t0)
        eng.close()


def test_refused_commits_change_nothing(engine_lib, gpu):
    """Too small a capacity, one orphan row, a map entry >= n_owners: table and counters as
    before, the sticky error at synchronize.  Argument and state checks, nothing faults."""
    from distributedratelimiting.redis_amd import TbeError, TokenBucketEngine, _capi
    count, n, me = TILE + 77, 2, 0
    ttl = _ttl([OPTS])
    kof, v, t = _table(count, "all")
    omap = _owner_map("B", n, me)
    rows, counts, leaving = _want(kof, v, t, None, TS, ttl, omap, n, me)
    rng = np.random.default_rng(9)
    ok, failed = rng.integers(0, 50, count).astype(np.uint64), rng.integers(0, 50, count).astype(np.uint64)
    with _stream(gpu):
        eng = TokenBucketEngine(count, *OPTS, device=0, stats=True)
        eng.import_state(v, t)
        eng.stats_import(ok, failed)
        totals = eng.stats_totals()

        def unchanged():
            _same_table(eng, v, t)
            o, f = eng.stats_export()
            assert np.array_equal(o, ok) and np.array_equal(f, failed) and eng.stats_totals() == totals

        got = _call(eng, gpu, TS, kof, omap, n, me, rows.shape[0] - 1, commit=True)
        assert np.array_equal(got[1], counts)
        with pytest.raises(TbeError) as ex:
            eng.synchronize()
        assert ex.value.status == _capi.TBE_EINVAL
        unchanged()
        eng.synchronize()                                  # the flag was read and cleared
        orphan = kof.copy()
        orphan[np.flatnonzero(leaving == 0)[5]] = NO       # a live row whose id no key holds
        got = _call(eng, gpu, TS, orphan, omap, n, me, rows.shape[0], commit=True)
        assert got[1][n + 1] == 1 and got[1][n] == counts[n]
        with pytest.raises(TbeError):
            eng.synchronize()
        unchanged()
        bad = omap.copy()
        bad[::7] = 2
        got = _call(eng, gpu, TS, kof, bad, n, me, count, commit=False)
        assert np.all(got[0] == SENT)
        with pytest.raises(TbeError):
            eng.synchronize()
        unchanged()
        with pytest.raises(TbeError):                      # the host form returns the refusal itself
            eng.migrate_out(TS, kof, omap, n, me, commit=True, capacity=rows.shape[0] - 1)
        with pytest.raises(TbeError):
            eng.migrate_out(TS, orphan, omap, n, me, commit=True)
        with pytest.raises(TbeError):
            eng.migrate_out(TS, kof, bad, n, me)
        eng.synchronize()                                  # ... and leaves the sticky flag alone
        unchanged()
        eng.close()


def test_bad_arguments_and_other_kinds(engine_lib, gpu):
    import torch
    from distributedratelimiting.redis_amd import (ApproximateEngine, QueueingTokenBucketEngine, TbeError,
                                                   TokenBucketEngine, _capi)
    kof = np.arange(100, dtype=np.uint64)
    with _stream(gpu):
        eng = TokenBucketEngine(100, *OPTS, device=0)
        for n, me in [(0, 0), (257, 0), (2, 2), (8, 8)]:
            with pytest.raises(TbeError) as ex:
                _call(eng, gpu, TS, kof, None, n, me, 100)
            assert ex.value.status == _capi.TBE_EINVAL
        with pytest.raises(TbeError):                      # a range past n_keys
            _call(eng, gpu, TS, kof, None, 2, 0, 100, first=1)
        lib, cur = _capi.load(), torch.cuda.current_stream(gpu).cuda_stream
        d = torch.zeros(128, dtype=torch.int64, device=gpu)
        assert lib.tbe_migrate_out_device(eng.handle, TS, 0, 100, None, None, 2, 0, None, 0, d.data_ptr(), None, 0,
                                          cur) == _capi.TBE_EINVAL
        assert lib.tbe_migrate_out_device(eng.handle, TS, 0, 100, d.data_ptr(), None, 2, 0, None, 0, None, None, 0,
                                          cur) == _capi.TBE_EINVAL
        eng.synchronize()
        eng.close()
        for other in (QueueingTokenBucketEngine(100, 5, 2, 10_000_000, 4, device=0),
                      ApproximateEngine(100, 5, 2, 10_000_000, 4, device=0)):
            with pytest.raises(TbeError) as ex:
                _call(other, gpu, TS, kof, None, 2, 0, 100)
            assert ex.value.status == _capi.TBE_EINVAL
            with pytest.raises(TbeError):
                other.migrate_out(TS, kof, None, 2, 0)
            other.close()


@pytest.mark.parametrize("count", [65, 3 * TILE + 5])
def test_classed_engine(engine_lib, gpu, count):
    """Three classes with different TokenLimits and TTLs (3 s, 9 s, 2 s): the class column,
    the lapse by each key's own class, and a cleared id's `available`."""
    from distributedratelimiting.redis_amd import TokenBucketEngine
    classes = [OPTS] + EXTRA
    ttl = _ttl(classes)
    assert ttl.tolist() == [3000, 9000, 2000]
    kof, v, t = _table(count, "all", seed=5)
    rng = np.random.default_rng(count)
    t = (TS - rng.integers(0, 10_000_000, count)).astype(np.int64)     # ages up to 10 s: some lapse in every class
    cls = rng.integers(0, 3, count).astype(np.uint8)
    n, me = 3, 2
    omap = _owner_map("B", n, me)
    with _stream(gpu):
        eng = TokenBucketEngine(count, *OPTS, device=0, classes=EXTRA)
        eng.set_class(np.arange(count, dtype=np.uint64), cls)
        eng.import_state(v, t)
        v0, t0 = eng.export_state()
        for ts in (TS, -1):
            rows, counts, leaving = _want(kof, v, t, cls, ts, ttl, omap, n, me)
            got = _call(eng, gpu, ts, kof, omap, n, me, count)
            assert np.array_equal(got[0][:rows.shape[0]], rows) and np.array_equal(got[1], counts)
            assert np.array_equal(got[2], leaving)
        rows, counts, leaving = _want(kof, v, t, cls, TS, ttl, omap, n, me)
        if count > 1000:                                   # rows of every class travel, and lapsed ones of every class do not
            assert set(rows[:, 3].tolist()) == {0, 1, 2}
            from distributedratelimiting.redis_amd import cluster
            dead = ~cluster.rows_live(t, TS, ttl[cls]) & (leaving == 1)
            assert set(cls[dead].tolist()) == {0, 1, 2}
        got = _call(eng, gpu, TS, kof, omap, n, me, rows.shape[0], commit=True)
        eng.synchronize()
        assert np.array_equal(got[0][:rows.shape[0]], rows)
        gone = np.flatnonzero(leaving)
        limits = np.array([c[0] for c in classes])
        v0[gone], t0[gone] = limits[cls[gone]].astype(np.float64), ABSENT
        _same_table(eng, v0, t0)
        assert np.array_equal(eng.get_class(np.arange(count, dtype=np.uint64)), cls)     # class bytes stay
        avail = eng.statistics(gone.astype(np.uint64), TS)[2]
        assert np.array_equal(avail, limits[cls[gone]])
        eng.close()


def test_stats_engine_zeroes_leaving_counters(engine_lib, gpu):
    from distributedratelimiting.redis_amd import TokenBucketEngine
    count, n, me = TILE + 300, 2, 1
    ttl = _ttl([OPTS])
    kof, v, t = _table(count, "alternate")
    omap = _owner_map("B", n, me)
    rows, counts, leaving = _want(kof, v, t, None, TS, ttl, omap, n, me)
    rng = np.random.default_rng(21)
    ok, failed = rng.integers(1, 90, count).astype(np.uint64), rng.integers(1, 90, count).astype(np.uint64)
    with _stream(gpu):
        eng = TokenBucketEngine(count, *OPTS, device=0, stats=True)
        eng.import_state(v, t)
        eng.stats_import(ok, failed)
        totals = eng.stats_totals()
        got = _call(eng, gpu, TS, kof, omap, n, me, rows.shape[0], commit=True)
        eng.synchronize()
        assert np.array_equal(got[0][:rows.shape[0]], rows)
        o, f = eng.stats_export()
        gone = leaving == 1
        assert 0 < gone.sum() < count
        assert not o[gone].any() and not f[gone].any()                 # absent leaving rows' counters too
        assert np.array_equal(o[~gone], ok[~gone]) and np.array_equal(f[~gone], failed[~gone])
        assert eng.stats_totals() == totals
        eng.close()


def test_host_form_gives_the_same(engine_lib, gpu):
    from distributedratelimiting.redis_amd import TokenBucketEngine
    count, n, me = 3 * TILE + 5, 8, 0
    ttl = _ttl([OPTS])
    kof, v, t = _table(count, "unheld")
    with _stream(gpu):
        eng = TokenBucketEngine(FIRST + count, *OPTS, device=0)
        eng.import_state(v, t, first=FIRST)
        v0, t0 = eng.export_state()
        for kind in ("B", None):
            omap = _owner_map(kind, n, me)
            rows, counts, leaving = _want(kof, v, t, None, TS, ttl, omap, n, me)
            got = eng.migrate_out(TS, kof, omap, n, me, first=FIRST)
            assert np.array_equal(got[0][:rows.shape[0]], rows) and not got[0][rows.shape[0]:].any()
            assert np.array_equal(got[1].astype(np.int64), counts) and np.array_equal(got[2], leaving)
            got = eng.migrate_out(TS, kof, omap, n, me, first=FIRST, capacity=0)
            assert np.array_equal(got[1].astype(np.int64), counts) and np.array_equal(got[2], leaving)
        _same_table(eng, v0, t0)
        got = eng.migrate_out(TS, kof, omap, n, me, first=FIRST, commit=True)
        assert np.array_equal(got[0][:rows.shape[0]], rows)
        gone = FIRST + np.flatnonzero(leaving)
        v0[gone], t0[gone] = float(OPTS[0]), ABSENT
        _same_table(eng, v0, t0)
        eng.close()
