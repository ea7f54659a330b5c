"""tbe_export_live_device / tbe_import_rows_device (include/tbe.h): the live rows of a
table against the numpy statement of the rule (snapshot.live_rows) on export_state, ids
equal and v equal bit for bit; and rows put back by id.

Sizes.  The export works on tiles of 2,048 rows (256 lanes x 8), and one round of its scan
kernel covers 1,024 tile counts, i.e. 2,097,152 rows: 5,000 rows are no multiple of 256 or
2,048, and 3,000,000 rows are 1,465 tiles, more than one scan round covers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ABSENT = np.iinfo(np.int64).min
TS = 1_760_000_100_000_123          # the snapshot's timestamp (us)
TTL_MS = 3_000                      # limit 5 at 2 tokens per second: ceil(2.5) s
TILE, SCAN_ROUND = 2_048, 1_024 * 2_048
SIZES = [5_000, 3_000_000]
assert 3_000_000 // TILE + 1 > 1_024 and SIZES[0] % 256 and SIZES[0] % TILE


def _stream(gpu):
    import torch
    return torch.cuda.stream(torch.cuda.Stream(gpu))


def _table(n, mix, seed=17):
    """(v, t_us, crafted ids) of an n-row table: 'some' about 30% live with the crafted
    rows below, 'none' no live row (absent or lapsed), 'all' every row live."""
    rng = np.random.default_rng(seed + n % 1000)
    v = rng.uniform(0.0, 5.0, n)
    ms = TS // 1000
    if mix == "all":
        return v, TS - rng.integers(0, 2_900_000, n), np.zeros(0, dtype=np.int64)
    lapsed = (ms - TTL_MS) * 1000 - 1 - rng.integers(0, 3_000_000, n)
    if mix == "none":
        lapsed[rng.random(n) < 0.4] = ABSENT
        return v, lapsed, np.zeros(0, dtype=np.int64)
    t = np.where(rng.random(n) < 0.3, TS - rng.integers(0, 2_900_000, n), lapsed)
    t[rng.random(n) < 0.2] = ABSENT
    crafted = []
    # live runs across a 256-row block, a tile and (large table) a scan-round boundary,
    # with absent rows on either side
    for edge in [256, TILE, 2 * TILE, SCAN_ROUND]:
        if edge + 40 < n:
            t[edge - 40:edge + 40] = ABSENT
            t[edge - 6:edge + 9] = TS - np.arange(15)
            crafted += list(range(edge - 40, edge + 40))
    absent, on_edge, past_edge, future = 10, 11, 12, 13
    t[absent] = ABSENT
    t[on_edge] = (ms - TTL_MS) * 1000 + 7             # ts // 1000 == t // 1000 + ttl: live
    t[past_edge] = (ms - TTL_MS - 1) * 1000 + 999     # one millisecond earlier: lapsed
    t[future] = TS + 5_000_000                        # t_us > ts_us: live
    t[n - 1] = TS - 1                                 # the last row of the table is live
    crafted += [absent, on_edge, past_edge, future, n - 1]
    return v, t, np.array(crafted, dtype=np.int64)


def _export(eng, ts_us, first=0, count=None, stream=None):
    ids, v, t = eng.export_live(ts_us, first=first, count=count, stream=stream)
    import torch
    torch.cuda.synchronize()
    return ids.cpu().numpy(), v.cpu().numpy(), t.cpu().numpy()


def _check_rows(got, v_tab, t_tab, ts_us, first=0, count=None):
    """got = (ids, v, t) against the rule on rows [first, first + count) of the table."""
    count = t_tab.shape[0] - first if count is None else count
    from distributedratelimiting.redis_amd import snapshot
    want = snapshot.live_rows(v_tab[first:first + count], t_tab[first:first + count], ts_us, TTL_MS) + first
    ids, v, t = got
    print("live", want.shape[0], "of", count, "exported", ids.shape[0])
    assert np.array_equal(ids, want)
    assert np.array_equal(v.view(np.uint64), v_tab[want].view(np.uint64))
    assert np.array_equal(t, t_tab[want])
    return want


@pytest.mark.parametrize("mix", ["some", "none", "all"])
@pytest.mark.parametrize("n", SIZES)
def test_export_against_the_rule(engine_lib, gpu, n, mix):
    import torch
    from distributedratelimiting.redis_amd import TokenBucketEngine
    v, t, crafted = _table(n, mix)
    rng = np.random.default_rng(3)
    with _stream(gpu):
        cur = torch.cuda.current_stream(gpu).cuda_stream
        eng = TokenBucketEngine(n, 5, 2, 10_000_000, device=0)
        eng.import_state(v, t)
        if mix != "none":
            # a random batch, enqueued and not waited for: the export must see its writes
            m = 3_000
            k = rng.integers(0, n, m).astype(np.uint64)
            k[np.isin(k, crafted)] = 100
            p = rng.integers(0, 4, m).astype(np.int32)
            bt = np.sort(TS - 500_000 + rng.integers(0, 400_000, m)).astype(np.int64)
            g = torch.empty(m, dtype=torch.uint8, device=gpu)
            r = torch.empty(m, dtype=torch.int32, device=gpu)
            eng.acquire_batch_device(torch.from_numpy(k.view(np.int64)).to(gpu), torch.from_numpy(p).to(gpu),
                                     torch.from_numpy(bt).to(gpu), g, r, stream=cur)
        got = _export(eng, TS, stream=cur)
        v1, t1 = eng.export_state()
        want = _check_rows(got, v1, t1, TS)
        if mix == "none":
            assert want.shape[0] == 0
        elif mix == "all":
            assert want.shape[0] == n
        else:
            from distributedratelimiting.redis_amd import snapshot
            assert 0.2 * n < snapshot.live_rows(v, t, TS, TTL_MS).shape[0] < 0.4 * n      # before the batch
            assert want.shape[0] < n
            changed = np.flatnonzero(t1 != t)
            assert changed.shape[0] > 0 and np.isin(changed, want).all()      # the batch's grants are in
            assert np.array_equal(t1[crafted], t[crafted])                    # untouched by the batch
            live = np.isin([10, 11, 12, 13, n - 1], want).tolist()
            assert live == [False, True, False, True, True]
            for key in (10, 11, 12, 13):                                     # the rule tbe_query applies
                assert (eng.query(key, TS) is not None) == bool(np.isin(key, want)), key
        eng.close()


@pytest.fixture(scope="module")
def small(engine_lib, gpu):
    """One 5,000-row engine with the 'some' table, left unchanged by the tests that share it."""
    from distributedratelimiting.redis_amd import TokenBucketEngine
    v, t, _ = _table(SIZES[0], "some")
    eng = TokenBucketEngine(SIZES[0], 5, 2, 10_000_000, device=0)
    eng.import_state(v, t)
    yield eng, v, t
    eng.close()


@pytest.mark.parametrize("first,count", [(3, 4_001), (SIZES[0] - 1_234, 1_234), (2_048, 2_048), (4_999, 1), (7, 0)])
def test_ranges(small, gpu, first, count):
    import torch
    eng, v, t = small
    with _stream(gpu):
        want = _check_rows(_export(eng, TS, first, count, torch.cuda.current_stream(gpu).cuda_stream), v, t, TS,
                           first, count)
        assert count == 0 or want.shape[0] > 0


def test_range_past_the_table_is_refused(small, gpu):
    import torch
    from distributedratelimiting.redis_amd import _capi
    eng, _, _ = small
    n_live = torch.full((1,), -7, dtype=torch.int64, device=gpu)
    for first, count in [(SIZES[0] - 10, 11), (SIZES[0] + 1, 0)]:
        with pytest.raises(_capi.TbeError) as ei:
            eng.export_live_device(TS, None, None, None, n_live, first=first, count=count)
        assert ei.value.status == _capi.TBE_EINVAL
    torch.cuda.synchronize()
    assert int(n_live.item()) == -7


def test_capacity_below_the_live_count(small, gpu):
    import torch
    eng, v, t = small
    from distributedratelimiting.redis_amd import snapshot
    want = snapshot.live_rows(v, t, TS, TTL_MS)
    guard = 64
    with _stream(gpu):
        cur = torch.cuda.current_stream(gpu).cuda_stream
        # (700: inside a tile; 0: the counting call; the live count itself and beyond)
        for cap in (700, 1, 0, want.shape[0], want.shape[0] + 9):
            bufs = [torch.full((8 * (cap + guard),), 0xAA, dtype=torch.uint8, device=gpu) for _ in range(3)]
            d_ids, d_v, d_t = bufs[0].view(torch.int64), bufs[1].view(torch.float64), bufs[2].view(torch.int64)
            n_live = torch.full((1,), -1, dtype=torch.int64, device=gpu)
            if cap:
                eng.export_live_device(TS, d_ids, d_v, d_t, n_live, capacity=cap, stream=cur)
            else:
                eng.export_live_device(TS, None, None, None, n_live, stream=cur)
            torch.cuda.synchronize()
            assert int(n_live.item()) == want.shape[0]            # always the full count
            m = min(cap, want.shape[0])
            assert np.array_equal(d_ids.cpu().numpy()[:m], want[:m])
            assert np.array_equal(d_v.cpu().numpy()[:m].view(np.uint64), v[want[:m]].view(np.uint64))
            assert np.array_equal(d_t.cpu().numpy()[:m], t[want[:m]])
            for b in bufs:                                        # nothing past the rows written
                assert (b.cpu().numpy()[8 * m:] == 0xAA).all(), cap


def test_negative_timestamp_exports_every_present_row(small, gpu):
    import torch
    eng, v, t = small
    with _stream(gpu):
        want = _check_rows(_export(eng, -1, stream=torch.cuda.current_stream(gpu).cuda_stream), v, t, -1)
    assert np.array_equal(want, np.flatnonzero(t != ABSENT))
    assert want.shape[0] > _check_rows(_export(eng, TS), v, t, TS).shape[0]     # (stream=None: complete on return)


def test_host_buffer_form(small, gpu):
    import ctypes
    eng, v, t = small
    from distributedratelimiting.redis_amd import snapshot
    want = snapshot.live_rows(v, t, TS, TTL_MS)
    for cap in (0, 100, SIZES[0]):
        ids = np.full(cap + 8, 0xAAAA, dtype=np.uint64)
        ov = np.full(cap + 8, -3.0)
        ot = np.full(cap + 8, -3, dtype=np.int64)
        n_live = ctypes.c_uint64(0)
        eng._check(eng._lib.tbe_export_live(eng.handle, TS, 0, SIZES[0], ids.ctypes.data if cap else None,
                                            ov.ctypes.data if cap else None, ot.ctypes.data if cap else None, cap,
                                            ctypes.byref(n_live)))
        assert n_live.value == want.shape[0]
        m = min(cap, want.shape[0])
        assert np.array_equal(ids[:m].astype(np.int64), want[:m]) and (ids[m:] == 0xAAAA).all()
        assert np.array_equal(ov[:m].view(np.uint64), v[want[:m]].view(np.uint64)) and (ov[m:] == -3.0).all()
        assert np.array_equal(ot[:m], t[want[:m]]) and (ot[m:] == -3).all()


@pytest.mark.parametrize("queue_limit", [8, 2_000])
def test_queueing_kind_exports_by_the_row_rule(engine_lib, gpu, queue_limit):
    import torch
    from distributedratelimiting.redis_amd import QueueingTokenBucketEngine
    n = SIZES[0]
    v, t, _ = _table(n, "some")
    with _stream(gpu):
        eng = QueueingTokenBucketEngine(n, 5, 2, 10_000_000, queue_limit, device=0)
        assert eng.layout()["queue_header_32"] == (queue_limit <= 1024)
        eng.import_state(v, t)
        want = _check_rows(_export(eng, TS, stream=torch.cuda.current_stream(gpu).cuda_stream), v, t, TS)
        assert 0 < want.shape[0] < n
        eng.close()


def test_approximate_kind_is_rejected(engine_lib, gpu):
    import torch
    from distributedratelimiting.redis_amd import ApproximateEngine, _capi
    with _stream(gpu):
        cur = torch.cuda.current_stream(gpu).cuda_stream
        eng = ApproximateEngine(64, 5, 2, 10_000_000, 4, device=0)
        n_live = torch.full((1,), -7, dtype=torch.int64, device=gpu)
        ids = torch.zeros(4, dtype=torch.int64, device=gpu)
        val = torch.zeros(4, dtype=torch.float64, device=gpu)
        with pytest.raises(_capi.TbeError) as ei:
            eng.export_live_device(TS, None, None, None, n_live, stream=cur)
        assert ei.value.status == _capi.TBE_EINVAL
        with pytest.raises(_capi.TbeError) as ei:
            eng.import_rows(ids, val, ids, stream=cur)
        assert ei.value.status == _capi.TBE_EINVAL
        torch.cuda.synchronize()
        assert int(n_live.item()) == -7
        eng.close()


def _bits(eng):
    v, t = eng.export_state()
    return v.view(np.uint64).copy(), t.copy()


def test_import_rows_by_permuted_ids(engine_lib, gpu):
    import torch
    from distributedratelimiting.redis_amd import TokenBucketEngine, _capi
    n = SIZES[0]
    v0, t0, _ = _table(n, "some")
    rng = np.random.default_rng(29)
    with _stream(gpu):
        cur = torch.cuda.current_stream(gpu).cuda_stream
        eng = TokenBucketEngine(n, 5, 2, 10_000_000, device=0)
        eng.import_state(v0, t0)
        v0, t0 = eng.export_state()                       # (an absent row holds {TokenLimit, absent})
        # 3,000 rows in a random order of ids; every fifth is made absent
        ids = rng.permutation(n)[:3_000].astype(np.int64)
        v = rng.uniform(0.0, 5.0, ids.shape[0])
        t = TS - rng.integers(0, 9_000_000, ids.shape[0])
        t[::5] = ABSENT
        dev = [torch.from_numpy(a).to(gpu) for a in (ids, v, t)]
        eng.import_rows(*dev, stream=cur)
        # (enqueued right behind it, on the same stream: a batch that the import precedes)
        k = ids[1:2].astype(np.uint64)                    # one present row (1 is no multiple of 5)
        g = torch.empty(1, dtype=torch.uint8, device=gpu)
        r = torch.empty(1, dtype=torch.int32, device=gpu)
        eng.acquire_batch_device(torch.from_numpy(k.view(np.int64)).to(gpu),
                                 torch.zeros(1, dtype=torch.int32, device=gpu),
                                 torch.full((1,), int(t[1]), dtype=torch.int64, device=gpu), g, r, stream=cur)
        eng.synchronize()
        assert g.cpu().numpy()[0] == 1 and r.cpu().numpy()[0] == int(v[1])    # decided on the imported row
        want_v, want_t = v0.copy(), t0.copy()
        want_v[ids], want_t[ids] = v, t
        want_v[ids[::5]] = 5.0                            # INT64_MIN: {TokenLimit, absent}
        v1, t1 = eng.export_state()
        assert np.array_equal(t1, want_t)
        assert np.array_equal(v1.view(np.uint64), want_v.view(np.uint64))
        # an invalid row voids the whole call and surfaces at synchronize(), like an invalid batch
        before = _bits(eng)
        for bad_id, bad_t in ((n, TS), (7, -5)):
            ids2, v2, t2 = ids[:500].copy(), np.full(500, 1.25), np.full(500, TS, dtype=np.int64)
            ids2[321], t2[321] = bad_id, bad_t
            eng.import_rows(*[torch.from_numpy(a).to(gpu) for a in (ids2, v2, t2)], stream=cur)
            with pytest.raises(_capi.TbeError) as ei:
                eng.synchronize()
            assert ei.value.status == _capi.TBE_EINVAL
            after = _bits(eng)
            assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]), (bad_id, bad_t)
            eng.synchronize()                             # the flag is cleared once reported
        # the host-buffer form refuses the same rows directly
        for bad_id, bad_t in ((n, TS), (7, -5)):
            a = (np.array([1, bad_id], dtype=np.uint64), np.array([1.0, 2.0]), np.array([TS, bad_t], dtype=np.int64))
            st = eng._lib.tbe_import_rows(eng.handle, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, 2)
            assert st == _capi.TBE_EINVAL
        after = _bits(eng)
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
        a = (np.array([4_999, 0], dtype=np.uint64), np.array([1.5, 2.5]), np.array([TS, ABSENT], dtype=np.int64))
        eng._check(eng._lib.tbe_import_rows(eng.handle, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, 2))
        v3, t3 = eng.export_state()
        assert (v3[4_999], t3[4_999], v3[0], t3[0]) == (1.5, TS, 5.0, ABSENT)
        eng.close()
