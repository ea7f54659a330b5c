"""tbe_approx_idle_device / tbe_approx_reset_device on the GPU: the scan against the numpy
statement of the idle rule (snapshot.approx_idle_rows) over the engine's own exported state,
with the client view derived (after a one-client refresh) and written (after a two-client
sync); the reset against a new engine, with unflagged neighbours bit-identical; and two
clients of one replicated tier that must agree before a key is dropped."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ABSENT = np.iinfo(np.int64).min
T0 = 1_760_572_800 * 1_000_000
LIMIT, TOKENS, TICKS, QLIMIT = 5, 2, 10_000_000, 4     # 2 tokens per second


def _stream(gpu):
    import torch
    return torch.cuda.stream(torch.cuda.Stream(gpu))


def _cur(gpu):
    import torch
    return torch.cuda.current_stream(gpu).cuda_stream


def _state(eng, keys=None):
    """(local, global, est, available, queued) arrays and the tier (v, p, t_us), all keys."""
    keys = range(eng.n_keys) if keys is None else keys
    ls = np.array([eng.local_state(k) for k in keys], dtype=np.float64).reshape(-1, 5)
    v, p, t = eng.export_global()
    return ls, v, p, t


def _rule(state, ts_us):
    from distributedratelimiting.redis_amd import fill_rate, snapshot
    ls, v, _, t = state
    return snapshot.approx_idle_rows(ls[:, 0].astype(np.int64), ls[:, 1].astype(np.int64), ls[:, 4].astype(np.int64),
                                     v, t, ts_us, fill_rate(TOKENS, TICKS))


def _scan(eng, ts_us, first, count, gpu):
    import torch
    d = torch.full((count,), 0xAA, dtype=torch.uint8, device=gpu)
    eng.idle_device(ts_us, d, first=first, stream=_cur(gpu))
    torch.cuda.synchronize()
    return d.cpu().numpy()


def _traffic(eng, rng, n_keys, n, id_base, hot=None):
    keys = rng.integers(0, n_keys if hot is None else hot, n).astype(np.uint64)
    permits = rng.choice([0, 1, 1, 2, 3], n).astype(np.int32)
    eng.acquire_batch(keys, permits, wait=True, id_base=id_base)


RANGES = [(0, 1), (3, 2047), (3, 2048), (3, 2049), (0, 5000)]


def test_scan_matches_the_rule_lazy_and_written(engine_lib, gpu):
    import torch
    from distributedratelimiting.redis_amd import ApproximateEngine, TokenBucketEngine, _capi
    n_keys = 5000
    rng = np.random.default_rng(17)
    with _stream(gpu):
        eng = ApproximateEngine(n_keys, LIMIT, TOKENS, TICKS, QLIMIT, device=0)
        torch.cuda.synchronize()
        _traffic(eng, rng, n_keys, 9000, 0, hot=3500)        # keys 3500.. never see a request
        eng.refresh(T0)                                      # one client: the view is derived from now on
        _traffic(eng, rng, n_keys, 1500, 100_000, hot=1200)  # estimate infinite: these queue (zero permits too)
        eng.refresh(T0 + 1_300_000)                          # decay 2.6: rows of 3 tokens keep 0.4, global 0
        _traffic(eng, rng, n_keys, 600, 200_000, hot=700)    # local > 0 on rows of every kind
        state = _state(eng)                                  # (the scans change nothing)
        ts = T0 + 1_400_000                                  # 0.4 - 0.1 * 2 > 0: not idle yet
        want = _rule(state, ts)
        assert 0.05 * n_keys < int(want.sum()) < 0.95 * n_keys
        for first, count in RANGES:
            got = _scan(eng, ts, first, count, gpu)
            assert np.array_equal(got, want[first:first + count].astype(np.uint8)), (first, count)
        # 0.2 s later the rows of 0.4 are worth nothing; then an earlier timestamp (before t)
        # and one at which every row has lapsed
        later = _rule(state, T0 + 1_600_000)
        assert int(later.sum()) > int(want.sum())
        assert np.array_equal(_scan(eng, T0 + 1_600_000, 0, n_keys, gpu), later.astype(np.uint8))
        for other in (T0, T0 + 90_000 * 1_000_000):
            assert np.array_equal(_scan(eng, other, 0, n_keys, gpu), _rule(state, other).astype(np.uint8))

        # bad arguments write nothing
        tb = TokenBucketEngine(64, LIMIT, TOKENS, TICKS, device=0)
        d = torch.full((64,), 0xAA, dtype=torch.uint8, device=gpu)
        for bad in (lambda: eng.idle_device(-1, d, stream=_cur(gpu)),
                    lambda: eng.idle_device(ts, d, first=n_keys - 63, stream=_cur(gpu)),
                    lambda: eng.idle_device(ts, d, first=n_keys + 1, stream=_cur(gpu)),
                    lambda: tb._check(tb._lib.tbe_approx_idle_device(tb.handle, ts, 0, 64, d.data_ptr(), _cur(gpu))),
                    lambda: tb._check(tb._lib.tbe_approx_reset_device(tb.handle, 0, 64, d.data_ptr(), _cur(gpu))),
                    lambda: eng.reset_device(d, first=n_keys - 63, stream=_cur(gpu))):
            with pytest.raises(_capi.TbeError) as ei:
                bad()
            assert ei.value.status == _capi.TBE_EINVAL
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == 0xAA).all()
        tb.close()

        # a two-client sync writes the view: client 0 of 2, the other client's counts random
        counts = torch.zeros(n_keys, dtype=torch.int32, device=gpu)
        eng.collect(counts)
        other = torch.from_numpy((rng.integers(0, 4, n_keys) == 0).astype(np.int32)).to(gpu)
        allc = torch.cat([counts, other])
        torch.cuda.synchronize()
        eng.sync(allc, 2, 0, T0 + 3_000_000, 400_000)
        _traffic(eng, rng, n_keys, 500, 300_000, hot=900)
        ts = T0 + 4_500_000
        state = _state(eng)
        want = _rule(state, ts)
        assert int((state[0][:, 1] != np.trunc(state[1])).sum()) > 0     # the view is no longer (int)v
        assert 0.05 * n_keys < int(want.sum()) < 0.95 * n_keys
        for first, count in RANGES:
            got = _scan(eng, ts, first, count, gpu)
            assert np.array_equal(got, want[first:first + count].astype(np.uint8)), (first, count)
        # the host form is the same scan
        idle = np.full(2049, 0xAA, dtype=np.uint8)
        eng._check(eng._lib.tbe_approx_idle(eng.handle, ts, 3, 2049, idle.ctypes.data))
        assert np.array_equal(idle, want[3:3 + 2049].astype(np.uint8))
        eng.close()


@pytest.mark.parametrize("lazy", [True, False])
def test_reset_gives_a_new_engines_state(engine_lib, gpu, lazy):
    import torch
    from distributedratelimiting.redis_amd import ApproximateEngine
    n_keys = 600
    rng = np.random.default_rng(23 + lazy)
    with _stream(gpu):
        eng = ApproximateEngine(n_keys, LIMIT, TOKENS, TICKS, QLIMIT, device=0)
        new = ApproximateEngine(n_keys, LIMIT, TOKENS, TICKS, QLIMIT, device=0)
        torch.cuda.synchronize()
        _traffic(eng, rng, n_keys, 1500, 0)
        eng.refresh(T0)
        _traffic(eng, rng, n_keys, 800, 10_000)              # queues fill while the estimate is infinite
        if lazy:
            eng.refresh(T0 + 700_000)
        else:
            counts = torch.zeros(n_keys, dtype=torch.int32, device=gpu)
            eng.collect(counts)
            allc = torch.cat([counts, torch.ones_like(counts)])
            torch.cuda.synchronize()
            eng.sync(allc, 2, 0, T0 + 700_000, 100_000)
        _traffic(eng, rng, n_keys, 400, 20_000)
        ls0, v0, p0, t0 = _state(eng)
        q0 = [eng.queue_of(k) for k in range(n_keys)]
        assert sum(1 for q in q0 if q) > 20 and int((ls0[:, 0] != 0).sum()) > 20 and np.isfinite(ls0[:, 2]).any()
        first, count = 5, n_keys - 9
        flags = np.zeros(count, dtype=np.uint8)
        flags[rng.integers(0, 3, count) == 0] = 1
        flags[[0, count - 1]] = 1
        flags[flags.nonzero()[0][3]] = 0x80                   # any non-zero byte is a flag
        d_flags = torch.from_numpy(flags).to(gpu)
        eng.reset_device(d_flags, first=first, stream=_cur(gpu))
        torch.cuda.synchronize()
        ls1, v1, p1, t1 = _state(eng)
        q1 = [eng.queue_of(k) for k in range(n_keys)]
        hit = np.zeros(n_keys, dtype=bool)
        hit[first:first + count] = flags != 0
        assert 100 < int(hit.sum()) < n_keys - 100
        # flagged: a new engine's query, tier row and queue
        lsn, vn, pn, tn = _state(new, keys=[0])
        assert lsn.tolist() == [[0.0, 0.0, 1.0, float(LIMIT), 0.0]] and (vn[0], pn[0], tn[0]) == (0.0, 0.0, ABSENT)
        assert (ls1[hit] == lsn[0]).all()
        assert (v1[hit].view(np.uint64) == 0).all() and (p1[hit].view(np.uint64) == 0).all() and (t1[hit] == ABSENT).all()
        assert all(q1[k] == [] for k in np.flatnonzero(hit))
        # unflagged neighbours, the rows outside the range included: bit-identical
        keep = ~hit
        assert np.array_equal(ls1[keep].view(np.uint64), ls0[keep].view(np.uint64))
        assert np.array_equal(v1[keep].view(np.uint64), v0[keep].view(np.uint64))
        assert np.array_equal(p1[keep].view(np.uint64), p0[keep].view(np.uint64))
        assert np.array_equal(t1[keep], t0[keep])
        assert all(q1[k] == q0[k] for k in np.flatnonzero(keep))
        # a reset key decides as a new engine's key does, now and through the next refresh
        ks = np.repeat(np.flatnonzero(hit)[:40].astype(np.uint64), 3)
        ps = np.tile(np.array([3, 2, 1], dtype=np.int32), 40)
        a = eng.acquire_batch(ks, ps, wait=True, id_base=50_000)
        b = new.acquire_batch(ks, ps, wait=True, id_base=50_000)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        eng.refresh(T0 + 2_000_000)
        new.refresh(T0 + 2_000_000)
        for k in np.flatnonzero(hit)[:40]:
            assert eng.local_state(int(k)) == new.local_state(int(k))
        va, pa, ta = eng.export_global()
        vb, pb, tb = new.export_global()
        for x, y in ((va, vb), (pa, pb), (ta, tb)):
            assert np.array_equal(x[hit].view(np.uint64), y[hit].view(np.uint64))
        # the host form: the same reset
        hflags = np.zeros(n_keys, dtype=np.uint8)
        hflags[7] = 1
        eng._check(eng._lib.tbe_approx_reset(eng.handle, 0, n_keys, hflags.ctypes.data))
        assert eng.local_state(7) == (0, 0, 1.0, LIMIT, 0) and eng.export_global(7, 1)[2][0] == ABSENT
        eng.close()
        new.close()


def test_two_clients_agree_before_a_key_is_dropped(engine_lib, gpu):
    """Clients A and B of one replicated tier on one GPU, each behind its own directory with
    the same keys.  A key that is idle for A and in use by B is, after the flags are combined,
    neither reclaimed nor reset in either engine; a key idle for both goes in both."""
    import torch
    from distributedratelimiting.redis_amd import ApproximateEngine
    from distributedratelimiting.redis_amd.cluster import DeviceDirectory
    cap = 64
    gkeys = (np.arange(1, 11, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)
    with _stream(gpu):
        engs = [ApproximateEngine(cap, LIMIT, TOKENS, TICKS, QLIMIT, device=0) for _ in range(2)]
        dirs = [DeviceDirectory(cap, device=0) for _ in range(2)]
        d_keys = torch.from_numpy(gkeys).to(gpu)
        ids = [d.assign(d_keys).cpu().numpy() for d in dirs]
        assert np.array_equal(ids[0], ids[1])
        ids = ids[0]
        counts = [torch.zeros(cap, dtype=torch.int32, device=gpu) for _ in range(2)]

        def epoch(ts):
            for e, c in zip(engs, counts):
                e.collect(c)
            allc = torch.cat(counts)
            torch.cuda.synchronize()
            for r, e in enumerate(engs):
                e.sync(allc, 2, r, ts, 1000)

        epoch(T0)
        epoch(T0 + 1_000_000)                                # the estimate leaves its warm-up
        used, queued, both = int(ids[2]), int(ids[5]), int(ids[7])
        st, _, _ = engs[1].acquire_batch(np.array([used], np.uint64), np.array([1], np.int32), wait=False)
        assert st.tolist() == [1]                            # B holds a token of `used`
        st, _, _ = engs[1].acquire_batch(np.array([queued] * 2, np.uint64), np.array([1, 4], np.int32),
                                         wait=True, id_base=10)
        assert st.tolist()[1] == 2                           # B queues on `queued`
        ts = T0 + 1_500_000
        before = [[e.local_state(k) for k in (used, queued, both)] for e in engs]
        tier_before = [e.export_global() for e in engs]
        flags = []
        for e in engs:
            d = torch.empty(cap, dtype=torch.uint8, device=gpu)
            e.idle_device(ts, d, stream=_cur(gpu))
            flags.append(d)
        fa, fb = (f.cpu().numpy() for f in flags)
        assert fa[used] == 1 and fb[used] == 0 and fa[queued] == 1 and fb[queued] == 0 and fa[both] == fb[both] == 1
        # the agreement of cluster.approx_idle_epoch: sum the "not idle" flags, idle where 0
        busy = (flags[0] == 0).to(torch.int32) + (flags[1] == 0).to(torch.int32)
        agreed = (busy == 0).to(torch.uint8)
        removed = [d.reclaim_idle(e, ts, d_idle=agreed.clone())[0] for d, e in zip(dirs, engs)]
        torch.cuda.synchronize()
        assert [int(r.item()) for r in removed] == [8, 8]
        for r, (d, e) in enumerate(zip(dirs, engs)):
            got = d.lookup(d_keys).cpu().numpy()
            held = np.isin(np.arange(10), [2, 5])
            assert np.array_equal(got[held], ids[held]) and (got[~held] == -1).all()
            assert [e.local_state(k) for k in (used, queued)] == before[r][:2]      # neither reset
            assert e.local_state(used)[2] in (5.0, 6.0)                             # (a reset key has estimate 1)
            assert e.local_state(both) == (0, 0, 1.0, LIMIT, 0)
            v, p, t = e.export_global()
            for k in (used, queued):
                assert (v[k], p[k], t[k]) == (tier_before[r][0][k], tier_before[r][1][k], tier_before[r][2][k])
            assert t[both] == ABSENT and p[both] == 0.0
        assert engs[1].queue_of(queued) == [(11, 4)] or engs[1].queue_of(queued) == [(10, 1), (11, 4)]
        # replicas and directories stay identical
        for x, y in zip(engs[0].export_global(), engs[1].export_global()):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        again = [d.assign(d_keys).cpu().numpy() for d in dirs]
        assert np.array_equal(again[0], again[1])
        # keep_ids: an id named there is neither removed nor reset
        keep = torch.tensor([int(again[0][0])], dtype=torch.int64, device=gpu)
        n0 = dirs[0].reclaim_idle(engs[0], ts, keep_ids=keep)[0]
        torch.cuda.synchronize()
        assert int(n0.item()) == 9 and int(dirs[0].lookup(d_keys[:1]).item()) == int(again[0][0])
        for x in engs + dirs:
            x.close()
