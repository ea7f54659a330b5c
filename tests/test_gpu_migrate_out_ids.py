"""tbe_migrate_out_ids_device / tbe_migrate_out_ids (include/tbe.h): tbe_migrate_out(_device)
plus the id of every packed row.  5000 ids = two full tiles of 2,048 and a partial one, three
owners under a map, plain and classed, unheld ids and lapsed rows mixed in.  Rows and counts
must equal tbe_migrate_out_device's, the ids cluster.plan_migration's send order."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ABSENT = np.iinfo(np.int64).min
NO = np.uint64(0xFFFFFFFFFFFFFFFF)
TS = 1_760_000_100_000_123
COUNT, FIRST = 5_000, 3
N, ME = 3, 1
OPTS = (5, 2, 10_000_000)                   # TTL ceil(2.5) s
EXTRA = [(9, 1, 10_000_000), (100, 50, 10_000_000)]   # TTLs 9 s and 2 s
SENT = -0x0123456789ABCDEF


def _case():
    """(key_of_id, v, t_us, cls, owner map): 30 % of the ids unheld (their rows absent, bar a
    few), 20 % of the rows absent, 20 % last granted 3 to 4 s before TS (lapsed for the 2.5 s
    and 2 s classes, live for the 9 s one)."""
    rng = np.random.default_rng(99)
    keys = rng.integers(0, 1 << 63, COUNT, dtype=np.int64).astype(np.uint64)
    v = rng.integers(0, 0x7FE0 << 48, COUNT, dtype=np.int64).view(np.float64).copy()
    t = TS - rng.integers(0, 1_900_000, COUNT)
    old = rng.random(COUNT) < 0.2
    t[old] = TS - 3_000_000 - rng.integers(0, 1_000_000, int(old.sum()))
    gone = rng.random(COUNT) < 0.3
    keys[gone] = NO
    t[gone] = ABSENT
    t[rng.random(COUNT) < 0.2] = ABSENT
    cls = rng.integers(0, 3, COUNT).astype(np.uint8)
    m = (np.arange(4096, dtype=np.int64) * N) >> 12        # map B: odd virtual nodes to the next owner
    m[1::2] = (m[1::2] + 1) % N
    return keys, v, t.astype(np.int64), cls, m.astype(np.uint8)


def _engine(classed):
    from distributedratelimiting.redis_amd import TokenBucketEngine, cluster
    keys, v, t, cls, omap = _case()
    eng = TokenBucketEngine(FIRST + COUNT + 2, *OPTS, device=0, classes=EXTRA if classed else None)
    if classed:
        eng.set_class(np.arange(FIRST, FIRST + COUNT, dtype=np.uint64), cls)
    else:
        cls = np.zeros(COUNT, dtype=np.uint8)
    eng.import_state(v, t, first=FIRST)
    ttl = np.array([cluster.class_ttl_ms(*c) for c in [OPTS] + (EXTRA if classed else [])], dtype=np.int64)
    live = cluster.rows_live(t, TS, ttl[cls])
    rows, counts, leaving, send = cluster._plan_migration(keys, v, t, cls, live, omap, N, ME)
    assert 0 < (~live & (t != ABSENT) & leaving.astype(bool)).sum()       # lapsed rows among the leaving ids
    assert counts[0] > 0 and counts[2] > 0 and counts[N] > rows.shape[0] > 1024    # rows from all three tiles
    return eng, keys, omap, rows, counts, leaving, send + FIRST


def _device_call(eng, gpu, keys, omap, capacity, with_ids, commit=False, pad=5):
    import torch
    cur = torch.cuda.current_stream(gpu).cuda_stream
    d_k = torch.from_numpy(keys.view(np.int64).copy()).to(gpu)
    d_m = torch.from_numpy(omap.copy()).to(gpu)
    d_rows = torch.full((capacity + pad, 4), SENT, dtype=torch.int64, device=gpu)
    d_ids = torch.full((capacity + pad,), SENT, dtype=torch.int64, device=gpu)
    d_counts = torch.full((N + 2,), -1, dtype=torch.int64, device=gpu)
    d_leave = torch.full((COUNT,), 7, dtype=torch.uint8, device=gpu)
    eng.migrate_out_device(TS, d_k, d_m, N, ME, d_rows, d_counts, d_leave, commit=commit, first=FIRST,
                           capacity=capacity, stream=cur, row_ids=d_ids if with_ids else None)
    torch.cuda.synchronize()
    return d_rows.cpu().numpy(), d_counts.cpu().numpy(), d_leave.cpu().numpy(), d_ids.cpu().numpy()


@pytest.mark.parametrize("classed", [False, True], ids=["plain", "classed"])
def test_row_ids_beside_unchanged_rows(engine_lib, gpu, classed):
    import torch
    with torch.cuda.stream(torch.cuda.Stream(gpu)):
        eng, keys, omap, rows, counts, leaving, ids = _engine(classed)
        v0, t0 = eng.export_state()
        m = rows.shape[0]
        plain = _device_call(eng, gpu, keys, omap, m, with_ids=False)
        got = _device_call(eng, gpu, keys, omap, m, with_ids=True)
        # rows, counts and flags: tbe_migrate_out_device's, which are the plan's
        assert np.array_equal(plain[0][:m], rows) and np.array_equal(plain[1], counts)
        for a, b in zip(plain[:3], got[:3]):
            assert np.array_equal(a, b)
        assert np.all(plain[3] == SENT)                   # no id output asked for, none written
        assert np.array_equal(got[3][:m], ids) and np.all(got[3][m:] == SENT)
        assert np.array_equal(got[2], leaving)
        # a capacity below the row count: nothing at or past it, in either array
        short = m - 500
        got = _device_call(eng, gpu, keys, omap, short, with_ids=True)
        assert np.array_equal(got[0][:short], rows[:short]) and np.all(got[0][short:] == SENT)
        assert np.array_equal(got[3][:short], ids[:short]) and np.all(got[3][short:] == SENT)
        assert np.array_equal(got[1], counts)
        # commit == 0 read only
        v1, t1 = eng.export_state()
        assert np.array_equal(t1, t0) and np.array_equal(v1.view(np.int64), v0.view(np.int64))
        # the host form, without and with ids, then a commit with ids
        h = eng.migrate_out(TS, keys, omap, N, ME, first=FIRST)
        assert len(h) == 3 and np.array_equal(h[0][:m], rows) and np.array_equal(h[1].astype(np.int64), counts)
        h = eng.migrate_out(TS, keys, omap, N, ME, first=FIRST, row_ids=True)
        assert np.array_equal(h[0][:m], rows) and np.array_equal(h[1].astype(np.int64), counts)
        assert np.array_equal(h[2], leaving) and np.array_equal(h[3][:m].astype(np.int64), ids)
        assert not h[3][m:].any()
        h = eng.migrate_out(TS, keys, omap, N, ME, first=FIRST, capacity=short, row_ids=True)
        assert np.array_equal(h[0], rows[:short]) and np.array_equal(h[3].astype(np.int64), ids[:short])
        v1, t1 = eng.export_state()
        assert np.array_equal(t1, t0)
        h = eng.migrate_out(TS, keys, omap, N, ME, first=FIRST, commit=True, row_ids=True)
        assert np.array_equal(h[0][:m], rows) and np.array_equal(h[3][:m].astype(np.int64), ids)
        v1, t1 = eng.export_state()
        gone = FIRST + np.flatnonzero(leaving)
        assert np.all(t1[gone] == ABSENT) and np.array_equal(np.delete(t1, gone), np.delete(t0, gone))
        eng.synchronize()                                  # no call was refused
        eng.close()
