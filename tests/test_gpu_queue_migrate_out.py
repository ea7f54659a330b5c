"""tbe_queue_migrate_out_ids_device / tbe_queue_migrate_out_ids (include/tbe.h) against
cluster.plan_queue_migration: counts, leaving flags, rows (word 3 = class | entries << 8) and
row ids identical, and table and queues after a commit + clearing export as the header says.

5,000 ids (two full tiles of 2,048 and a partial one), about 20% of them held by no key.
Rows and queues are put in place through import_state and queue_import_ids, never through
decisions: live rows, lapsed rows and absent rows, each with and without queued entries.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ABSENT = np.iinfo(np.int64).min
NO = np.uint64(0xFFFFFFFFFFFFFFFF)
TS = 1_760_000_100_000_123
COUNT = 5_000
SENT = -0x0123456789ABCDEF
# (TokenLimit, TokensPerPeriod, ticks, QueueLimit, order): TTLs 4 s, 3 s, 3 s
QC = [(4, 1, 10_000_000, 8, 0), (3, 1, 10_000_000, 5, 1), (6, 2, 10_000_000, 40, 0)]


def _owner_map(kind, n, me):
    if kind is None:
        return None
    m = (np.arange(4096, dtype=np.int64) * n) >> 12        # map B: odd virtual nodes to the next owner
    m[1::2] = (m[1::2] + 1) % n
    return m.astype(np.uint8)


def _setup(classed, seed=0):
    """An engine whose ids hold: key or none, a live / lapsed / absent row, a queue or none."""
    from distributedratelimiting.redis_amd import QueueingTokenBucketEngine, cluster
    rng = np.random.default_rng(77 + seed)
    classes = QC if classed else QC[:1]
    eng = QueueingTokenBucketEngine(COUNT, *classes[0], device=0, classes=classes[1:] if classed else None)
    ids = np.arange(COUNT, dtype=np.uint64)
    cls = (ids % np.uint64(3)).astype(np.uint8) if classed else np.zeros(COUNT, dtype=np.uint8)
    if classed:
        eng.set_class(ids, cls)
    kof = rng.integers(0, 1 << 63, COUNT, dtype=np.int64).astype(np.uint64)
    unheld = rng.random(COUNT) < 0.2
    kof[unheld] = NO
    v = rng.integers(0, 0x7FE0 << 48, COUNT, dtype=np.int64).view(np.float64).copy()
    t = (TS - rng.integers(0, 2_000_000, COUNT)).astype(np.int64)          # live for every class
    kind = rng.integers(0, 3, COUNT)                                       # 0 live, 1 lapsed, 2 absent
    t[kind == 1] = TS - 6_000_000 - rng.integers(0, 1_000_000, int((kind == 1).sum()))
    t[kind == 2] = ABSENT
    t[unheld] = ABSENT
    qcount = np.where(rng.random(COUNT) < 0.4, rng.integers(1, 4, COUNT), 0).astype(np.uint32)
    qcount[unheld] = 0
    ne = int(qcount.sum())
    ent = ((np.arange(ne, dtype=np.uint64) + np.uint64(1 << 41)) << np.uint64(16)) | np.uint64(1)
    eng.import_state(v, t)
    v, t1 = eng.export_state()                                             # an absent row holds {TokenLimit, absent}
    assert np.array_equal(t1, t)
    eng.queue_import_ids(ids, qcount, ent)
    ttl = np.array([cluster.class_ttl_ms(*c[:3]) for c in classes], dtype=np.int64)[cls]
    live = cluster.rows_live(t, TS, ttl)
    held = ~unheld
    groups = {"lapsed, queued": held & (kind == 1) & (qcount > 0), "absent, queued": held & (kind == 2) & (qcount > 0),
              "lapsed, empty": held & (kind == 1) & (qcount == 0), "live, queued": held & (kind == 0) & (qcount > 0)}
    print({k: int(m.sum()) for k, m in groups.items()}, "unheld", int(unheld.sum()))
    assert all(int(m.sum()) >= 300 for m in groups.values()) and 800 <= int(unheld.sum()) <= 1_200
    assert not live[kind == 1].any()
    return eng, dict(kof=kof, v=v, t=t, cls=cls, live=live, qcount=qcount, ent=ent, groups=groups)


def _call(eng, gpu, s, omap, n, me, capacity, commit=False, pad=4):
    import torch
    d_k = torch.from_numpy(s["kof"].view(np.int64).copy()).to(gpu)
    d_m = None if omap is None else torch.from_numpy(omap.copy()).to(gpu)
    d_rows = torch.full((capacity + pad, 4), SENT, dtype=torch.int64, device=gpu)
    d_ids = torch.full((capacity + pad,), SENT, dtype=torch.int64, device=gpu)
    d_counts = torch.full((n + 2,), -1, dtype=torch.int64, device=gpu)
    d_leave = torch.full((COUNT,), 7, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    eng.queue_migrate_out_device(TS, d_k, d_m, n, me, d_rows if capacity else None, d_counts, d_leave, commit=commit,
                                 capacity=capacity, row_ids=d_ids if capacity else None)
    torch.cuda.synchronize()
    return d_rows.cpu().numpy(), d_counts.cpu().numpy(), d_leave.cpu().numpy(), d_ids.cpu().numpy()


def _state(eng):
    v, t = eng.export_state()
    q, st, e, _ = eng.queue_export_ids(np.arange(COUNT, dtype=np.uint64))
    return v.view(np.int64).copy(), t.copy(), q, st, e


@pytest.mark.parametrize("classed", [False, True], ids=["plain", "classed"])
def test_rows_counts_flags_and_ids_against_the_plan(engine_lib, gpu, classed):
    from distributedratelimiting.redis_amd import cluster
    eng, s = _setup(classed)
    before = _state(eng)
    for n, me in [(2, 0), (2, 1), (8, 0), (8, 5)]:
        for kind in ("B", None):
            omap = _owner_map(kind, n, me)
            rows, counts, leaving, row_ids = cluster.plan_queue_migration(
                s["kof"], s["v"], s["t"], s["cls"], s["live"], s["qcount"], omap, n, me)
            m = rows.shape[0]
            lv = leaving.astype(bool)
            # queued keys are sent whatever their row holds, verbatim; lapsed empty ones are not
            sent = np.zeros(COUNT, dtype=bool)
            sent[row_ids] = True
            g = s["groups"]
            for name in ("lapsed, queued", "absent, queued", "live, queued"):
                assert sent[g[name] & lv].all() and (g[name] & lv).sum() >= 20, name
            assert not sent[g["lapsed, empty"]].any() and (g["lapsed, empty"] & lv).sum() >= 20
            assert np.array_equal(rows[:, 2], s["t"][row_ids]) and np.array_equal(rows[:, 3] >> 8, s["qcount"][row_ids])
            got = _call(eng, gpu, s, omap, n, me, COUNT)
            assert np.array_equal(got[1], counts), (n, me, kind)
            assert np.array_equal(got[2], leaving), (n, me, kind)
            assert np.array_equal(got[0][:m], rows) and np.all(got[0][m:] == SENT), (n, me, kind)
            assert np.array_equal(got[3][:m], row_ids) and np.all(got[3][m:] == SENT), (n, me, kind)
            h = eng.queue_migrate_out(TS, s["kof"], omap, n, me)
            assert np.array_equal(h[1].astype(np.int64), counts) and np.array_equal(h[2], leaving)
            assert np.array_equal(h[0][:m], rows) and np.array_equal(h[3][:m].astype(np.int64), row_ids)
            c0 = _call(eng, gpu, s, omap, n, me, 0)                        # counting call
            assert np.array_equal(c0[1], counts) and np.array_equal(c0[2], leaving)
    eng.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(before, _state(eng)))   # commit == 0 reads only
    eng.close()


@pytest.mark.parametrize("classed", [False, True], ids=["plain", "classed"])
def test_commit_then_clearing_export(engine_lib, gpu, classed):
    import torch
    from distributedratelimiting.redis_amd import cluster
    eng, s = _setup(classed, seed=1)
    n, me = 2, 1                                   # about half of the 4,000 held ids stay, 40% of them queued: ~800
    omap = _owner_map("B", n, me)
    rows, counts, leaving, row_ids = cluster.plan_queue_migration(
        s["kof"], s["v"], s["t"], s["cls"], s["live"], s["qcount"], omap, n, me)
    m = rows.shape[0]
    before = _state(eng)
    got = _call(eng, gpu, s, omap, n, me, m, commit=True)
    assert np.array_equal(got[0][:m], rows) and np.array_equal(got[3][:m], row_ids)
    eng.synchronize()
    mid = _state(eng)
    assert np.array_equal(mid[2], before[2]) and np.array_equal(mid[4], before[4])   # the commit leaves the queues alone
    ne = int(s["qcount"][row_ids].sum())
    d_ids = torch.from_numpy(row_ids.copy()).to(gpu)
    d_q = torch.zeros(m, dtype=torch.int32, device=gpu)
    d_e = torch.zeros(ne, dtype=torch.int64, device=gpu)
    d_n = torch.zeros(1, dtype=torch.int64, device=gpu)
    torch.cuda.synchronize()
    eng.queue_export_ids_device(d_ids, d_q, None, d_e, d_n, clear=True)
    torch.cuda.synchronize()
    eng.synchronize()
    assert int(d_n.item()) == ne and np.array_equal(d_q.cpu().numpy(), (rows[:, 3] >> 8).astype(np.int32))
    starts = np.concatenate([[0], np.cumsum(s["qcount"].astype(np.int64))])
    want = np.concatenate([s["ent"][starts[i]:starts[i + 1]] for i in row_ids.tolist()] + [np.zeros(0, dtype=np.uint64)])
    assert np.array_equal(d_e.cpu().numpy().view(np.uint64), want)
    after = _state(eng)
    lv = leaving.astype(bool)
    caps = np.array([c[0] for c in QC], dtype=np.float64)[s["cls"]]
    assert np.all(after[1][lv] == ABSENT) and np.array_equal(after[0][lv], caps[lv].view(np.int64))
    assert not after[2][lv].any()                                         # every leaving queue is gone
    assert np.array_equal(after[0][~lv], before[0][~lv]) and np.array_equal(after[1][~lv], before[1][~lv])
    assert np.array_equal(after[2][~lv], before[2][~lv])
    keep = np.repeat(~lv, before[2].astype(np.int64))
    assert np.array_equal(after[4], before[4][keep]) and int((~lv & (before[2] > 0)).sum()) >= 500
    eng.close()


def test_an_orphan_with_only_a_queue_refuses_the_commit(engine_lib, gpu):
    from distributedratelimiting.redis_amd import TbeError
    eng, s = _setup(False, seed=2)
    orphan = int(np.flatnonzero((s["kof"] == NO))[5])
    eng.queue_import_ids([orphan], [2], [(5 << 16) | 1, (6 << 16) | 1])     # absent row, two queued entries
    before = _state(eng)
    n, me = 2, 0
    omap = _owner_map("B", n, me)
    got = _call(eng, gpu, s, omap, n, me, COUNT, commit=True)
    assert got[1][n + 1] == 1
    with pytest.raises(TbeError):
        eng.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(before, _state(eng)))
    with pytest.raises(TbeError):
        eng.queue_migrate_out(TS, s["kof"], omap, n, me, commit=True)
    eng.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(before, _state(eng)))
    assert eng.queue_migrate_out(TS, s["kof"], omap, n, me)[1][n + 1] == 1   # reading is fine
    eng.close()


def test_a_bad_map_entry_writes_nothing(engine_lib, gpu):
    from distributedratelimiting.redis_amd import TbeError
    eng, s = _setup(False, seed=3)
    before = _state(eng)
    n, me = 2, 0
    omap = _owner_map("B", n, me)
    omap[::7] = n
    got = _call(eng, gpu, s, omap, n, me, COUNT, commit=True)
    assert np.all(got[0] == SENT) and np.all(got[3] == SENT)
    with pytest.raises(TbeError):
        eng.synchronize()
    with pytest.raises(TbeError):
        eng.queue_migrate_out(TS, s["kof"], omap, n, me, commit=True)
    assert all(np.array_equal(a, b) for a, b in zip(before, _state(eng)))
    eng.close()
