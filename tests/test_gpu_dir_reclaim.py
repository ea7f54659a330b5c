"""Reclaiming expired keys in the device u64 key directory (include/tbe_cluster.h:
tbe_dir_reclaim, tbe_dir_reclaim_device) against the host mirror's id rule and against what
Redis would answer: one bucket per key, dropped at its EXPIRE (TB:232-235).  Every
comparison is exact: ids, keys, counts and replies."""
import numpy as np
import pytest

from oracle import cref

pytestmark = pytest.mark.gpu

NONE = int(2**64 - 1)
ABSENT = np.iinfo(np.int64).min
T0 = 1_760_000_000_000_000
TTL_MS = 3_000                      # limit 5 at 2 tokens per second: ceil(2.5) s
GAMMA = np.uint64(0x9E3779B97F4A7C15)


def _side_stream(gpu):
    import torch
    return torch.cuda.stream(torch.cuda.Stream(gpu))


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev(keys, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64)).to(gpu)


def _gkey(num):
    """A global u64 key per small number (a bijection: an odd multiplier)."""
    with np.errstate(over="ignore"):
        return np.asarray(num, dtype=np.uint64) * GAMMA + np.uint64(0x5851F42D4C957F2D)


def _decide(eng, ids, permits, ts, gpu):
    """One engine batch on device ids, on the current stream; (granted, remaining)."""
    import torch
    n = ids.numel()
    g = torch.empty(n, dtype=torch.uint8, device=gpu)
    r = torch.empty(n, dtype=torch.int32, device=gpu)
    eng.acquire_batch_device(ids, torch.from_numpy(np.asarray(permits, dtype=np.int32)).to(gpu),
                             torch.from_numpy(np.asarray(ts, dtype=np.int64)).to(gpu), g, r,
                             stream=torch.cuda.current_stream(gpu).cuda_stream)
    return g.cpu().numpy(), r.cpu().numpy()


def _flags(cap, ids, gpu):
    import torch
    f = np.zeros(cap, dtype=np.uint8)
    f[np.asarray(ids, dtype=np.int64)] = 1
    return torch.from_numpy(f).to(gpu)


def _erange(d):
    from distributedratelimiting.redis_amd import _capi
    with pytest.raises(_capi.TbeError) as ei:
        d.size()
    return ei.value.status == _capi.TBE_ERANGE


def test_churn_against_redis_truth(engine_lib, gpu):
    """12 cycles of a sliding key window: far more distinct keys than ids or slots pass
    through, under 6,000 are ever held.  Ids follow the mirror, replies follow one bucket
    per global key with natural expiry, and each reclaim removes exactly the keys whose
    bucket is gone."""
    from distributedratelimiting.redis_amd import TokenBucketEngine, fill_rate
    from distributedratelimiting.redis_amd.cluster import DeviceDirectory, HostDirectory
    cap = 8_192
    rng = np.random.default_rng(23)
    with _side_stream(gpu):
        d = DeviceDirectory(cap, device=0)
        h = HostDirectory(cap)
        eng = TokenBucketEngine(cap, 5, 2, 10_000_000, device=0)
        ref = cref.CTokenBucket(2_000 * 11 + 4_000, 5, fill_rate(2, 10_000_000))
        num_of = dict(zip(_gkey(np.arange(26_000)).tolist(), range(26_000)))
        seen = set()
        peak = 0
        for c in range(12):
            num = rng.integers(2_000 * c, 2_000 * c + 4_000, 3_000)
            keys = _gkey(num)
            seen.update(num.tolist())
            want_ids = h.assign(keys)
            peak = max(peak, h.size())
            ids = d.assign(_dev(keys, gpu))
            assert np.array_equal(_u64(ids), want_ids), c
            ts = np.full(3_000, T0 + 2_000_000 * c, dtype=np.int64)
            p = rng.integers(0, 4, 3_000).astype(np.int32)
            g, r = _decide(eng, ids, p, ts, gpu)
            g_ref, r_ref = ref.acquire_batch(num.astype(np.uint64), p, ts)   # keyed by the global key
            assert np.array_equal(g, g_ref) and np.array_equal(r, r_ref), c
            # Redis truth: a key is gone when its bucket's last grant is a TTL behind
            _, t_ref = ref.export_state()
            gone = (t_ref == ABSENT) | (t_ref < 1000 * (int(ts[0]) // 1000 - TTL_MS))
            dead = [i for k, i in h.ids.items() if gone[num_of[k]]]
            n_dead = h.reclaim(dead)
            assert d.reclaim(eng, int(ts[0])) == n_dead, c
            assert d.size() == h.size(), c
        print("distinct keys", len(seen), "peak held", peak, "held at end", h.size())
        assert len(seen) > 2 * cap and peak < 6_000      # far past capacity without a reclaim
        probe = _gkey(np.arange(18_000, 26_000, 3))       # held and removed keys
        assert np.array_equal(_u64(d.lookup(_dev(probe, gpu))), h.lookup(probe))
        assert 0 < int((h.lookup(probe) != np.uint64(NONE)).sum()) < probe.shape[0]
        eng.close()
        d.close()


@pytest.mark.parametrize("which", ["alternate", "all", "none"])
def test_probe_chains_across_the_table_end(engine_lib, gpu, which):
    """48 keys whose home slots are the last four and first four of 128: one cluster that
    wraps the table end.  After the victims leave, every survivor is still found through
    what were the victims' slots, and the victims come back under the mirror's ids."""
    from distributedratelimiting.redis_amd.cluster import DeviceDirectory, HostDirectory, _mix64
    cap, nslots = 64, 128
    cand = _gkey(np.arange(1, 20_000))
    home = (_mix64(cand) & np.uint64(nslots - 1)).astype(np.int64)   # k_dir_claim: mix64(key) & smask
    keys = cand[(home >= nslots - 4) | (home < 4)][:48]
    assert keys.shape[0] == 48
    assert set(((_mix64(keys) & np.uint64(nslots - 1)).astype(np.int64)).tolist()) == {124, 125, 126, 127, 0, 1, 2, 3}
    victims = {"alternate": keys[::2], "all": keys, "none": keys[:0]}[which]
    with _side_stream(gpu):
        d = DeviceDirectory(cap, device=0)
        h = HostDirectory(cap)
        ids = h.assign(keys)
        assert np.array_equal(_u64(d.assign(_dev(keys, gpu))), ids)
        vid = h.lookup(victims).astype(np.int64)
        count = d.reclaim_device(_flags(cap, vid, gpu))
        assert int(count.item()) == h.reclaim(vid.tolist()) == victims.shape[0]
        got = _u64(d.lookup(_dev(keys, gpu)))
        assert np.array_equal(got, h.lookup(keys))
        gone = np.isin(keys, victims)
        assert np.array_equal(got[~gone], ids[~gone]) and (got[gone] == np.uint64(NONE)).all()
        assert d.size() == h.size() == 48 - victims.shape[0]
        # the victims come back (reversed: other first occurrences), then everything resolves
        back = victims[::-1]
        if back.shape[0]:
            assert np.array_equal(_u64(d.assign(_dev(back, gpu))), h.assign(back))
        assert np.array_equal(_u64(d.assign(_dev(keys, gpu))), h.assign(keys))
        assert np.array_equal(_u64(d.lookup(_dev(keys, gpu))), h.lookup(keys))
        assert d.size() == h.size() == 48
        d.close()


def test_stack_then_counter_across_tiles_and_overflow(engine_lib, gpu):
    """One batch takes 700 ids from the stack and 1,300 from the counter, its new keys
    spread over three 1,024-request blocks; a batch past the room overflows, and a reclaim
    afterwards works but leaves the error in place."""
    from distributedratelimiting.redis_amd.cluster import DeviceDirectory, HostDirectory
    cap = 4_096
    rng = np.random.default_rng(5)
    with _side_stream(gpu):
        d = DeviceDirectory(cap, device=0)
        h = HostDirectory(cap)
        first = _gkey(np.arange(1_500))
        ids = h.assign(first)
        assert np.array_equal(_u64(d.assign(_dev(first, gpu))), ids)
        vid = rng.permutation(ids.astype(np.int64))[:700]
        assert int(d.reclaim_device(_flags(cap, vid, gpu)).item()) == h.reclaim(vid.tolist()) == 700
        assert len(h.free) == 700 and h.fresh == 1_500
        # 2,000 new keys, 600 of them twice, and 400 requests of surviving keys, shuffled
        new = _gkey(np.arange(10_000, 12_000))
        surv = np.array([k for k in first.tolist() if k in h.ids], dtype=np.uint64)
        batch = rng.permutation(np.concatenate([new, new[:600], surv[:400]]))
        assert batch.shape[0] == 3_000
        firsts = np.sort(np.unique(batch, return_index=True)[1][np.isin(np.unique(batch), new)])
        assert firsts[0] < 1_024 and (firsts >= 2_048).any() and ((firsts >= 1_024) & (firsts < 2_048)).any()
        want = h.assign(batch)
        assert np.array_equal(_u64(d.assign(_dev(batch, gpu))), want)
        assert h.free == [] and h.fresh == 1_500 + 1_300 and d.size() == h.size() == 2_800
        # room is 4,096 - 2,800 = 1,296: one key more overflows
        over = _gkey(np.arange(20_000, 21_297))
        want = h.assign(over)
        got = _u64(d.assign(_dev(over, gpu)))
        assert h.overflow and (want[:1_296] != np.uint64(NONE)).all() and want[1_296] == np.uint64(NONE)
        assert np.array_equal(got, want)
        assert _erange(d)
        # a reclaim stays in bounds, frees ids, drops the key that has no id; the error stays
        vid = h.lookup(over[:50]).astype(np.int64)
        assert int(d.reclaim_device(_flags(cap, vid, gpu)).item()) == h.reclaim(vid.tolist()) == 50
        assert _erange(d)
        probe = np.concatenate([over, batch[:200]])
        assert np.array_equal(_u64(d.lookup(_dev(probe, gpu))), h.lookup(probe))
        again = over[-3:][::-1]                            # the key without an id among them
        assert np.array_equal(_u64(d.assign(_dev(again, gpu))), h.assign(again))
        assert _erange(d)
        d.close()


def test_reclaim_survives_clock_step_back(engine_lib, gpu):
    """A's bucket is spent; A lapses and is reclaimed; B takes A's id and is decided at a
    timestamp before A's lapse.  Redis has no bucket named B: it starts full."""
    from distributedratelimiting.redis_amd import TokenBucketEngine
    from distributedratelimiting.redis_amd.cluster import DeviceDirectory, HostDirectory
    a, b = _gkey([1]), _gkey([2])
    with _side_stream(gpu):
        d = DeviceDirectory(16, device=0)
        h = HostDirectory(16)
        eng = TokenBucketEngine(16, 5, 2, 10_000_000, device=0)
        ida = d.assign(_dev(a, gpu))
        assert np.array_equal(_u64(ida), h.assign(a))
        g, r = _decide(eng, ida, [5], [T0], gpu)
        assert g.tolist() == [1] and r.tolist() == [0]
        assert d.reclaim(eng, T0 + 10_000_000) == h.reclaim(h.lookup(a).tolist()) == 1
        idb = d.assign(_dev(b, gpu))
        assert np.array_equal(_u64(idb), h.assign(b)) and _u64(idb)[0] == _u64(ida)[0]
        g, r = _decide(eng, idb, [5], [T0 + 1_000_000], gpu)     # 1 s after A's grant: A would hold 2 tokens
        assert g.tolist() == [1] and r.tolist() == [0]
        eng.close()
        d.close()


def test_keep_list(engine_lib, gpu):
    """Ids of an assign whose engine batch is not submitted yet have no row: they are dead
    unless the caller names them, and go with the next reclaim that does not.  An id given
    twice and ids >= capacity in the list change nothing."""
    from distributedratelimiting.redis_amd import TokenBucketEngine
    from distributedratelimiting.redis_amd.cluster import DeviceDirectory, HostDirectory
    cap = 64
    keys = _gkey([10, 11, 12, 13])
    with _side_stream(gpu):
        d = DeviceDirectory(cap, device=0)
        h = HostDirectory(cap)
        eng = TokenBucketEngine(cap, 5, 2, 10_000_000, device=0)
        ids = d.assign(_dev(keys, gpu))
        hid = h.assign(keys)
        assert np.array_equal(_u64(ids), hid)
        _decide(eng, ids[:2], [1, 1], [T0, T0], gpu)
        # keys 0 and 1 are alive, 2 and 3 have no row but are kept
        keep = [int(hid[2]), int(hid[3]), int(hid[2]), cap, cap + 5, 2**40]
        assert d.reclaim(eng, T0 + 1_000_000, keep_ids=keep) == h.reclaim(hid[2:].tolist(), keep_ids=keep) == 0
        assert np.array_equal(_u64(d.lookup(_dev(keys, gpu))), hid) and d.size() == 4
        assert _u64(d.keys_of(ids)).tolist() == keys.tolist()
        # everything is dead by now; key 2 alone is kept
        keep = [int(hid[2]), 2**63, int(hid[2])]
        assert d.reclaim(eng, T0 + 10_000_000, keep_ids=keep) == h.reclaim(hid.tolist(), keep_ids=keep) == 3
        assert _u64(d.lookup(_dev(keys, gpu))).tolist() == [NONE, NONE, int(hid[2]), NONE]
        assert _u64(d.keys_of(ids)).tolist() == [NONE, NONE, int(keys[2]), NONE] and d.size() == 1
        assert d.reclaim(eng, T0 + 10_000_000) == h.reclaim(hid.tolist()) == 1
        assert d.size() == h.size() == 0
        # the freed ids come back in the mirror's order
        more = np.concatenate([keys[::-1], _gkey([14])])
        assert np.array_equal(_u64(d.assign(_dev(more, gpu))), h.assign(more))
        eng.close()
        d.close()


def test_reverse_lookup_after_reuse_and_snapshot(engine_lib, gpu, tmp_path):
    """The id -> key table exists before the reclaim: afterwards it shows the new keys of
    reused ids and nothing for ids that are not held; a snapshot saved then restores, behind
    a fresh directory, an engine that decides like the one that kept running."""
    import torch
    from distributedratelimiting.redis_amd import TokenBucketEngine, snapshot
    from distributedratelimiting.redis_amd.cluster import DeviceDirectory, HostDirectory
    cap = 256
    rng = np.random.default_rng(8)
    all_ids = torch.arange(cap, dtype=torch.int64, device=gpu)

    def inverse(h):
        inv = np.full(cap, NONE, dtype=np.uint64)
        for k, i in h.ids.items():
            inv[i] = k
        return inv

    with _side_stream(gpu):
        d = DeviceDirectory(cap, device=0)
        h = HostDirectory(cap)
        eng = TokenBucketEngine(cap, 5, 2, 10_000_000, device=0)
        assert (_u64(d.keys_of(all_ids)) == np.uint64(NONE)).all()
        keys = _gkey(np.arange(100))
        ids = d.assign(_dev(keys, gpu))
        assert np.array_equal(_u64(ids), h.assign(keys))
        assert np.array_equal(_u64(d.keys_of(all_ids)), inverse(h))
        _decide(eng, ids[:50], rng.integers(1, 4, 50), np.full(50, T0), gpu)
        _decide(eng, ids[50:], rng.integers(1, 4, 50), np.full(50, T0 + 4_000_000), gpu)
        assert d.reclaim(eng, T0 + 5_000_000) == h.reclaim(h.lookup(keys[:50]).tolist()) == 50
        assert np.array_equal(_u64(d.keys_of(all_ids)), inverse(h))
        new = _gkey(np.arange(500, 530))
        nid = d.assign(_dev(new, gpu))
        assert np.array_equal(_u64(nid), h.assign(new))
        assert set(_u64(nid).tolist()) < set(_u64(ids[:50]).tolist())      # 30 of the 50 freed ids
        _decide(eng, nid, rng.integers(1, 4, 30), np.full(30, T0 + 5_000_000), gpu)
        inv = inverse(h)
        assert np.array_equal(_u64(d.keys_of(all_ids)), inv)
        assert int((inv == np.uint64(NONE)).sum()) == cap - 80
        # save, restore behind a directory that has met other keys, decide one more batch
        path = tmp_path / "dir.npz"
        assert snapshot.save(path, eng, T0 + 5_500_000, d) == 80
        d2 = DeviceDirectory(cap, device=0)
        d2.assign(_dev(_gkey(np.arange(9_000, 9_040)), gpu))
        eng2 = TokenBucketEngine(cap, 5, 2, 10_000_000, device=0)
        assert snapshot.load([path], eng2, d2) == 80
        batch = rng.permutation(np.concatenate([keys, new, _gkey(np.arange(600, 620))] * 3))   # some keys run dry
        p = rng.integers(0, 4, batch.shape[0])
        ts = np.full(batch.shape[0], T0 + 6_000_000)
        ia, ib = d.assign(_dev(batch, gpu)), d2.assign(_dev(batch, gpu))
        assert np.array_equal(_u64(ia), h.assign(batch)) and not np.array_equal(_u64(ia), _u64(ib))
        ga, ra = _decide(eng, ia, p, ts, gpu)
        gb, rb = _decide(eng2, ib, p, ts, gpu)
        assert np.array_equal(ga, gb) and np.array_equal(ra, rb)
        assert 0 < int(ga.sum()) < ga.shape[0]
        for x in (eng, eng2, d, d2):
            x.close()


def test_queueing_kind_and_approximate_refused(engine_lib, gpu):
    """Queueing kind: a key with queued waits is never dead, whatever its row; once a refresh
    has granted them and a further TTL has passed it goes.  The approximate kind has no
    expiry: TBE_EINVAL, and the directory is as it was."""
    from distributedratelimiting.redis_amd import _capi
    from distributedratelimiting.redis_amd.cluster import DeviceDirectory, HostDirectory
    from distributedratelimiting.redis_amd.engine import ApproximateEngine, QueueingTokenBucketEngine
    cap = 64
    keys = _gkey([31, 32, 33, 34])
    with _side_stream(gpu):
        d = DeviceDirectory(cap, device=0)
        h = HostDirectory(cap)
        eng = QueueingTokenBucketEngine(cap, 5, 2, 10_000_000, queue_limit=4, device=0)
        ids = _u64(d.assign(_dev(keys, gpu)))
        assert np.array_equal(ids, h.assign(keys))
        # every key spends its bucket; keys 0 and 1 then queue a wait for 3 permits
        req = np.concatenate([ids, ids[:2]])
        st, rem, _ = eng.wait_batch(req, [5, 5, 5, 5, 3, 3], np.full(6, T0), 100)
        assert st.tolist() == [_capi.TBE_WAIT_GRANTED] * 4 + [_capi.TBE_WAIT_QUEUED] * 2
        # 10 s later every row has lapsed; the two keys with queued waits stay
        t1 = T0 + 10_000_000
        assert d.reclaim(eng, t1) == h.reclaim(ids[2:].tolist()) == 2
        assert np.array_equal(_u64(d.lookup(_dev(keys, gpu))), h.lookup(keys))
        assert _u64(d.lookup(_dev(keys, gpu))).tolist() == [int(ids[0]), int(ids[1]), NONE, NONE]
        k, rid, _ = eng.refresh(t1)                                   # grants both waits
        assert sorted(k.tolist()) == sorted(ids[:2].tolist()) and sorted(rid.tolist()) == [104, 105]
        assert d.reclaim(eng, t1 + 1_000_000) == 0 and d.size() == 2  # granted at t1: alive
        assert d.reclaim(eng, t1 + 4_000_000) == h.reclaim(ids[:2].tolist()) == 2
        assert d.size() == h.size() == 0
        # approximate kind
        again = d.assign(_dev(keys, gpu))
        assert np.array_equal(_u64(again), h.assign(keys))
        apx = ApproximateEngine(cap, 5, 2, 10_000_000, queue_limit=4, device=0)
        with pytest.raises(_capi.TbeError) as ei:
            d.reclaim(apx, t1 + 20_000_000)
        assert ei.value.status == _capi.TBE_EINVAL
        assert np.array_equal(_u64(d.lookup(_dev(keys, gpu))), h.lookup(keys)) and d.size() == 4
        assert np.array_equal(_u64(d.keys_of(again)), keys)
        for x in (apx, eng, d):
            x.close()


def test_device_form_on_a_side_stream(engine_lib, gpu):
    """expired_device -> reclaim_device -> assign on one stream with no host
    synchronisation in between: the stream's order alone carries the flags and the table."""
    import torch
    from distributedratelimiting.redis_amd import TokenBucketEngine
    from distributedratelimiting.redis_amd.cluster import DeviceDirectory, HostDirectory
    cap = 3_000
    with _side_stream(gpu):
        cur = torch.cuda.current_stream(gpu).cuda_stream
        d = DeviceDirectory(cap, device=0)
        h = HostDirectory(cap)
        eng = TokenBucketEngine(cap, 5, 2, 10_000_000, device=0)
        keys = _gkey(np.arange(2_500))
        want = h.assign(keys)
        ids = d.assign(_dev(keys, gpu))
        n = keys.shape[0]
        ones = torch.ones(n, dtype=torch.int32, device=gpu)
        g = torch.empty(n, dtype=torch.uint8, device=gpu)
        r = torch.empty(n, dtype=torch.int32, device=gpu)
        # every third key is used again 4 s later and stays alive; the others lapse
        eng.acquire_batch_device(ids, ones, torch.full((n,), T0, dtype=torch.int64, device=gpu), g, r, stream=cur)
        late = ids[::3].contiguous()
        m = late.numel()
        eng.acquire_batch_device(late, ones[:m], torch.full((m,), T0 + 4_000_000, dtype=torch.int64, device=gpu),
                                 g[:m], r[:m], stream=cur)
        more = _dev(np.concatenate([_gkey(np.arange(5_000, 6_000)), keys[:300]]), gpu)
        dead = torch.empty(cap, dtype=torch.uint8, device=gpu)
        eng.expired_device(T0 + 5_000_000, dead, clear=True, stream=cur)
        count = d.reclaim_device(dead)
        ids2 = d.assign(more)
        # only now does the host look
        gone = np.ones(n, dtype=bool)
        gone[::3] = False
        assert np.array_equal(_u64(ids), want)
        assert int(count.item()) == h.reclaim(want[gone].tolist()) == int(gone.sum())
        assert np.array_equal(_u64(ids2), h.assign(_u64(more)))
        assert d.size() == h.size()
        assert np.array_equal(_u64(d.lookup(_dev(keys, gpu))), h.lookup(keys))
        eng.close()
        d.close()
