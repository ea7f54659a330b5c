"""Approximate limit classes (tbe_create_approx_classes, the tbe_approx_*_classes
calls and tbe_set_class on the approximate kind in include/tbe.h): one engine holds several
differently configured ApproximateTokenBucket limiters.

Keys are independent, so the exact reference is one client model per class: a reference over
all n_keys per (client, class), fed only its class's requests in arrival order, synced only at
its class's epochs and compared on its class's keys only.  A reference numbers the requests it
is given 0, 1, ... from the batch's id_base; `ClassRefs` keeps the map from those ids to the
ids the engine gave the same requests (id_base + position in the whole batch).  Everything is
compared exactly."""
import numpy as np
import pytest

from oracle.semantics import (AP_FAILED, NEWEST_FIRST, OLDEST_FIRST, ApproxClient, ApproxGlobalTable,
                              approx_refresh_all, wrap32)

pytestmark = pytest.mark.gpu

S_US = 1_760_572_800 * 1_000_000
FAILED, GRANTED, QUEUED, REJECTED = 0, 1, 2, 3
ABSENT = np.iinfo(np.int64).min
ZERO_SLOTS = 4
# (TokenLimit, TokensPerPeriod, ReplenishmentPeriod ticks, QueueLimit, order); class 0 is the config's
BASE = [(20, 10, 10_000_000, 8, OLDEST_FIRST), (5, 2, 20_000_000, 3, NEWEST_FIRST),
        (16383, 1000, 10_000_000, 0, OLDEST_FIRST),            # forces 4-byte replies
        (3, 1, 5_000_000, 16, NEWEST_FIRST)]


def _engine(n_keys, classes=BASE, **kw):
    from distributedratelimiting.redis_amd import ApproximateEngine
    c0 = classes[0]
    return ApproximateEngine(n_keys, c0[0], c0[1], c0[2], c0[3], c0[4], device=0, zero_wait_slots=ZERO_SLOTS,
                             approx_classes=classes[1:], **kw)


def _set_by_mod(eng, n_keys, n_classes):
    cls = (np.arange(n_keys) % n_classes).astype(np.uint8)
    eng.set_class(np.arange(n_keys, dtype=np.uint64), cls)
    return cls


class ClassRefs:
    """refs[r][c]: oracle.cref.CApprox of client r with class c's options, over all n_keys."""

    def __init__(self, n_keys, classes, cls, n_clients=1):
        from oracle.cref import CApprox
        self.n_keys, self.classes, self.cls, self.n_clients = n_keys, classes, cls, n_clients
        self.refs = [[CApprox(n_keys, *c, zero_slots=ZERO_SLOTS) for c in classes] for _ in range(n_clients)]
        self.ids = [[{} for _ in classes] for _ in range(n_clients)]     # reference id -> engine id
        self.keys_of = [np.flatnonzero(cls == c) for c in range(len(classes))]
        self.seen = [set() for _ in classes]          # statuses per class
        self.evictions = [0] * len(classes)
        self.drained = [0] * len(classes)

    def acquire(self, r, keys, permits, wait, id_base):
        """(status, available, [(cause, evicted id)]) of the whole batch, as the engine reports them."""
        n = len(keys)
        status, avail, ev = np.empty(n, np.uint8), np.empty(n, np.int32), []
        kc = self.cls[keys.astype(np.int64)]
        for c, ref in enumerate(self.refs[r]):
            idx = np.flatnonzero(kc == c)
            if not idx.size:
                continue
            st, av, cause, ids = ref.acquire_batch(keys[idx], permits[idx], wait=wait, id_base=id_base)
            status[idx], avail[idx] = st, av
            m = self.ids[r][c]
            for j in np.flatnonzero(st == QUEUED).tolist():
                m[id_base + j] = id_base + int(idx[j])
            ev += [(int(idx[int(ca)]), m[int(i)]) for ca, i in zip(cause.tolist(), ids.tolist())]
            self.seen[c].update(st.tolist())
            self.evictions[c] += len(ids)
        return status, avail, sorted(ev)

    def sync(self, classes, ts_us, stagger_us):
        """One epoch of the given classes: per client the drain log (keys, ids, available) in
        (key, drain) order, with the engine's ids."""
        logs = [([], [], []) for _ in range(self.n_clients)]
        for c in classes:
            allc = np.concatenate([self.refs[r][c].collect() for r in range(self.n_clients)])
            for r in range(self.n_clients):
                k, i, rem = self.refs[r][c].sync(allc, self.n_clients, r, ts_us, stagger_us)
                assert np.all(self.cls[k.astype(np.int64)] == c)      # only its own keys ever queue
                logs[r][0].extend(k.tolist())
                logs[r][1].extend(self.ids[r][c][x] for x in i.tolist())
                logs[r][2].extend(rem.tolist())
                self.drained[c] += len(k)
        out = []
        for k, i, rem in logs:
            o = np.argsort(np.array(k, dtype=np.uint64), kind="stable")     # a key has one class: drain order kept
            out.append((np.array(k, np.uint64)[o], np.array(i, np.int64)[o], np.array(rem, np.int32)[o]))
        return out

    def state(self, r):
        """Per-key arrays of client r taken from each key's own class's reference."""
        out = None
        for c, ref in enumerate(self.refs[r]):
            e = ref.export()
            if out is None:
                out = {k: v.copy() for k, v in e.items()}
            ks = self.keys_of[c]
            for k in out:
                out[k][ks] = e[k][ks]
        return out

    def queue_of(self, r, key):
        c = int(self.cls[key])
        return [(self.ids[r][c][i], p) for i, p in self.refs[r][c].queue_of(key)]

    def nonvacuous(self, wait):
        for c, opt in enumerate(self.classes):
            want = {FAILED, GRANTED, QUEUED, REJECTED} if wait else {FAILED, GRANTED, REJECTED}
            assert self.seen[c] >= want, (c, self.seen[c])
            if wait:
                assert self.drained[c] >= 1, c
                if opt[4] == NEWEST_FIRST:
                    assert self.evictions[c] >= 1, c


def _draw(rng, n_keys, n, cls, classes, hot):
    """Keys (half of them from `hot` when given) and permits drawn from the choices of each
    key's own class, which end at its REJECTED boundary TokenLimit + 1."""
    keys = rng.integers(0, n_keys, n)
    if hot is not None:
        pick = rng.random(n) < 0.5
        keys[pick] = rng.choice(hot, int(pick.sum()))
    lim = np.array([c[0] for c in classes])[cls[keys]]
    which = rng.integers(0, 8, n)
    permits = np.select([which == 0, which <= 2, which == 3, which == 4, which == 5, which == 6],
                        [0, 1, 2, 3, np.maximum(1, lim // 2), lim], lim + 1)
    return keys.astype(np.uint64), permits.astype(np.int32)


def _check_state(eng, refs, r, keys):
    """local_state of the sampled keys and the whole tier's bit patterns against the references."""
    want = refs.state(r)
    for k in keys:
        got = eng.local_state(int(k))
        assert got == (int(want["local"][k]), int(want["global"][k]), float(want["est"][k]),
                       int(want["available"][k]), int(want["queued"][k])), (k, got)
    v, p, t = eng.export_global()
    assert np.array_equal(t, want["t_us"])
    live = t != ABSENT
    assert np.array_equal(v[live].view(np.uint64), want["v"][live].view(np.uint64))
    assert np.array_equal(p[live].view(np.uint64), want["p"][live].view(np.uint64))


# ---------------------------------------------------------------- 1. fold and sync, smallest shapes
@pytest.mark.parametrize("n_clients", [1, 3])
@pytest.mark.parametrize("wait", [True, False])
@pytest.mark.parametrize("n_keys", [300, 50_000])
def test_fold_and_sync(engine_lib, gpu, n_keys, wait, n_clients):
    """300 keys: one pass, dense 16-row buckets; 50,000 keys: two passes, 64-row buckets of
    about 5 requests (sparse: rows gathered).  4,000 requests per client and epoch, 6 epochs,
    every class synced at every epoch (the unmasked calls)."""
    import torch
    n, epochs = 4000, 6
    rng = np.random.default_rng(20_000 + n_keys + 10 * n_clients + wait)
    cls = (np.arange(n_keys) % 4).astype(np.uint8)
    hot = rng.choice(n_keys, 200, replace=False) if n_keys > 300 else None
    refs = ClassRefs(n_keys, BASE, cls, n_clients)
    # the whole run on the references first: the conditions that keep the case from being vacuous
    plan, rid = [], 0
    for epoch in range(epochs):
        batches = []
        for r in range(n_clients):
            keys, permits = _draw(rng, n_keys, n, cls, BASE, hot)
            batches.append((keys, permits, rid, refs.acquire(r, keys, permits, wait, rid)))
            rid += n
        ts = S_US + epoch * 1_000_000 + int(rng.integers(0, 300_000))
        stagger = 1_000_000 // n_clients
        logs = refs.sync(range(4), ts, stagger)
        plan.append((batches, ts, stagger, logs, [refs.state(r) for r in range(n_clients)]))
    refs.nonvacuous(wait)

    engines = [_engine(n_keys) for _ in range(n_clients)]
    lay = engines[0].layout()
    # the engine's own bucket size: the first batch has a dense bucket (>= R/8 requests) at 300 keys
    # and a sparse one at 50,000 (empty buckets count)
    r_bits = lay["r_bits"]
    n_buckets = (n_keys + (1 << r_bits) - 1) >> r_bits
    per_bucket = np.bincount(plan[0][0][0][0].astype(np.int64) >> r_bits, minlength=n_buckets)
    assert len(per_bucket) == n_buckets
    if n_keys == 300:
        assert per_bucket.max() >= (1 << r_bits) // 8
    else:
        assert per_bucket.min() < (1 << r_bits) // 8
    assert not lay["packed"] and not lay["medium"] and lay["passes"] == (1 if n_keys == 300 else 2)
    for e in engines:
        e.set_class(np.arange(n_keys, dtype=np.uint64), cls)
    counts = [torch.zeros(n_keys, dtype=torch.int32, device=gpu) for _ in range(n_clients)]
    torch.cuda.synchronize()
    sample = range(0, n_keys, 7 if n_keys == 300 else 613)
    for batches, ts, stagger, logs, states in plan:
        for r, (keys, permits, base, (st, av, ev)) in enumerate(batches):
            g_st, g_av, (cause, ids) = engines[r].acquire_batch(keys, permits, wait=wait, id_base=base)
            assert np.array_equal(g_st, st)
            assert np.array_equal(g_av, av)
            assert list(zip(cause.tolist(), ids.tolist())) == ev
        for r in range(n_clients):
            engines[r].collect(counts[r])
        allc = torch.cat(counts)                      # all_counts keeps its [n_clients][n_keys] layout
        torch.cuda.synchronize()
        for r in range(n_clients):
            got = engines[r].sync(allc, n_clients, r, ts, stagger)
            for a, b in zip(got, logs[r]):
                assert np.array_equal(a, b)
        for r in range(n_clients):
            want = states[r]
            for k in sample:
                assert engines[r].local_state(k) == (int(want["local"][k]), int(want["global"][k]),
                                                     float(want["est"][k]), int(want["available"][k]),
                                                     int(want["queued"][k])), (r, k)
            v, p, t = engines[r].export_global()
            assert np.array_equal(t, want["t_us"])
            live = t != ABSENT
            assert live.all()                             # every class was synced
            assert np.array_equal(v.view(np.uint64), want["v"].view(np.uint64))
            assert np.array_equal(p.view(np.uint64), want["p"].view(np.uint64))
    for e in engines:
        e.close()


# ---------------------------------------------------------------- 2. masked epochs
def _full_state(eng, keys):
    """Everything the engine keeps of `keys`: local_state, the queue's entries, the tier rows' bits."""
    v, p, t = eng.export_global()
    out = {}
    for k in keys:
        k = int(k)
        ls = eng.local_state(k)
        est_bits = np.float64(ls[2]).view(np.uint64)
        out[k] = (ls[0], ls[1], int(est_bits), ls[3], ls[4], tuple(eng.queue_of(k)) if ls[4] else (),
                  int(v[k:k + 1].view(np.uint64)[0]), int(p[k:k + 1].view(np.uint64)[0]), int(t[k]))
    return out


@pytest.mark.parametrize("fused", [True, False])
def test_masked_epochs(engine_lib, gpu, fused):
    """Epochs 0.5 s apart: the 0.5 s class is synced at every epoch, the 1 s classes at every
    second, the 2 s class at every fourth.  A masked call leaves every key of an unmasked
    class bit for bit as it was and collects 0 for it.  fused: refresh(classes=) against
    collect(classes=) + sync(classes=).
    The estimate (A:443) is ReplenishmentPeriod over the measured interval between syncs,
    field p of the tier row, an average that starts at 0 and takes a fifth of each new interval
    (A:262).  After the 8 epochs with requests the 2 s class has synced twice (p = 0.4 s,
    estimate 5, engine and reference agree); the schedule then runs on without requests until
    it has synced 8 times, p = 2 (1 - 0.8^7) = 1.58 s, and its estimate is 1 -- where syncing it
    at every epoch with the others would leave it at 4."""
    import torch
    n_keys, n = 300, 4000
    rng = np.random.default_rng(777 + fused)
    cls = (np.arange(n_keys) % 4).astype(np.uint8)
    refs = ClassRefs(n_keys, BASE, cls)
    eng = _engine(n_keys)
    eng.set_class(np.arange(n_keys, dtype=np.uint64), cls)
    d_counts = torch.full((n_keys,), -7, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    rid = 0
    for epoch in range(32):
        if epoch < 8:
            keys, permits = _draw(rng, n_keys, n, cls, BASE, None)
            st, av, ev = refs.acquire(0, keys, permits, True, rid)
            g_st, g_av, (cause, ids) = eng.acquire_batch(keys, permits, wait=True, id_base=rid)
            assert np.array_equal(g_st, st) and np.array_equal(g_av, av)
            assert list(zip(cause.tolist(), ids.tolist())) == ev
            rid += n
        due = [3] + ([0, 2] if epoch % 2 == 1 else []) + ([1] if epoch % 4 == 3 else [])
        ts = S_US + epoch * 500_000
        others = np.flatnonzero(~np.isin(cls, due))
        before = _full_state(eng, others) if epoch < 8 else None
        want = refs.sync(due, ts, 0)[0]
        if fused:
            got = eng.refresh(ts, classes=due)
        else:
            eng.collect(d_counts, classes=due)
            torch.cuda.synchronize()
            c = d_counts.cpu().numpy()
            assert not c[others].any()
            got = eng.sync(d_counts, 1, 0, ts, 0, classes=due)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        if epoch < 8:
            assert _full_state(eng, others) == before
            _check_state(eng, refs, 0, range(0, n_keys, 3))
        if epoch == 7:
            refs.nonvacuous(True)
            assert eng.local_state(1)[2] == refs.state(0)["est"][1] == 5.0      # two syncs of the 2 s class
    state = refs.state(0)
    _check_state(eng, refs, 0, range(n_keys))
    for k in range(n_keys):
        assert state["est"][k] == 1.0, (k, cls[k], state["est"][k])
    # the same 32 epochs with every class synced each time: the 2 s class is estimated at 4 clients
    naive = _engine(n_keys)
    naive.set_class(np.arange(n_keys, dtype=np.uint64), cls)
    for epoch in range(32):
        naive.refresh(S_US + epoch * 500_000)
    assert [naive.local_state(k)[2] for k in range(4)] == [2.0, 4.0, 2.0, 1.0]
    naive.close()
    eng.close()


# ---------------------------------------------------------------- 3. more than 16 classes, a long ring
def test_twenty_classes_and_long_ring(engine_lib, gpu):
    """20 classes over 64 keys; class 17 has QueueLimit 2,000 (a ring of 2,004 entries, every
    other class uses the first few slots of the same stride) and its keys queue, drain and
    queue again until their rings wrap."""
    n_keys = 64
    classes = [(4 + c, 1 + c % 3, 10_000_000 * (1 + c % 2), c % 5, c % 2) for c in range(20)]
    classes[17] = (6, 3, 10_000_000, 2000, OLDEST_FIRST)
    rng = np.random.default_rng(1717)
    cls = (np.arange(n_keys) % 20).astype(np.uint8)
    refs = ClassRefs(n_keys, classes, cls)
    eng = _engine(n_keys, classes)
    assert eng.approx_classes() == classes and eng.classes() == [c[:3] for c in classes]
    eng.set_class(np.arange(n_keys, dtype=np.uint64), cls)
    assert np.array_equal(eng.get_class(np.arange(n_keys, dtype=np.uint64)), cls)
    long_keys = np.flatnonzero(cls == 17)
    rid, drained = 0, np.zeros(n_keys, np.int64)
    for epoch in range(8):
        keys = np.concatenate([rng.integers(0, n_keys, 1500), rng.choice(long_keys, 2500)]).astype(np.uint64)
        rng.shuffle(keys)
        lim = np.array([c[0] for c in classes])[cls[keys.astype(np.int64)]]
        which = rng.integers(0, 6, keys.size)        # 0..3, TokenLimit, and the REJECTED boundary
        permits = np.where(which < 4, np.minimum(which, lim), lim + which - 4).astype(np.int32)
        on_long = np.isin(keys, long_keys)           # one permit each (a tenth: none), so that 2,000 entries fit
        permits[on_long] = (rng.random(int(on_long.sum())) < 0.9).astype(np.int32)
        st, av, ev = refs.acquire(0, keys, permits, True, rid)
        g_st, g_av, (cause, ids) = eng.acquire_batch(keys, permits, wait=True, id_base=rid)
        assert np.array_equal(g_st, st) and np.array_equal(g_av, av)
        assert list(zip(cause.tolist(), ids.tolist())) == ev
        for k in long_keys[:2].tolist() + [3, 16]:
            assert eng.queue_of(k) == refs.queue_of(0, k)
        rid += keys.size
        ts = S_US + epoch * 3_000_000
        got, want = eng.refresh(ts), refs.sync(range(20), ts, 0)[0]
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        np.add.at(drained, want[0].astype(np.int64), 1)
        _check_state(eng, refs, 0, range(n_keys))
    # OldestFirst without evictions or cancels: a key's head has advanced by its drained entries, so
    # its newest entry was written at slot (drained + queued - 1) mod 2,004: past the ring's end
    for k in long_keys.tolist():
        assert drained[k] + len(refs.queue_of(0, k)) > 2004, (k, drained[k])
    assert all(refs.seen[c] >= ({GRANTED, QUEUED} if c == 17 else {GRANTED, REJECTED}) for c in range(20))
    eng.close()


# ---------------------------------------------------------------- 4. RetryAfter per class
def _retry_ticks(client, key, p):
    """.NET ticks of A:390-395 on the key's current state with its class's TokenLimit and fill
    rate (int32 wrap, two f64 multiplies, truncation)."""
    s = client.st(key)
    deficit = max(0, wrap32(s.global_ + s.local + p + s.qcount - client.token_limit))
    t = (float(deficit) * client.decay_rate) * 1e7
    return 2 ** 63 - 1 if t >= 2.0 ** 63 else int(t)


@pytest.mark.parametrize("n_keys", [300, 50_000])
def test_retry_after_per_class(engine_lib, gpu, n_keys):
    """Both *_retry forms against the formula evaluated on the Python client model of the
    key's class, FAILED paths of every class present, device form equal to host form."""
    import torch
    n = 3000
    rng = np.random.default_rng(4242 + n_keys)
    cls = (np.arange(n_keys) % 4).astype(np.uint8)
    hot = rng.choice(n_keys, 120, replace=False) if n_keys > 300 else None
    clients = [ApproxClient(*c, zero_slots=ZERO_SLOTS) for c in BASE]
    tables = [ApproxGlobalTable(c.decay_rate) for c in clients]
    eng, twin = _engine(n_keys), _engine(n_keys)
    for e in (eng, twin):
        e.set_class(np.arange(n_keys, dtype=np.uint64), cls)
    failed_of = [0] * 4
    distinct = [set() for _ in range(4)]
    rid = 0
    for epoch in range(3):
        wait = epoch != 1
        keys, permits = _draw(rng, n_keys, n, cls, BASE, hot)
        exp_st, exp_ticks = [], []
        for i, (k, p) in enumerate(zip(keys.tolist(), permits.tolist())):
            c = int(cls[k])
            status = clients[c].wait(k, p, rid + i)[0] if wait else clients[c].acquire(k, p)
            exp_st.append(status)
            exp_ticks.append(_retry_ticks(clients[c], k, p) if status == AP_FAILED else -1)
            if status == AP_FAILED:
                failed_of[c] += 1
                distinct[c].add(exp_ticks[-1])
        st, av, _, ticks = eng.acquire_batch(keys, permits, wait=wait, id_base=rid, retry_after=True)
        assert st.tolist() == exp_st
        assert ticks.tolist() == exp_ticks
        d = [torch.from_numpy(x).to(gpu) for x in (keys.view(np.int64), permits)]
        d_st = torch.empty(n, dtype=torch.uint8, device=gpu)
        d_av = torch.empty(n, dtype=torch.int32, device=gpu)
        d_t = torch.empty(n, dtype=torch.int64, device=gpu)
        twin.acquire_batch_device(d[0], d[1], d_st, d_av, wait=wait, id_base=rid, d_retry_after=d_t)
        twin.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(d_st.cpu().numpy(), st) and np.array_equal(d_av.cpu().numpy(), av)
        assert np.array_equal(d_t.cpu().numpy(), ticks)
        rid += n
        ts = S_US + epoch * 700_000
        for c in range(4):                             # every key of the class, as the engine syncs them
            approx_refresh_all([clients[c]], tables[c], ts, 0, range(c, n_keys, 4))
        eng.refresh(ts)
        twin.refresh(ts)
    assert all(f > 0 for f in failed_of), failed_of
    # the classes' rates differ (10, 1, 1000, 2 per second): a non-zero deficit d gives d * rate * 1e7 ticks
    assert all(len(s) >= 2 for s in distinct), distinct
    eng.close()
    twin.close()


# ---------------------------------------------------------------- 5. class changes
def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else a.dtype)).to(gpu)


@pytest.mark.parametrize("device_form", [False, True])
def test_class_changes(engine_lib, gpu, device_form):
    from distributedratelimiting.redis_amd import TbeError
    n_keys = 40
    eng = _engine(n_keys)
    ids = np.arange(n_keys, dtype=np.uint64)
    cls = _set_by_mod(eng, n_keys, 4)
    # key 2 (class 2) leases 7 and its class alone is synced: a present tier row {v = 7}.  (A
    # first sync measures a period of 0 and so an infinite estimate, A:443: the class-0 keys below
    # keep their untouched caps because the sync is masked.)
    st, _, _ = eng.acquire_batch([2], [7], wait=True, id_base=50)
    assert st.tolist() == [GRANTED]
    eng.refresh(S_US, classes=[2])
    assert eng.local_state(2)[:2] == (0, 7)
    # class 0 (TokenLimit 20, QueueLimit 8).  key 4: 20 leased, one entry of 5 queued; key 8: a zero-permit registration only; key 16:
    # 3 leased and not synced
    st, _, _ = eng.acquire_batch([4, 4, 8, 8, 16], [20, 5, 20, 0, 3], wait=True, id_base=100)
    assert st.tolist() == [GRANTED, QUEUED, GRANTED, QUEUED, GRANTED]
    assert [eng.local_state(k)[4] for k in (4, 8, 16)] == [1, 1, 0] and eng.local_state(16)[0] == 3
    tier = [x.copy() for x in eng.export_global()]
    assert np.array_equal(np.flatnonzero(tier[2] != ABSENT), np.flatnonzero(cls == 2))

    def set_class(i, c):
        i, c = np.asarray(i, np.uint64), np.asarray(c, np.uint8)
        if device_form:
            eng.set_class_device(_dev(i, gpu), _dev(c, gpu))
            eng.synchronize()
        else:
            eng.set_class(i, c)

    # void calls: a queued entry, a zero-permit registration only, an id or a class out of range
    for bad_ids, bad_cls in (([2, 4], [1, 1]), ([8, 2], [3, 1]), ([2, n_keys], [1, 1]), ([2, 13], [1, 4])):
        before = _full_state(eng, range(n_keys))
        with pytest.raises(TbeError) as ei:
            set_class(bad_ids, bad_cls)
        assert ei.value.status == 1                     # TBE_EINVAL, or the sticky error at synchronize
        assert np.array_equal(eng.get_class(ids), cls)  # nothing written, the other id of the call included
        assert _full_state(eng, range(n_keys)) == before
    # after the voids the engine still decides correctly: key 16 (class 0) has 20 - 3 = 17 left
    st, av, _ = eng.acquire_batch([16, 16], [18, 17], wait=False)
    assert st.tolist() == [FAILED, GRANTED] and av.tolist() == [17, 0]
    # keys without queues to class 1 (TokenLimit 5): a fresh limiter's client side over the same tier rows
    set_class([2, 16], [1, 1])
    cls[[2, 16]] = 1
    assert np.array_equal(eng.get_class(ids), cls)
    assert eng.local_state(2) == (0, 0, 1.0, 5, 0)     # global 7 and est inf went with the old limiter
    assert eng.local_state(16) == (0, 0, 1.0, 5, 0)    # and so did the 20 permits never synced
    for a, b in zip(eng.export_global(), tier):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    st, av, _ = eng.acquire_batch([2, 2, 2], [6, 5, 1], wait=False)
    assert st.tolist() == [REJECTED, GRANTED, FAILED] and av.tolist() == [-1, 0, 0]
    # the key's next sync runs with class 1's options over the kept row {v = 7}: decay 1/s over
    # 0.1 s, then + 5; period 2 s over the measured 0.02 s
    eng.refresh(S_US + 100_000, classes=[1])
    assert eng.local_state(2) == (0, 11, 100.0, 0, 0)
    eng.close()


# ---------------------------------------------------------------- 6. maintenance by class
def _maintenance_plan():
    """The reference side of test_maintenance_by_class, as a list of steps to replay on the engine.
    Keys [0, 200) are busy, keys [200, 260) lease one permit before the first sync and nothing
    after, keys [260, 300) are never used.  Syncs are 0.4 s apart, so at the second one a light
    key's row has decayed to 0 in the fast classes (10 and 1000 tokens per second) and to 0.6
    and 0.2 in the slow ones (1 and 2 per second), with a global score of 0 everywhere: whether
    it is idle 50 ms later depends on its class's decay rate alone.
    The first sync measures a period of 0, an infinite estimate and so a cap of 0 (A:443, A:37):
    the second batch queues on most busy keys of every class -- zero-permit registrations in
    class 2, whose QueueLimit is 0 -- which is where queue_of and cancel are checked."""
    from distributedratelimiting.redis_amd import fill_rate, snapshot
    n_keys, n = 300, 4000
    rng = np.random.default_rng(606)
    cls = (np.arange(n_keys) % 4).astype(np.uint8)
    refs = ClassRefs(n_keys, BASE, cls)
    ok, failed = np.zeros(n_keys, np.uint64), np.zeros(n_keys, np.uint64)
    steps, rid = [], 0

    def full(keys):
        state = refs.state(0)
        return {int(k): (int(state["local"][k]), int(state["global"][k]), float(state["est"][k]),
                         int(state["available"][k]), int(state["queued"][k])) for k in keys}

    for epoch in range(3):
        keys, permits = _draw(rng, 200, n, cls, BASE, None)
        if epoch == 0:
            keys = np.concatenate([keys, np.arange(200, 260, dtype=np.uint64)])
            permits = np.concatenate([permits, np.ones(60, np.int32)])
        st, av, ev = refs.acquire(0, keys, permits, True, rid)
        ki = keys.astype(np.int64)
        np.add.at(ok, ki[st == GRANTED], 1)
        np.add.at(failed, ki[st == FAILED], 1)
        np.add.at(failed, ki[[c for c, _ in ev]], 1)                       # an eviction fails the evicted lease
        steps.append(("batch", keys, permits, rid, st, av, ev))
        rid += len(keys)
        if epoch == 1:
            state = refs.state(0)
            qk = [int(k) for c in range(4) for k in np.flatnonzero((state["queued"] > 0) & (cls == c))[:5]]
            assert {int(cls[k]) for k in qk} == {0, 1, 2, 3}
            steps.append(("queues", {k: refs.queue_of(0, k) for k in qk}))
            # the oldest entry of each of those keys, and an id that is not queued
            ck = [k for k in qk for _ in range(2)]
            ci = [refs.queue_of(0, k)[0][0] if j == 0 else 1 << 40 for k in qk for j in range(2)]
            for k in qk:                               # the reference cancels by its own id of the same entry
                ref = refs.refs[0][int(cls[k])]
                assert ref.cancel([k], [ref.queue_of(k)[0][0]]).tolist() == [1]
            steps.append(("cancel", ck, ci, [1, 0] * len(qk)))
            steps.append(("queues", {k: refs.queue_of(0, k) for k in qk}))
            steps.append(("state", full(qk)))
        ts = S_US + epoch * 400_000
        log = refs.sync(range(4), ts, 0)[0]
        np.add.at(ok, log[0].astype(np.int64), 1)
        steps.append(("sync", ts, log))
        if epoch == 1:
            state = refs.state(0)
            rates = [fill_rate(c[1], c[2]) for c in BASE]
            rule = [snapshot.approx_idle_rows(state["local"], state["global"], state["queued"], state["v"],
                                              state["t_us"], ts + 50_000, rates[c]) for c in range(4)]
            want_idle = np.select([cls == c for c in range(4)], rule)
            # not vacuous: idle and busy keys in every class, and class 0's rate alone would flag other keys
            for c in range(4):
                assert 0 < want_idle[cls == c].sum() < (cls == c).sum()
            assert (rule[0] != want_idle).any() and not want_idle[200:260][cls[200:260] == 1].any()
            assert want_idle[200:260][cls[200:260] == 0].all()
            steps.append(("idle", ts + 50_000, want_idle))
    steps.append(("stats", ok, failed))
    steps.append(("state", full(range(1, n_keys, 2))))
    return n_keys, cls, steps


def test_maintenance_by_class(engine_lib, gpu):
    """idle_device against snapshot.approx_idle_rows evaluated per class with that class's decay
    rate, reset_device to the class's TokenLimit, cancel, queue_of and the stats=True totals
    against the per-class references."""
    import torch
    n_keys, cls, steps = _maintenance_plan()
    eng = _engine(n_keys, stats=True)
    eng.set_class(np.arange(n_keys, dtype=np.uint64), cls)
    for step in steps:
        if step[0] == "batch":
            _, keys, permits, rid, st, av, ev = step
            g_st, g_av, (cause, ids) = eng.acquire_batch(keys, permits, wait=True, id_base=rid)
            assert np.array_equal(g_st, st) and np.array_equal(g_av, av)
            assert list(zip(cause.tolist(), ids.tolist())) == ev
        elif step[0] == "queues":
            for k, q in step[1].items():
                assert eng.queue_of(k) == q
        elif step[0] == "cancel":
            assert eng.cancel(step[1], step[2]).tolist() == step[3]
        elif step[0] == "state":
            for k, want in step[1].items():
                assert eng.local_state(k) == want, k
        elif step[0] == "sync":
            assert len(step[2][0]) <= eng.refresh_bound() <= n_keys * (16 + ZERO_SLOTS)
            for a, b in zip(eng.refresh(step[1]), step[2]):
                assert np.array_equal(a, b)
        elif step[0] == "idle":
            d_idle = torch.empty(n_keys, dtype=torch.uint8, device=gpu)
            eng.idle_device(step[1], d_idle)
            eng.synchronize()
            torch.cuda.synchronize()
            assert np.array_equal(d_idle.cpu().numpy().astype(bool), step[2])
        elif step[0] == "stats":
            got_ok, got_failed = eng.stats_export()
            assert np.array_equal(got_ok, step[1]) and np.array_equal(got_failed, step[2])
            assert eng.stats_totals() == (int(step[1].sum()), int(step[2].sum()))
    # reset every second key: cap == TokenLimit of its class, the class byte stays, the other rows too
    flags = (np.arange(n_keys) % 2 == 0).astype(np.uint8)
    eng.reset_device(torch.from_numpy(flags).to(gpu))
    eng.synchronize()
    assert np.array_equal(eng.get_class(np.arange(n_keys, dtype=np.uint64)), cls)
    for k in range(0, n_keys, 2):
        assert eng.local_state(k) == (0, 0, 1.0, BASE[int(cls[k])][0], 0)
    for k, want in steps[-1][1].items():
        assert eng.local_state(k) == want, k
    eng.close()


# ---------------------------------------------------------------- 7. refusals and layout
def test_refusals_layout_and_recreate(engine_lib, gpu, tmp_path):
    import torch
    from distributedratelimiting.redis_amd import ApproximateEngine, TbeError, snapshot
    n = 70_000
    eng = _engine(n)
    lay = eng.layout()
    assert not lay["packed"] and not lay["narrow"] and not lay["medium"]      # class 2: TokenLimit 16383
    assert eng.approx_classes() == BASE and eng.classes() == [c[:3] for c in BASE]
    small = [c for c in BASE if c[0] <= 16382]
    two = _engine(1000, small)
    assert not two.layout()["packed"] and two.layout()["medium"]              # two-byte replies
    two.close()
    with pytest.raises(ValueError, match="classes"):
        snapshot.save(str(tmp_path / "classed.npz"), eng, S_US)
    assert not (tmp_path / "classed.npz").exists()
    # a mask that names a class the engine does not have
    d_counts = torch.zeros(n, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    for call in (lambda: eng.refresh(S_US, classes=[0, 4]), lambda: eng.collect(d_counts, classes=[255]),
                 lambda: eng.sync(d_counts, 1, 0, S_US, 0, classes=[4])):
        with pytest.raises(TbeError) as ei:
            call()
        assert ei.value.status == 1
    eng.set_class(np.arange(n, dtype=np.uint64), np.full(n, 3, dtype=np.uint8))
    eng.close()
    eng = _engine(n)                                   # most likely over the same device memory
    assert not eng.get_class(np.arange(n, dtype=np.uint64)).any()
    st, av, _ = eng.acquire_batch([5, n - 1, 5, 5, 5], [1, 1, 18, 8, 1], wait=True)   # class 0: TokenLimit 20,
    assert st.tolist() == [GRANTED, GRANTED, GRANTED, QUEUED, FAILED]                 # QueueLimit 8, OldestFirst
    assert av.tolist() == [19, 19, 1, 1, 1]
    eng.close()
    # a plain approximate engine: class 0 only, and the masked calls with and without bit 0
    plain = ApproximateEngine(100, 10, 1, 10_000_000, 4, 0, device=0)
    assert plain.approx_classes() == [(10, 1, 10_000_000, 4, 0)]
    plain.set_class([1, 2], [0, 0])
    assert plain.get_class([1, 2]).tolist() == [0, 0]
    with pytest.raises(TbeError):
        plain.set_class([1, 2], [0, 1])
    plain.acquire_batch([7], [4], wait=False)
    before = (plain.local_state(7), [x.copy() for x in plain.export_global()])
    d_c = torch.full((100,), 9, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    plain.collect(d_c, classes=[])
    torch.cuda.synchronize()
    assert not d_c.cpu().numpy().any()
    assert all(a.size == 0 for a in plain.refresh(S_US, classes=[]))
    assert plain.local_state(7) == before[0]
    assert all(np.array_equal(a, b) for a, b in zip(plain.export_global(), before[1]))
    with pytest.raises(TbeError):
        plain.refresh(S_US, classes=[1])
    plain.refresh(S_US, classes=[0])
    assert plain.local_state(7)[:2] == (0, 4)
    plain.close()
