"""Queueing limit classes (tbe_create_queue_classes in include/tbe.h): one
queueing engine, per-key {TokenLimit, fill rate, TTL, QueueLimit, order}.  Every comparison
is exact.

Reference: keys are independent, so one oracle.cref.CQueueingTokenBucket per class, each fed
its class's requests in arrival order, decides what the classed engine must decide.  The C
reference numbers a sub-batch's requests id_base + i, so each class keeps a growing array
that maps its reference ids to the engine's ids (id_base + index in the full batch)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ABSENT = np.iinfo(np.int64).min
FAILED, GRANTED, QUEUED, REJECTED = 0, 1, 2, 3
# (TokenLimit, TokensPerPeriod, ticks, QueueLimit, order)
QC = [(4, 1, 10_000_000, 16, 0), (2, 1, 30_000_000, 3, 1),
      (3, 1, 10_000_000, 0, 0), (6, 10, 10_000_000, 40, 1)]
T0 = 1_760_000_000_000_000


def _engine(n_keys, classes=QC, **kw):
    from distributedratelimiting.redis_amd import QueueingTokenBucketEngine
    c0 = classes[0]
    return QueueingTokenBucketEngine(n_keys, c0[0], c0[1], c0[2], c0[3], c0[4], device=0,
                                     classes=classes[1:], **kw)


def _mix_cls(n_keys, n_cls=4):
    from oracle import trace
    return (trace.mix64(np.arange(n_keys, dtype=np.uint64)) % np.uint64(n_cls)).astype(np.uint8)


def _set_all(eng, cls):
    ids = np.arange(len(cls), dtype=np.uint64)
    eng.set_class(ids, cls)
    assert np.array_equal(eng.get_class(ids), cls)


class _PerClass:
    """One CQueueingTokenBucket per class; every key stays in its class."""

    def __init__(self, n_keys, cls, classes=QC, threads=1):
        from distributedratelimiting.redis_amd import fill_rate
        from oracle import cref
        self.cls, self.threads = cls, threads
        self.refs = [cref.CQueueingTokenBucket(n_keys, c[0], fill_rate(c[1], c[2]), c[3], c[4]) for c in classes]
        self.ids = [np.empty(0, np.int64) for _ in classes]      # reference id -> engine id
        self.counts = np.zeros((len(classes), 4), np.int64)      # statuses per class
        self.evictions = np.zeros(len(classes), np.int64)
        self.drained = np.zeros(len(classes), np.int64)

    def wait(self, keys, permits, ts, id_base):
        n = len(keys)
        status = np.empty(n, np.uint8)
        rem = np.empty(n, np.int32)
        kc = self.cls[keys.astype(np.int64)]
        ev_c, ev_i = [], []
        for c, ref in enumerate(self.refs):
            m = kc == c
            if not m.any():
                continue
            at = np.flatnonzero(m)
            base = len(self.ids[c])
            self.ids[c] = np.concatenate([self.ids[c], id_base + at])
            s, r, cause, evid = ref.acquire_batch(keys[m], permits[m], ts[m], base, threads=self.threads)
            status[m], rem[m] = s, r
            ev_c.append(at[cause.astype(np.int64)])
            ev_i.append(self.ids[c][evid])
            self.counts[c] += np.bincount(s, minlength=4)
            self.evictions[c] += len(evid)
        ev_c, ev_i = np.concatenate(ev_c), np.concatenate(ev_i)
        o = np.lexsort((ev_i, ev_c))
        self.last_causes = ev_c[o].astype(np.int64)
        return status, rem, ev_c[o].astype(np.uint64), ev_i[o]

    def refresh(self, ts):
        ks, ids, rems = [], [], []
        for c, ref in enumerate(self.refs):
            k, i, r = ref.refresh(ts, threads=self.threads)       # (key, drain) order either way
            ks.append(k)
            ids.append(self.ids[c][i])
            rems.append(r)
            self.drained[c] += len(k)
        k, i, r = np.concatenate(ks), np.concatenate(ids), np.concatenate(rems)
        o = np.argsort(k, kind="stable")                          # classes hold disjoint keys
        self.last_drained_keys = k[o]
        return k[o], i[o], r[o]

    def queue_of(self, key):
        c = self.cls[key]
        return [(int(self.ids[c][i]), p) for i, p in self.refs[c].queue_of(key)]

    def cancel(self, keys, eng_ids):
        out = np.zeros(len(keys), np.uint8)
        for j, (k, i) in enumerate(zip(keys.tolist(), eng_ids.tolist())):
            c = self.cls[k]
            at = np.flatnonzero(self.ids[c] == i)
            out[j] = self.refs[c].cancel([k], [int(at[0])])[0] if len(at) else 0
        return out

    def state(self):
        v = np.empty(len(self.cls), np.float64)
        t = np.empty(len(self.cls), np.int64)
        for c, ref in enumerate(self.refs):
            vc, tc = ref.bucket_state()
            m = self.cls == c
            v[m], t[m] = vc[m], tc[m]
        return v, t


def _workload(rng, n_keys, n, t, hot_share=0.0):
    keys = rng.integers(0, n_keys, n).astype(np.uint64)
    if hot_share:
        keys[rng.random(n) < hot_share] = 1234
    permits = rng.choice(np.array([0, 1, 1, 2, 3, 5, 7], dtype=np.int32), n)
    ts = t + np.sort(rng.integers(0, 1000, n)).astype(np.int64)
    return keys, permits, ts


def _not_vacuous(ref, hot_share=0.0):
    """The issue's conditions, on the reference's outputs alone."""
    share = ref.counts / ref.counts.sum(axis=1, keepdims=True)
    print("status shares per class (FAILED, GRANTED, QUEUED, REJECTED):\n", np.round(share, 3))
    print("evictions", ref.evictions.tolist(), "drained", ref.drained.tolist())
    for c in (0, 1, 3):
        assert share[c, QUEUED] >= 0.25 and share[c, GRANTED] >= 0.20 and ref.drained[c] >= 500, c
    assert ref.counts[2, QUEUED] == 0 and share[2, FAILED] >= 0.20
    assert share[0, REJECTED] >= 0.20 and share[2, REJECTED] >= 0.20 and share[1, REJECTED] >= 0.35
    assert ref.evictions[1] >= 1000
    if hot_share >= 0.08:
        assert ref.evictions[3] >= 1000


def _same_state(eng, ref):
    v, t = eng.export_state()
    v_ref, t_ref = ref.state()
    assert np.array_equal(t, t_ref), f"{int((t != t_ref).sum())} keys differ in t_us"
    present = t_ref != ABSENT
    assert np.array_equal(v[present].view(np.uint64), v_ref[present].view(np.uint64))


def _dev(a, gpu):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(gpu)


def _host_round(eng, ref, keys, permits, ts, id_base, t_tick, tag):
    s, r, (ec, ei) = eng.wait_batch(keys, permits, ts, id_base)
    s_ref, r_ref, ec_ref, ei_ref = ref.wait(keys, permits, ts, id_base)
    assert np.array_equal(s, s_ref), f"status mismatch, {tag}"
    assert np.array_equal(r, r_ref), f"remaining mismatch, {tag}"
    assert np.array_equal(ec, ec_ref) and np.array_equal(ei, ei_ref), f"evictions mismatch, {tag}"
    lk_ref, li_ref, lr_ref = ref.refresh(t_tick)
    assert eng.refresh_bound() >= len(lk_ref)
    lk, li, lr = eng.refresh(t_tick)
    assert np.array_equal(lk, lk_ref) and np.array_equal(li, li_ref) and np.array_equal(lr, lr_ref), \
        f"refresh log mismatch, {tag}"
    return s, r


def _tick_round(eng, ref, keys, permits, ts, id_base, t_tick, gpu, tag):
    import torch
    n = len(keys)
    cap = int(eng.refresh_bound()) + n
    d_s = torch.empty(n, dtype=torch.uint8, device=gpu)
    d_r = torch.empty(n, dtype=torch.int32, device=gpu)
    d_ks = torch.empty(cap, dtype=torch.int64, device=gpu)
    d_id = torch.empty(cap, dtype=torch.int64, device=gpu)
    d_rem = torch.empty(cap, dtype=torch.int32, device=gpu)
    d_cnt = torch.zeros(1, dtype=torch.int32, device=gpu)
    dk, dp, dt = _dev(keys, gpu), _dev(permits, gpu), _dev(ts, gpu)
    torch.cuda.synchronize()
    eng.wait_batch_tick_device(dk, dp, dt, d_s, d_r, id_base, t_tick, d_ks, d_id, d_rem, d_cnt)
    eng.synchronize()
    s_ref, r_ref, ec_ref, ei_ref = ref.wait(keys, permits, ts, id_base)
    assert np.array_equal(d_s.cpu().numpy(), s_ref), f"status mismatch, {tag}"
    assert np.array_equal(d_r.cpu().numpy(), r_ref), f"remaining mismatch, {tag}"
    ec, ei = eng.evicted()
    assert np.array_equal(ec, ec_ref) and np.array_equal(ei, ei_ref), f"evictions mismatch, {tag}"
    lk_ref, li_ref, lr_ref = ref.refresh(t_tick)
    m = int(d_cnt.item())
    assert m == len(lk_ref), f"{m} grants logged, {len(lk_ref)} expected, {tag}"
    ks = d_ks[:m].cpu().numpy().view(np.uint64)
    o = np.argsort(ks, kind="stable")
    assert np.array_equal(ks[o] >> np.uint64(16), lk_ref), tag
    assert np.array_equal(d_id[:m].cpu().numpy()[o], li_ref) and np.array_equal(d_rem[:m].cpu().numpy()[o], lr_ref), tag


# ---------------------------------------------------------------- 1. the smoke shape
def test_smoke_shape(engine_lib, oracle_lib, gpu):
    from distributedratelimiting.redis_amd import QueueingTokenBucketEngine
    n_keys, n = 10_000, 50_000
    rng = np.random.default_rng(1)
    cls = _mix_cls(n_keys)
    eng = _engine(n_keys)
    assert eng.queue_classes() == QC and eng.classes() == [c[:3] for c in QC]
    _set_all(eng, cls)
    c0 = QC[0]
    plain = QueueingTokenBucketEngine(n_keys, c0[0], c0[1], c0[2], c0[3], c0[4], device=0)
    ref = _PerClass(n_keys, cls)
    t, differs = T0, False
    for b in range(3):
        keys, permits, ts = _workload(rng, n_keys, n, t)
        t += 2_000_000
        s, r = _host_round(eng, ref, keys, permits, ts, b * n, t, f"batch {b}")
        s0, r0, _ = plain.wait_batch(keys, permits, ts, b * n)
        plain.refresh(t)
        differs |= not (np.array_equal(s, s0) and np.array_equal(r, r0))
    _not_vacuous(ref)
    assert differs, "a class-0 engine gives the same replies: the classes decide nothing here"
    for k in rng.choice(n_keys, 200, replace=False).tolist():
        assert eng.queue_of(k) == ref.queue_of(k), k
    _same_state(eng, ref)
    plain.close()
    eng.close()


# ---------------------------------------------------------------- 2. paths of the fold
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("share", [0.0, 0.01, 0.08, 0.5])
def test_fold_paths(engine_lib, oracle_lib, gpu, share, fused):
    n_keys, n = 6_000, 40_000
    rng = np.random.default_rng(2)
    cls = _mix_cls(n_keys)
    assert cls[1234] == 3                              # NewestFirst, QueueLimit 40
    eng = _engine(n_keys)
    _set_all(eng, cls)
    ref = _PerClass(n_keys, cls)
    t = T0
    for b in range(3):
        keys, permits, ts = _workload(rng, n_keys, n, t, share)
        t += 2_000_000
        if fused:
            _tick_round(eng, ref, keys, permits, ts, b * n, t, gpu, f"batch {b}")
        else:
            _host_round(eng, ref, keys, permits, ts, b * n, t, f"batch {b}")
    _not_vacuous(ref, share)
    assert eng.queue_of(1234) == ref.queue_of(1234)
    _same_state(eng, ref)
    eng.close()


# ---------------------------------------------------------------- 3. full-R dense buckets
BIG = 3 * (1 << 20) - 5          # R = 2048, 1536 buckets, a short last bucket


def _dense_trace(rng, n, t_start):
    """Half of the requests in 64 buckets (the short last one among them; in half of those only
    rows 0..511), five keys with 300 requests each, one with 3,000, the rest uniform; two
    timestamp jumps of more than a second."""
    nb = (BIG + 2047) // 2048
    hot_b = np.concatenate([rng.choice(nb - 1, 63, replace=False), [nb - 1]]).astype(np.int64)
    m = n // 2
    b = hot_b[rng.integers(0, 64, m)]
    narrow = (np.searchsorted(np.sort(hot_b), b) % 2) == 0
    row = np.where(narrow, rng.integers(0, 512, m), rng.integers(0, 2048, m))
    dense = np.minimum(b * 2048 + row, BIG - 1)
    heavy = np.repeat(rng.integers(0, BIG, 5), 300)
    one = np.full(3_000, int(hot_b[7]) * 2048 + 77)
    rest = rng.integers(0, BIG, n - m - heavy.size - one.size)
    keys = np.concatenate([dense, heavy, one, rest]).astype(np.uint64)
    rng.shuffle(keys)
    permits = rng.choice(np.array([0, 1, 1, 2, 3, 5, 7], dtype=np.int32), n)
    step = rng.integers(0, 3, n).astype(np.int64)
    step[rng.choice(n, 2, replace=False)] += 1_500_000
    return keys, permits, t_start + np.cumsum(step)


def test_dense_full_r_fused_ticks(engine_lib, oracle_lib, gpu):
    rng = np.random.default_rng(20261)
    cls = _mix_cls(BIG)
    eng = _engine(BIG)
    assert eng.layout()["r_bits"] == 11 and BIG % 2048 != 0
    _set_all(eng, cls)
    ref = _PerClass(BIG, cls, threads=16)
    n, t = 1 << 20, T0
    for b in range(2):
        keys, permits, ts = _dense_trace(rng, n, t)
        t = int(ts[-1]) + 700_000
        _tick_round(eng, ref, keys, permits, ts, b * n, t, gpu, f"batch {b}")
    print("statuses per class:\n", ref.counts, "evictions", ref.evictions.tolist(), "drained", ref.drained.tolist())
    # (a quarter of the 16,000 narrow rows are class 1, QueueLimit 3, at ~16 requests a batch each)
    assert ref.drained.sum() > 10_000 and ref.evictions[1] > 1_000
    _same_state(eng, ref)
    last = BIG - 1
    for k in (last, last - 3, int(keys[0])):
        assert eng.queue_of(k) == ref.queue_of(k), k
    eng.close()


# ---------------------------------------------------------------- 4. > 16 classes, 64-bit headers
def test_many_classes_and_wide_headers(engine_lib, oracle_lib, gpu):
    n_keys, n = 3_000, 30_000
    classes = [QC[i % 4] for i in range(20)]
    classes[17] = (QC[1][0], QC[1][1], QC[1][2], 2000, QC[1][4])
    rng = np.random.default_rng(4)
    cls = _mix_cls(n_keys, 20)
    eng = _engine(n_keys, classes)
    assert not eng.layout()["queue_header_32"]                    # tbe_layout bit 9: QueueLimit 2000 > 1024
    assert eng.queue_classes() == classes
    _set_all(eng, cls)
    ref = _PerClass(n_keys, cls, classes)
    long_keys = np.flatnonzero(cls == 17)[:10]
    t, deepest = T0, 0
    for b in range(3):
        keys, permits, ts = _workload(rng, n_keys, n, t)
        at = rng.choice(n, 15_000, replace=False)      # ten class-17 keys, 1,500 one-permit requests each
        keys[at] = np.repeat(long_keys, 1_500).astype(np.uint64)
        permits[at] = 1
        t += 2_000_000
        _host_round(eng, ref, keys, permits, ts, b * n, t, f"batch {b}")
        deepest = max(deepest, max(len(ref.queue_of(int(k))) for k in long_keys))
    assert deepest > 1024, deepest
    for k in long_keys.tolist() + rng.choice(n_keys, 50, replace=False).tolist():
        assert eng.queue_of(k) == ref.queue_of(k), k
    _same_state(eng, ref)
    eng.close()


# ---------------------------------------------------------------- 5. attempt_batch
def test_attempt_interleaved_with_wait(engine_lib, gpu):
    from oracle import semantics as sem
    n_keys, n = 10_000, 5_000
    rng = np.random.default_rng(5)
    cls = _mix_cls(n_keys)
    tables = [sem.QueueingTokenBucketTable(sem.TokenBucketConfig.from_options(*c[:3]), c[3], c[4]) for c in QC]
    eng = _engine(n_keys)
    _set_all(eng, cls)
    t, blocked = T0, 0
    for b in range(3):
        # the waits land on few keys, so that the attempts below find queues
        keys, permits, ts = _workload(rng, 300, n, t)
        s, r, (ec, ei) = eng.wait_batch(keys, permits, ts, b * n)
        s_ref, r_ref, ev_ref = [], [], []
        for i, (k, p, x) in enumerate(zip(keys.tolist(), permits.tolist(), ts.tolist())):
            st, rem, ev = tables[cls[k]].acquire(k, p, x, b * n + i)
            s_ref.append(st)
            r_ref.append(rem)
            ev_ref += [(i, e) for e in ev]
        assert s.tolist() == s_ref and r.tolist() == r_ref, f"wait {b}"
        assert sorted(zip(ec.tolist(), ei.tolist())) == sorted(ev_ref), f"wait {b}"
        keys, permits, ts = _workload(rng, 600, n, t + 1_000)
        s, r = eng.attempt_batch(keys, permits, ts)
        a_ref = [tables[cls[k]].attempt(k, p, x) for k, p, x in zip(keys.tolist(), permits.tolist(), ts.tolist())]
        assert s.tolist() == [a[0] for a in a_ref] and r.tolist() == [a[1] for a in a_ref], f"attempt {b}"
        # OldestFirst keys with a queue fail without a script call (remaining -1)
        blocked += sum(1 for a, p in zip(a_ref, permits.tolist()) if a == (FAILED, -1) and p > 0)
        assert sorted(set(s.tolist())) == [FAILED, GRANTED, REJECTED]
        t += 2_000_000
        log_ref = sorted((rec for tb in tables for rec in tb.refresh(t)), key=lambda rec: rec[0])
        lk, li, lr = eng.refresh(t)
        assert list(zip(lk.tolist(), li.tolist(), lr.tolist())) == log_ref, f"refresh {b}"
    assert blocked > 100, blocked
    for k in range(0, 600, 7):
        assert eng.queue_of(k) == tables[cls[k]].queue_of(k), k
    eng.close()


# ---------------------------------------------------------------- 6. class changes
def test_class_changes(engine_lib, gpu):
    from distributedratelimiting.redis_amd import _capi
    from oracle import semantics as sem
    n_keys, n = 2_000, 4_000
    rng = np.random.default_rng(6)
    tables = [sem.QueueingTokenBucketTable(sem.TokenBucketConfig.from_options(*c[:3]), c[3], c[4]) for c in QC]
    for tb in tables[1:]:
        tb.tb.state = tables[0].tb.state               # one Redis, four limiters' scripts
    cls = _mix_cls(n_keys)
    eng = _engine(n_keys)
    _set_all(eng, cls)
    all_ids = np.arange(n_keys, dtype=np.uint64)
    t, moved, queued_seen = T0, 0, 0
    for b in range(5):
        keys, permits, ts = _workload(rng, n_keys, n, t)
        t += 2_000_000
        s, r, (ec, ei) = eng.wait_batch(keys, permits, ts, b * n)
        s_ref, r_ref, ev_ref = [], [], []
        for i, (k, p, x) in enumerate(zip(keys.tolist(), permits.tolist(), ts.tolist())):
            st, rem, ev = tables[cls[k]].acquire(k, p, x, b * n + i)
            s_ref.append(st)
            r_ref.append(rem)
            ev_ref += [(i, e) for e in ev]
        assert s.tolist() == s_ref and r.tolist() == r_ref, f"batch {b}"
        assert sorted(zip(ec.tolist(), ei.tolist())) == sorted(ev_ref), f"batch {b}"
        log_ref = sorted((rec for tb in tables for rec in tb.refresh(t)), key=lambda rec: rec[0])
        lk, li, lr = eng.refresh(t)
        assert list(zip(lk.tolist(), li.tolist(), lr.tolist())) == log_ref, f"refresh {b}"
        busy = np.array([bool(tables[cls[k]].queues.get(k)) for k in range(n_keys)])
        queued_seen += int(busy.sum())
        # a call that holds one key with a queued entry is void, in either form
        if busy.any():
            bad = np.array([int(np.flatnonzero(~busy)[0]), int(np.flatnonzero(busy)[0])], np.uint64)
            to = ((cls[bad.astype(np.int64)] + 1) % 4).astype(np.uint8)
            with pytest.raises(_capi.TbeError) as e1:
                eng.set_class(bad, to)
            assert e1.value.status == _capi.TBE_EINVAL
            eng.set_class_device(_dev(bad, gpu), _dev(to, gpu))
            with pytest.raises(_capi.TbeError) as e2:
                eng.synchronize()
            assert e2.value.status == _capi.TBE_EINVAL
            eng.synchronize()                          # the flag is cleared by the report
        for bad_ids, bad_cls in (([3, 5], [1, 4]), ([3, n_keys], [1, 1])):
            free = np.flatnonzero(~busy)[:2]
            bi = np.array([free[0], bad_ids[1] if bad_ids[1] == n_keys else free[1]], np.uint64)
            bc = np.array(bad_cls, np.uint8)
            with pytest.raises(_capi.TbeError):
                eng.set_class(bi, bc)
            eng.set_class_device(_dev(bi, gpu), _dev(bc, gpu))
            with pytest.raises(_capi.TbeError):
                eng.synchronize()
            eng.synchronize()
        assert np.array_equal(eng.get_class(all_ids), cls), "a void call changed a class"
        # half of the keys whose queue is empty move to another class
        free = np.flatnonzero(~busy)
        ids = rng.choice(free, len(free) // 2, replace=False).astype(np.uint64)
        new = ((cls[ids.astype(np.int64)] + rng.integers(1, 4, ids.size)) % 4).astype(np.uint8)
        if b % 2 == 0:
            eng.set_class(ids, new)
        else:
            eng.set_class_device(_dev(ids, gpu), _dev(new, gpu))
            eng.synchronize()
        cls[ids.astype(np.int64)] = new
        moved += ids.size
        assert np.array_equal(eng.get_class(all_ids), cls)
    assert moved > 1_000 and queued_seen > 500
    state = tables[0].tb.state
    v, tt = eng.export_state()
    t_ref = np.array([state[k].t_us if k in state else ABSENT for k in range(n_keys)], dtype=np.int64)
    assert np.array_equal(tt, t_ref)
    for k in state:
        assert np.float64(v[k]).view(np.uint64) == np.float64(state[k].v).view(np.uint64), k
    for k in rng.choice(n_keys, 100, replace=False).tolist():
        assert eng.queue_of(k) == tables[cls[k]].queue_of(k), k
    eng.close()


# ---------------------------------------------------------------- 7. maintenance by class
TTL_MS = np.array([4_000, 6_000, 3_000, 1_000], dtype=np.int64)   # ceil(max(TokenLimit / rate, 1)) s


def test_maintenance_calls_judge_by_class(engine_lib, gpu):
    import torch
    from oracle import semantics as sem
    n = 5_000
    assert [sem.TokenBucketTable(sem.TokenBucketConfig.from_options(*c[:3])).ttl_ms for c in QC] == TTL_MS.tolist()
    ts = T0 + 100_000_000 + 123
    rng = np.random.default_rng(77)
    cls = _mix_cls(n)
    v = rng.uniform(0.0, 0.9, n)                       # under one token: a wait of one permit queues
    t = ts - rng.integers(0, 8_000_000, n)             # ages up to 8 s: around every class's TTL
    t[rng.random(n) < 0.15] = ABSENT
    ttl = TTL_MS[cls]
    gone = (t == ABSENT) | (t < 1000 * (ts // 1000 - ttl))
    age = np.where(t == ABSENT, -1, ts - t)
    mid = (age > 3_100_000) & (age < 3_900_000)        # lapsed for classes 2 and 3 (3 s, 1 s), not for 0 and 1
    assert gone[mid & (cls >= 2)].all() and not gone[mid & (cls < 2)].any()
    assert (mid & (cls >= 2)).sum() > 100 and (mid & (cls < 2)).sum() > 100
    eng = _engine(n)
    _set_all(eng, cls)
    eng.import_state(v, t)
    # queued entries on every fifth present key of classes 0, 1 and 3 (class 2 never queues):
    # each wait runs the script at its row's own time, where nothing has lapsed or refilled and
    # v < 1 denies one permit, so the rows stay exactly as imported
    cand = np.flatnonzero((t != ABSENT) & (cls != 2) & (age > 0))[::5]
    qk = cand.astype(np.uint64)
    s, _, _ = eng.wait_batch(qk, np.ones(len(qk), np.int32), t[cand], 0)
    assert (s == QUEUED).all()
    queued = np.zeros(n, dtype=bool)
    queued[cand] = True
    assert (queued & gone).sum() > 50
    dead = gone & ~queued
    first, count = 3, 4_001
    buf = torch.full((count + 64,), 0xAA, dtype=torch.uint8, device=gpu)
    buf2 = torch.full((count,), 0xAA, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    eng.expired_device(ts, buf[:count], first=first)
    eng.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[:count], dead[first:first + count].astype(np.uint8))
    assert (got[count:] == 0xAA).all()
    for k in rng.choice(n, 48, replace=False).tolist() + np.nonzero(mid)[0][:16].tolist():
        q = eng.query(k, ts)
        assert (q is None) == bool(gone[k]), k
        if q is not None:
            assert q[0] == v[k]
    d_ids, d_v, d_t = eng.export_live(ts)
    live = np.nonzero(~gone)[0]                        # (queue headers play no part in the export)
    assert np.array_equal(d_ids.cpu().numpy(), live)
    assert np.array_equal(d_v.cpu().numpy().view(np.uint64), v[live].view(np.uint64))
    assert np.array_equal(d_t.cpu().numpy(), t[live])
    # statistics: available by the key's class, queued from its header
    keys = rng.choice(n, 600, replace=False).astype(np.uint64)
    _, _, avail, nq = eng.statistics(keys, ts)
    tables = [sem.TokenBucketTable(sem.TokenBucketConfig.from_options(*c[:3])) for c in QC]
    for k, a, q in zip(keys.tolist(), avail.tolist(), nq.tolist()):
        tb = tables[cls[k]]
        tb.state.clear()
        if t[k] != ABSENT:
            tb.state[k] = sem.BucketState(float(v[k]), int(t[k]))
        assert a == tb.acquire(k, 10**6, ts)[1], k     # the `remaining` a denied request is told
        assert q == int(queued[k]), k
    assert len(set(avail.tolist())) >= 4               # class caps 4, 2, 3, 6 and refilled rows
    # clear: lapsed rows of the range become absent, the others and the classes stay
    eng.expired_device(ts, buf2, first=first, clear=True)
    eng.synchronize()
    assert np.array_equal(buf2.cpu().numpy(), got[:count])
    _, t2 = eng.export_state()
    cleared = np.zeros(n, dtype=bool)
    cleared[first:first + count] = gone[first:first + count]
    assert (t2[cleared] == ABSENT).all() and np.array_equal(t2[~cleared], t[~cleared])
    assert np.array_equal(eng.get_class(np.arange(n, dtype=np.uint64)), cls)
    eng.close()


# ---------------------------------------------------------------- 8. cancel and stats
def test_cancel_and_stats(engine_lib, oracle_lib, gpu):
    n_keys, n = 10_000, 50_000
    rng = np.random.default_rng(3)
    cls = _mix_cls(n_keys)
    eng = _engine(n_keys, stats=True)
    _set_all(eng, cls)
    ref = _PerClass(n_keys, cls)
    ok = np.zeros(n_keys, np.uint64)
    failed = np.zeros(n_keys, np.uint64)

    def counted_round(eng, ref, keys, permits, ts, id_base, t_tick, tag):
        """_host_round, counting what tbe.h says the engine counts."""
        ev_before, dr_before = ref.evictions.sum(), ref.drained.sum()
        s, r = _host_round(eng, ref, keys, permits, ts, id_base, t_tick, tag)
        np.add.at(ok, keys[s == GRANTED].astype(np.int64), 1)
        np.add.at(failed, keys[s == FAILED].astype(np.int64), 1)
        np.add.at(failed, keys[ref.last_causes].astype(np.int64), 1)   # an evicted entry sits on its cause's key
        np.add.at(ok, ref.last_drained_keys.astype(np.int64), 1)
        assert len(ref.last_causes) == ref.evictions.sum() - ev_before
        assert len(ref.last_drained_keys) == ref.drained.sum() - dr_before
        return s, r

    keys, permits, ts = _workload(rng, n_keys, n, T0)
    s, _ = counted_round(eng, ref, keys, permits, ts, 0, T0 + 1_000, "batch 0")   # an early tick: queues stay
    at = np.concatenate([np.flatnonzero(s == QUEUED)[:400], np.flatnonzero(s == GRANTED)[:100],
                         np.flatnonzero(s == FAILED)[:50]])
    ck = np.concatenate([keys[at], keys[:20]])
    ci = np.concatenate([at, np.arange(20) + 10 * n]).astype(np.int64)         # 20 unknown ids
    got = eng.cancel(ck, ci)
    want = ref.cancel(ck, ci)
    assert np.array_equal(got, want) and 50 < int(want.sum()) < len(want)
    for k in np.unique(ck)[:200].tolist():
        assert eng.queue_of(k) == ref.queue_of(k), k
    keys, permits, ts = _workload(rng, n_keys, n, T0 + 2_000_000)
    counted_round(eng, ref, keys, permits, ts, n, T0 + 4_000_000, "batch 1")
    _same_state(eng, ref)
    # lease statistics (tbe.h): grants and drained grants count ok, FAILED and evictions failed,
    # QUEUED, REJECTED and cancels nothing
    got_ok, got_failed = eng.stats_export()
    assert np.array_equal(got_ok, ok) and np.array_equal(got_failed, failed)
    assert eng.stats_totals() == (int(ok.sum()), int(failed.sum()))
    assert ref.evictions.sum() > 1_000 and ref.drained.sum() > 1_000
    some = rng.choice(n_keys, 500).astype(np.uint64)
    s_ok, s_failed, _, s_q = eng.statistics(some, T0 + 4_000_000)
    assert np.array_equal(s_ok, ok[some.astype(np.int64)]) and np.array_equal(s_failed, failed[some.astype(np.int64)])
    assert s_q.tolist() == [sum(p for _, p in ref.queue_of(int(k))) for k in some]
    eng.close()


# ---------------------------------------------------------------- 9. refusals and layout
def test_refusals_layout_and_recreate(engine_lib, gpu, tmp_path):
    from distributedratelimiting.redis_amd import ApproximateEngine, snapshot
    with pytest.raises(ValueError):
        ApproximateEngine(100, 10, 1, 10_000_000, 4, 0, device=0, classes=[(3, 1, 10_000_000, 2, 0)])
    n = 70_000
    eng = _engine(n)
    lay = eng.layout()
    assert not lay["packed"] and not lay["narrow"] and not lay["medium"] and lay["queue_header_32"]
    assert eng.queue_classes() == QC and eng.classes() == [c[:3] for c in QC]
    with pytest.raises(ValueError, match="classes"):
        snapshot.save(str(tmp_path / "classed.npz"), eng, T0)
    assert not (tmp_path / "classed.npz").exists()
    _set_all(eng, np.full(n, 2, dtype=np.uint8))
    eng.close()
    eng = _engine(n)                                   # most likely over the same device memory
    assert not eng.get_class(np.arange(n, dtype=np.uint64)).any()
    s, r, _ = eng.wait_batch([5, n - 1, 5], [1, 1, 4], [T0, T0, T0], 0)
    assert s.tolist() == [GRANTED, GRANTED, QUEUED] and r.tolist()[:2] == [3, 3]   # class 0: TokenLimit 4
    eng.close()
