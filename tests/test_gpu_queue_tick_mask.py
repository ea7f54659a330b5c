"""Per-class replenish ticks of the queueing kind (tbe_refresh_classes,
tbe_refresh_classes_device, tbe_wait_batch_tick_classes_device in include/tbe.h).  Every
comparison is exact.

Reference: as tests/test_gpu_queue_classes.py, one oracle.cref.CQueueingTokenBucket per class,
each fed its class's requests; a masked tick calls refresh(ts) on the references of the classes
in the mask alone, as the reference's per-limiter timer drains that limiter's queue alone
(Q:237-271).  In a schedule, an entry (dt, mask) means: one _workload batch at t, then
t += dt, then a tick at t with that mask."""
import ctypes

import numpy as np
import pytest
from test_gpu_queue_classes import (BIG, QC, T0, _dense_trace, _dev, _engine, _mix_cls, _PerClass, _same_state,
                                    _set_all, _workload)

pytestmark = pytest.mark.gpu

FAILED, GRANTED, QUEUED, REJECTED = 0, 1, 2, 3
S = 1_000_000
ALL4 = {0, 1, 2, 3}


class _Masked(_PerClass):
    """_PerClass whose tick refreshes the references of the masked classes alone."""

    def refresh(self, ts, mask=None):
        ks, ids, rems = [np.empty(0, np.uint64)], [np.empty(0, np.int64)], [np.empty(0, np.int32)]
        self.last_by_class = np.zeros(len(self.refs), np.int64)
        for c, ref in enumerate(self.refs):
            if mask is not None and c not in mask:
                continue
            k, i, r = ref.refresh(ts, threads=self.threads)
            ks.append(k.astype(np.uint64))
            ids.append(self.ids[c][i])
            rems.append(r.astype(np.int32))
            self.drained[c] += len(k)
            self.last_by_class[c] = len(k)
        k, i, r = np.concatenate(ks), np.concatenate(ids), np.concatenate(rems)
        o = np.argsort(k, kind="stable")
        self.last_drained_keys = k[o]
        return k[o], i[o], r[o]


def _clear_class_grants(n_keys, cls, classes, batch, t_tick, mask, threads=1):
    """What keeps a masked tick from passing vacuously: a second per-class reference fed the same
    first batch and ticked unmasked grants this much in the classes whose bit is clear."""
    twin = _Masked(n_keys, cls, classes, threads=threads)
    twin.wait(*batch, 0)
    twin.refresh(t_tick)
    return int(sum(g for c, g in enumerate(twin.last_by_class) if c not in mask))


def _bufs(eng, n, gpu):
    import torch
    cap = int(eng.refresh_bound()) + n
    return (torch.empty(n, dtype=torch.uint8, device=gpu), torch.empty(n, dtype=torch.int32, device=gpu),
            torch.empty(cap, dtype=torch.int64, device=gpu), torch.empty(cap, dtype=torch.int64, device=gpu),
            torch.empty(cap, dtype=torch.int32, device=gpu), torch.full((1,), 77, dtype=torch.int32, device=gpu))


def _log_of(d_ks, d_id, d_rem, d_cnt):
    m = int(d_cnt.item())
    ks = d_ks[:m].cpu().numpy().view(np.uint64)
    o = np.argsort(ks, kind="stable")
    return ks[o] >> np.uint64(16), d_id[:m].cpu().numpy()[o], d_rem[:m].cpu().numpy()[o]


def _same_log(got, want, tag):
    print(f"{tag}: {len(want[0])} grants")
    assert len(got[0]) == len(want[0]), f"{len(got[0])} grants logged, {len(want[0])} expected, {tag}"
    for g, w in zip(got, want):
        assert np.array_equal(g, w), f"drain log mismatch, {tag}"


def _round(eng, ref, batch, id_base, t_tick, mask, mode, gpu, tag):
    """One batch and one masked tick through `mode`: "host" (wait_batch, refresh), "fused"
    (wait_batch_tick_device) or "device" (wait_batch_device, refresh_device)."""
    import torch
    keys, permits, ts = batch
    s_ref, r_ref, ec_ref, ei_ref = ref.wait(keys, permits, ts, id_base)
    want = ref.refresh(t_tick, mask)
    classes = None if mask is None else sorted(mask)
    if mode == "host":
        s, r, (ec, ei) = eng.wait_batch(keys, permits, ts, id_base)
        assert eng.refresh_bound() >= len(want[0])
        got = eng.refresh(t_tick, classes=classes)
    else:
        n = len(keys)
        d_s, d_r, d_ks, d_id, d_rem, d_cnt = _bufs(eng, n, gpu)
        dk, dp, dt = _dev(keys, gpu), _dev(permits, gpu), _dev(ts, gpu)
        torch.cuda.synchronize()
        if mode == "fused":
            eng.wait_batch_tick_device(dk, dp, dt, d_s, d_r, id_base, t_tick, d_ks, d_id, d_rem, d_cnt,
                                       classes=classes)
            eng.synchronize()
            ec, ei = eng.evicted()
        else:
            eng.wait_batch_device(dk, dp, dt, d_s, d_r, id_base)
            eng.synchronize()
            ec, ei = eng.evicted()
            eng.refresh_device(t_tick, d_ks, d_id, d_rem, d_cnt, classes=classes)
            eng.synchronize()
        s, r = d_s.cpu().numpy(), d_r.cpu().numpy()
        got = _log_of(d_ks, d_id, d_rem, d_cnt)
    assert np.array_equal(s, s_ref), f"status mismatch, {tag}"
    assert np.array_equal(r, r_ref), f"remaining mismatch, {tag}"
    assert np.array_equal(ec, ec_ref) and np.array_equal(ei, ei_ref), f"evictions mismatch, {tag}"
    _same_log(got, want, tag)
    return s


def _schedule(eng, ref, rng, n_keys, n, sched, mode, gpu, share=0.0, check=None):
    t, first = T0, None
    for b, (dt, mask) in enumerate(sched):
        batch = _workload(rng, n_keys, n, t, share)
        t += dt
        first = first or (batch, t, mask)
        _round(eng, ref, batch, b * n, t, mask, mode, gpu, f"tick {b} {mode}")
        if check:
            check(b, ref)
        _same_state(eng, ref)
    return first


# ---------------------------------------------------------------- 1. host calls
def test_host_masked_ticks(engine_lib, oracle_lib, gpu):
    n_keys, n = 10_000, 50_000
    rng = np.random.default_rng(1)
    cls = _mix_cls(n_keys)
    eng = _engine(n_keys)
    _set_all(eng, cls)
    ref = _Masked(n_keys, cls)
    # the first tick comes 10 s after its batch: beyond class 0's 4 s and class 3's 1 s TTL, so a
    # masked-out row that the tick rewrites absent shows in the state comparison
    sched = [(10 * S, {1}), (1 * S, {0, 3}), (3 * S, {1}), (1 * S, {0, 2, 3}), (2 * S, ALL4)]

    def check(b, ref):
        assert ref.last_by_class.sum() >= 1_000, (b, ref.last_by_class)

    batch, t1, m1 = _schedule(eng, ref, rng, n_keys, n, sched, "host", gpu, check=check)
    assert _clear_class_grants(n_keys, cls, QC, batch, t1, m1) >= 2_500
    for k in rng.choice(n_keys, 200, replace=False).tolist():
        assert eng.queue_of(k) == ref.queue_of(k), k
    eng.close()


# ---------------------------------------------------------------- 2. fused ticks
@pytest.mark.parametrize("mode", ["fused", "device"])
@pytest.mark.parametrize("share", [0.0, 0.08])
def test_fused_masked_ticks(engine_lib, oracle_lib, gpu, share, mode):
    n_keys, n = 6_000, 40_000
    rng = np.random.default_rng(2)
    cls = _mix_cls(n_keys)
    assert cls[1234] == 3
    eng = _engine(n_keys)
    _set_all(eng, cls)
    ref = _Masked(n_keys, cls)
    sched = [(10 * S, {1}), (1 * S, {0, 3}), (2 * S, ALL4)]

    def check(b, ref):
        if b == 0:
            assert ref.last_by_class.sum() >= 1_000, ref.last_by_class

    batch, t1, m1 = _schedule(eng, ref, rng, n_keys, n, sched, mode, gpu, share, check)
    assert _clear_class_grants(n_keys, cls, QC, batch, t1, m1) >= 2_500
    assert eng.queue_of(1234) == ref.queue_of(1234)
    eng.close()


# ---------------------------------------------------------------- 3. mask words 1 to 3, 64-bit headers
@pytest.mark.parametrize("mode", ["fused", "host"])
def test_mask_words_and_wide_headers(engine_lib, oracle_lib, gpu, mode):
    n_keys, n, n_cls = 3_000, 30_000, 130
    classes = [QC[i % 4] for i in range(n_cls)]
    cls = _mix_cls(n_keys, n_cls)
    sched = [(10 * S, {1, 64, 67, 129}), (1 * S, set(range(0, n_cls, 2))), (2 * S, set(range(n_cls)))]

    def check(b, ref):
        if b == 0:
            got = [int(ref.last_by_class[c]) for c in (1, 64, 67, 129)]
            assert min(got) >= 10, got

    rng = np.random.default_rng(4)
    eng = _engine(n_keys, classes)
    assert eng.layout()["queue_header_32"]
    _set_all(eng, cls)
    ref = _Masked(n_keys, cls, classes)
    batch, t1, m1 = _schedule(eng, ref, rng, n_keys, n, sched, mode, gpu, check=check)
    assert _clear_class_grants(n_keys, cls, classes, batch, t1, m1) >= 2_500
    eng.close()
    # one class's QueueLimit at 2,000: 64-bit queue headers, the u64 forms of both kernels
    wide = list(classes)
    wide[17] = (QC[1][0], QC[1][1], QC[1][2], 2000, QC[1][4])
    rng = np.random.default_rng(4)
    eng = _engine(n_keys, wide)
    assert not eng.layout()["queue_header_32"]
    _set_all(eng, cls)
    ref = _Masked(n_keys, cls, wide)
    _schedule(eng, ref, rng, n_keys, n, sched[:2], mode, gpu, check=check)
    eng.close()


# ---------------------------------------------------------------- 4. full-R buckets, a short last bucket
def test_dense_full_r_masked_fused_ticks(engine_lib, oracle_lib, gpu):
    rng = np.random.default_rng(20262)
    cls = _mix_cls(BIG)
    eng = _engine(BIG)
    assert eng.layout()["r_bits"] == 11 and BIG % 2048 != 0
    _set_all(eng, cls)
    ref = _Masked(BIG, cls, threads=16)
    n, t = 1 << 18, T0
    for b, (dt, mask) in enumerate([(700_000, {0, 3}), (10 * S, {1})]):
        batch = _dense_trace(rng, n, t)
        t = int(batch[2][-1]) + dt
        _round(eng, ref, batch, b * n, t, mask, "fused", gpu, f"dense tick {b}")
        assert ref.last_by_class.sum() >= 1_000, ref.last_by_class
    _same_state(eng, ref)
    last = BIG - 1
    assert eng.queue_of(last) == ref.queue_of(last)
    eng.close()


# ---------------------------------------------------------------- 5. an engine without extra classes
def _plain(n_keys):
    from distributedratelimiting.redis_amd import QueueingTokenBucketEngine
    c0 = QC[0]
    return QueueingTokenBucketEngine(n_keys, c0[0], c0[1], c0[2], c0[3], c0[4], device=0)


def _bits(eng):
    v, t = eng.export_state()
    return v.view(np.uint64).copy(), t.copy()


def test_unclassed_engine(engine_lib, gpu):
    import torch
    n_keys, n = 5_000, 30_000
    rng = np.random.default_rng(5)
    a, b = _plain(n_keys), _plain(n_keys)
    keys, permits, ts = _workload(rng, n_keys, n, T0)
    for e in (a, b):
        e.wait_batch(keys, permits, ts, 0)
    some = rng.choice(n_keys, 100, replace=False).tolist()
    # classes=[]: nothing logged, nothing changed
    before, q_before = _bits(a), [a.queue_of(k) for k in some]
    lk, li, lr = a.refresh(T0 + 10 * S, classes=[])
    assert len(lk) == len(li) == len(lr) == 0
    after = _bits(a)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert [a.queue_of(k) for k in some] == q_before and sum(len(q) for q in q_before) > 50
    d_s, d_r, d_ks, d_id, d_rem, d_cnt = _bufs(a, n, gpu)
    a.refresh_device(T0 + 10 * S, d_ks, d_id, d_rem, d_cnt, classes=[])
    a.synchronize()
    assert int(d_cnt.item()) == 0
    after = _bits(a)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # classes=[0]: the unmasked tick of the twin, by log and state
    got, want = a.refresh(T0 + 2 * S, classes=[0]), b.refresh(T0 + 2 * S)
    assert len(want[0]) >= 1_000
    _same_log(got, want, "classes=[0]")
    for x, y in zip(_bits(a), _bits(b)):
        assert np.array_equal(x, y)
    # the fused call with classes=[] gives wait_batch_device's replies; with [0] the unmasked fused call's
    for step, classes in enumerate(([], [0])):
        t = T0 + (3 + 2 * step) * S
        keys, permits, ts = _workload(rng, n_keys, n, t)
        dk, dp, dt = _dev(keys, gpu), _dev(permits, gpu), _dev(ts, gpu)
        outs = []
        for e in (a, b):
            d_s, d_r, d_ks, d_id, d_rem, d_cnt = _bufs(e, n, gpu)
            torch.cuda.synchronize()
            if e is a:
                e.wait_batch_tick_device(dk, dp, dt, d_s, d_r, (step + 1) * n, t + S, d_ks, d_id, d_rem, d_cnt,
                                         classes=classes)
            elif classes:
                e.wait_batch_tick_device(dk, dp, dt, d_s, d_r, (step + 1) * n, t + S, d_ks, d_id, d_rem, d_cnt)
            else:
                e.wait_batch_device(dk, dp, dt, d_s, d_r, (step + 1) * n)
                d_cnt.zero_()
            e.synchronize()
            outs.append((d_s.cpu().numpy(), d_r.cpu().numpy(), e.evicted(), _log_of(d_ks, d_id, d_rem, d_cnt)))
        (s0, r0, ev0, log0), (s1, r1, ev1, log1) = outs
        assert np.array_equal(s0, s1) and np.array_equal(r0, r1)
        assert np.array_equal(ev0[0], ev1[0]) and np.array_equal(ev0[1], ev1[1])
        assert len(log0[0]) == (0 if not classes else len(log1[0]))
        _same_log(log0, log1, f"fused classes={classes}")
        if classes:
            assert len(log1[0]) >= 1_000
        for x, y in zip(_bits(a), _bits(b)):
            assert np.array_equal(x, y)
    for k in some:
        assert a.queue_of(k) == b.queue_of(k), k
    a.close()
    b.close()


# ---------------------------------------------------------------- 6. statistics
def test_statistics_of_masked_ticks(engine_lib, oracle_lib, gpu):
    n_keys, n = 10_000, 50_000
    rng = np.random.default_rng(6)
    cls = _mix_cls(n_keys)
    eng = _engine(n_keys, stats=True)
    _set_all(eng, cls)
    ref = _Masked(n_keys, cls)
    ok = np.zeros(n_keys, np.uint64)
    failed = np.zeros(n_keys, np.uint64)
    t = T0
    for b, (dt, mask, mode) in enumerate([(10 * S, {1}, "host"), (1 * S, {0, 3}, "fused"), (2 * S, {1, 3}, "device")]):
        batch = _workload(rng, n_keys, n, t)
        t += dt
        s = _round(eng, ref, batch, b * n, t, mask, mode, gpu, f"stats tick {b}")
        keys = batch[0]
        np.add.at(ok, keys[s == GRANTED].astype(np.int64), 1)
        np.add.at(failed, keys[s == FAILED].astype(np.int64), 1)
        np.add.at(failed, keys[ref.last_causes].astype(np.int64), 1)
        np.add.at(ok, ref.last_drained_keys.astype(np.int64), 1)
        assert len(ref.last_drained_keys) >= 1_000
    some = rng.choice(n_keys, 500).astype(np.uint64)
    s_ok, s_failed, _, s_q = eng.statistics(some, t)
    assert np.array_equal(s_ok, ok[some.astype(np.int64)]) and np.array_equal(s_failed, failed[some.astype(np.int64)])
    assert s_q.tolist() == [sum(p for _, p in ref.queue_of(int(k))) for k in some]
    got_ok, got_failed = eng.stats_export()
    assert np.array_equal(got_ok, ok) and np.array_equal(got_failed, failed)
    assert eng.stats_totals() == (int(ok.sum()), int(failed.sum()))
    eng.close()


# ---------------------------------------------------------------- refusals that need a live engine
def test_refusals(engine_lib, gpu):
    from distributedratelimiting.redis_amd import ApproximateEngine, TokenBucketEngine, _capi
    import torch
    EINVAL = _capi.TBE_EINVAL
    eng = _engine(64)                       # four classes
    lib, h = eng._lib, eng.handle
    n = ctypes.c_uint64(5)
    d = torch.zeros(16, dtype=torch.int64, device=gpu)
    d_cnt = torch.full((1,), 77, dtype=torch.int32, device=gpu)
    p, cnt = d.data_ptr(), d_cnt.data_ptr()
    good = _capi.class_mask([0, 3])

    def all_three(handle, ts, mask, n_granted, count):
        return [lib.tbe_refresh_classes(handle, ts, mask, n_granted),
                lib.tbe_refresh_classes_device(handle, ts, mask, p, p, p, 16, count, None),
                lib.tbe_wait_batch_tick_classes_device(handle, p, p, p, 0, 0, 1, p, p, ts, mask, p, p, p, 16, count,
                                                       None)]

    assert all_three(h, T0, None, ctypes.byref(n), cnt) == [EINVAL] * 3                      # NULL mask
    for bad in ([4], [0, 64], [255]):                                                        # a bit >= 4 classes
        assert all_three(h, T0, _capi.class_mask(bad), ctypes.byref(n), cnt) == [EINVAL] * 3, bad
    assert "class" in lib.tbe_last_error(h).decode()
    assert all_three(h, -1, good, ctypes.byref(n), cnt) == [EINVAL] * 3                      # ts_us < 0
    assert all_three(h, T0, good, None, None) == [EINVAL] * 3                                # NULL n_granted / d_count
    plain = _plain(64)
    assert all_three(plain.handle, T0, _capi.class_mask([1]), ctypes.byref(n), cnt) == [EINVAL] * 3   # one class
    plain.close()
    tb = TokenBucketEngine(64, 4, 1, 10_000_000, device=0)
    ap = ApproximateEngine(64, 4, 1, 10_000_000, 8, device=0)
    for other in (tb, ap):
        assert all_three(other.handle, T0, _capi.class_mask([0]), ctypes.byref(n), cnt) == [EINVAL] * 3
        other.close()
    torch.cuda.synchronize()
    assert int(d_cnt.item()) == 77          # no refused call touched the device
    with pytest.raises(ValueError):
        eng.refresh(T0, classes=[256])
    # every accepted form works on the empty engine
    assert all_three(h, T0, good, ctypes.byref(n), cnt)[:2] == [0, 0] and n.value == 0
    eng.synchronize()
    assert int(d_cnt.item()) == 0
    eng.close()
