"""Limit classes (tbe_create_classes / tbe_set_class in include/tbe.h): one
engine, per-key {TokenLimit, fill rate, TTL}.  Every comparison is exact: replies, t_us of
every key, and the bits of v on present keys (v of an absent row is not part of the
contract on a classed engine).

Oracles: for keys that keep their class, one oracle.cref.CTokenBucket per class, each fed
its class's requests in arrival order; for class changes, one semantics.TokenBucketTable per
class, all sharing one state dict (what Redis holds when several limiters' scripts run on
the same hashes, with the lapse judged by the key's current class)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ABSENT = np.iinfo(np.int64).min
# (TokenLimit, TokensPerPeriod, ticks): rates 1/s, 1/3 per second (inexact), 500/s, 10/s
CLASSES = [(10, 1, 10_000_000), (3, 1, 30_000_000), (100, 50, 1_000_000), (5, 10, 10_000_000)]
TTL_MS = np.array([10_000, 9_000, 1_000, 1_000], dtype=np.int64)
T0 = 1_760_000_000_000_000
BIG = 3 * (1 << 20) - 5          # R = 2048, 1536 buckets, 2 passes, a short last bucket


def _engine(n_keys, **kw):
    from distributedratelimiting.redis_amd import TokenBucketEngine
    return TokenBucketEngine(n_keys, *CLASSES[0], device=0, classes=CLASSES[1:], **kw)


def _mix_cls(n_keys):
    from oracle import trace
    return (trace.mix64(np.arange(n_keys, dtype=np.uint64)) % np.uint64(4)).astype(np.uint8)


class _PerClass:
    """One CTokenBucket per class; every key stays in its class."""

    def __init__(self, n_keys, cls):
        from distributedratelimiting.redis_amd import fill_rate
        from oracle import cref
        self.cls = cls
        self.refs = [cref.CTokenBucket(n_keys, c[0], fill_rate(c[1], c[2])) for c in CLASSES]

    def acquire(self, keys, permits, ts):
        g = np.empty(len(keys), np.uint8)
        r = np.empty(len(keys), np.int32)
        kc = self.cls[keys.astype(np.int64)]
        for c, ref in enumerate(self.refs):
            m = kc == c
            if m.any():
                g[m], r[m] = ref.acquire_batch(keys[m], permits[m], ts[m])
        return g, r

    def state(self):
        v = np.empty(len(self.cls), np.float64)
        t = np.empty(len(self.cls), np.int64)
        for c, ref in enumerate(self.refs):
            vc, tc = ref.export_state()
            m = self.cls == c
            v[m], t[m] = vc[m], tc[m]
        return v, t


def _same_state(eng, v_ref, t_ref):
    v, t = eng.export_state()
    assert np.array_equal(t, t_ref), f"{int((t != t_ref).sum())} keys differ in t_us"
    present = t_ref != ABSENT
    assert np.array_equal(v[present].view(np.uint64), v_ref[present].view(np.uint64))


def _dev(a, gpu):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(gpu)


def _set_all(eng, cls):
    eng.set_class(np.arange(len(cls), dtype=np.uint64), cls)
    assert np.array_equal(eng.get_class(np.arange(len(cls), dtype=np.uint64)), cls)


# ---------------------------------------------------------------- 1. the smoke shape
def test_smoke_shape(engine_lib, oracle_lib, gpu):
    from distributedratelimiting.redis_amd import TokenBucketEngine
    from oracle import trace
    n_keys, n = 10_000, 50_000
    cls = _mix_cls(n_keys)
    eng = _engine(n_keys)
    assert eng.layout()["r_bits"] == 4 and eng.layout()["passes"] == 2
    assert eng.classes() == CLASSES
    _set_all(eng, cls)
    plain = TokenBucketEngine(n_keys, *CLASSES[0], device=0)
    ref = _PerClass(n_keys, cls)
    differs = False
    for b in range(3):
        keys, permits, ts = trace.make_batch(0x5EED0001, n_keys, b, n, 200_000, 1, 3)
        g, r = eng.acquire_batch(keys, permits, ts)
        g_ref, r_ref = ref.acquire(keys, permits, ts)
        assert np.array_equal(g, g_ref), f"granted mismatch in batch {b}"
        assert np.array_equal(r, r_ref), f"remaining mismatch in batch {b}"
        g0, r0 = plain.acquire_batch(keys, permits, ts)
        differs |= not (np.array_equal(g, g0) and np.array_equal(r, r0))
    assert differs, "a class-0 engine gives the same replies: the classes decide nothing here"
    _same_state(eng, *ref.state())
    plain.close()
    eng.close()


# ---------------------------------------------------------------- 2. full-R dense shape
def _dense_trace(rng, n, t_start):
    """Half of the requests in 64 buckets (the short last one among them; in half of those
    only rows 0..511, so a 1,536-request chunk leaves more than 512 pending after round 1),
    five keys with 300 requests each, one with 3,000, the rest uniform."""
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
    permits = np.array([0, 1, 2, 4, 11], dtype=np.int32)[rng.integers(0, 5, n)]
    step = rng.integers(0, 3, n).astype(np.int64)
    step[rng.choice(n, 4, replace=False)] += 1_500_000        # jumps of more than a second
    ts = t_start + np.cumsum(step)
    return keys, permits, ts


@pytest.fixture(scope="module")
def dense_case(oracle_lib):
    rng = np.random.default_rng(20260)
    cls = _mix_cls(BIG)
    n = 1 << 20
    k0, p0, t0 = _dense_trace(rng, n, T0)
    k1, p1, t1 = _dense_trace(rng, n, int(t0[-1]) + 700_000)
    keys, permits, ts = np.concatenate([k0, k1]), np.concatenate([p0, p1]), np.concatenate([t0, t1])
    assert (np.diff(ts) >= 0).all()
    ref = _PerClass(BIG, cls)
    g, r = ref.acquire(keys, permits, ts)
    v, t = ref.state()
    _, per_key = np.unique(keys[:n], return_counts=True)
    assert per_key.max() >= 3_000                                # more than kHotMin = 2048
    return {"cls": cls, "keys": keys, "permits": permits, "ts": ts, "g": g, "r": r, "v": v, "t": t, "n": n}


def test_dense_host_call(engine_lib, dense_case, gpu):
    c = dense_case
    eng = _engine(BIG)
    lay = eng.layout()
    assert lay["r_bits"] == 11 and lay["passes"] == 2
    _set_all(eng, c["cls"])
    n = c["n"]
    for b in range(2):
        s = slice(b * n, (b + 1) * n)
        assert not eng.batch_format(n)["sparse"]
        g, r = eng.acquire_batch(c["keys"][s], c["permits"][s], c["ts"][s])
        print("batch", b, "grant rate", float(g.mean()))
        assert np.array_equal(g, c["g"][s]), f"granted mismatch in batch {b}"
        assert np.array_equal(r, c["r"][s]), f"remaining mismatch in batch {b}"
    _same_state(eng, c["v"], c["t"])
    eng.close()


def test_dense_pipelined_device_batches(engine_lib, dense_case, gpu):
    import torch
    c = dense_case
    eng = _engine(BIG)
    assert eng.layout()["pipeline"]
    n_all = len(c["keys"])
    d_ids = torch.arange(BIG, dtype=torch.int64, device=gpu)
    d_cls = _dev(c["cls"], gpu)
    cuts = [0, 700_001, 1_400_000, n_all]              # odd sizes, each batch in buffers of its own
    parts = [(slice(a, b), _dev(c["keys"][a:b], gpu), _dev(c["permits"][a:b], gpu), _dev(c["ts"][a:b], gpu),
              torch.empty(b - a, dtype=torch.uint8, device=gpu), torch.empty(b - a, dtype=torch.int32, device=gpu))
             for a, b in zip(cuts[:-1], cuts[1:])]
    torch.cuda.synchronize()
    eng.set_class_device(d_ids, d_cls)                 # ordered before the batches below
    for _, dk, dp, dt, dg, dr in parts:                # back to back, no synchronise: they pipeline
        eng.acquire_batch_device(dk, dp, dt, dg, dr)
    eng.synchronize()
    for s, _, _, _, dg, dr in parts:
        assert np.array_equal(dg.cpu().numpy(), c["g"][s]), s
        assert np.array_equal(dr.cpu().numpy(), c["r"][s]), s
    _same_state(eng, c["v"], c["t"])
    eng.close()


# ---------------------------------------------------------------- 3. sparse shape
def test_sparse_shape(engine_lib, oracle_lib, gpu):
    rng = np.random.default_rng(303)
    cls = _mix_cls(BIG)
    eng = _engine(BIG)
    _set_all(eng, cls)
    ref = _PerClass(BIG, cls)
    n = (1 << 14) + 600
    assert eng.batch_format(n)["sparse"]
    t_start = T0
    uni = rng.integers(0, BIG, 1 << 14)
    for b in range(3):                                 # later batches find rows, some lapsed
        if b:                                          # half of the uniform keys come back
            uni = np.concatenate([uni[:1 << 13], rng.integers(0, BIG, 1 << 13)])
        keys_b = np.concatenate([uni, 900 * 2048 + rng.integers(0, 2048, 600)]).astype(np.uint64)
        rng.shuffle(keys_b)
        permits = np.array([0, 1, 2, 4, 11], dtype=np.int32)[rng.integers(0, 5, n)]
        ts = t_start + np.cumsum(rng.integers(0, 40, n).astype(np.int64))
        g, r = eng.acquire_batch(keys_b, permits, ts)
        g_ref, r_ref = ref.acquire(keys_b, permits, ts)
        assert np.array_equal(g, g_ref), f"granted mismatch in batch {b}"
        assert np.array_equal(r, r_ref), f"remaining mismatch in batch {b}"
        t_start = int(ts[-1]) + 1_300_000              # classes 2 and 3 lapse before the next batch
    _same_state(eng, *ref.state())
    eng.close()


# ---------------------------------------------------------------- 4. class changes
def test_class_changes(engine_lib, gpu):
    import torch
    from distributedratelimiting.redis_amd import _capi
    from oracle import semantics as sem
    n_keys, n, nb = 64, 4_000, 500
    rng = np.random.default_rng(44)
    tables = [sem.TokenBucketTable(sem.TokenBucketConfig.from_options(*c)) for c in CLASSES]
    for t in tables[1:]:
        t.state = tables[0].state                      # one Redis, four limiters' scripts
    state = tables[0].state
    assert [t.ttl_ms for t in tables] == TTL_MS.tolist()
    keys = rng.integers(0, n_keys, n).astype(np.uint64)
    permits = rng.integers(0, 4, n).astype(np.int32)
    ts = T0 + np.sort(rng.integers(0, 32_000_000, n)).astype(np.int64)
    cls = _mix_cls(n_keys)
    eng = _engine(n_keys)
    assert eng.layout()["passes"] == 1
    _set_all(eng, cls)
    lapses = grants = 0
    for b in range(n // nb):
        s = slice(b * nb, (b + 1) * nb)
        g, r = eng.acquire_batch(keys[s], permits[s], ts[s])
        g_ref, r_ref = [], []
        for k, p, t in zip(keys[s].tolist(), permits[s].tolist(), ts[s].tolist()):
            tb = tables[cls[k]]
            st = state.get(k)
            lapses += st is not None and t // 1000 > st.t_us // 1000 + tb.ttl_ms
            ok, rem = tb.acquire(k, p, t)
            g_ref.append(int(ok))
            r_ref.append(rem)
        grants += sum(g_ref)
        assert g.tolist() == g_ref, f"granted mismatch in batch {b}"
        assert r.tolist() == r_ref, f"remaining mismatch in batch {b}"
        # half of the keys change class, by the host form and by the device form in turn
        ids = rng.choice(n_keys, n_keys // 2, replace=False).astype(np.uint64)
        new = rng.integers(0, 4, ids.size).astype(np.uint8)
        if b % 2 == 0:
            eng.set_class(ids, new)
        else:
            eng.set_class_device(_dev(ids, gpu), _dev(new, gpu))
        cls[ids.astype(np.int64)] = new
        # a void call changes nothing: class 4, then id n_keys, in either form
        for bad_ids, bad_cls in (([3, 5], [1, 4]), ([3, n_keys], [1, 1])):
            bi, bc = np.array(bad_ids, np.uint64), np.array(bad_cls, np.uint8)
            with pytest.raises(_capi.TbeError) as ei:
                eng.set_class(bi, bc)
            assert ei.value.status == _capi.TBE_EINVAL
            eng.set_class_device(_dev(bi, gpu), _dev(bc, gpu))
            with pytest.raises(_capi.TbeError) as ei:
                eng.synchronize()
            assert ei.value.status == _capi.TBE_EINVAL
            eng.synchronize()                          # the flag is cleared by the report
        assert np.array_equal(eng.get_class(np.arange(n_keys, dtype=np.uint64)), cls)
        d_got = torch.empty(n_keys, dtype=torch.uint8, device=gpu)
        d_all = torch.arange(n_keys, dtype=torch.int64, device=gpu)
        torch.cuda.synchronize()                       # (no stream given: the inputs are complete)
        eng.get_class_device(d_all, d_got)
        eng.synchronize()
        assert np.array_equal(d_got.cpu().numpy(), cls)
    print("lapses", lapses, "grant rate", grants / n)
    assert lapses > 50 and 0.2 < grants / n < 0.9      # the lapse and the deny branch are both taken
    v, t = eng.export_state()
    t_ref = np.array([state[k].t_us if k in state else ABSENT for k in range(n_keys)], dtype=np.int64)
    assert np.array_equal(t, t_ref)
    for k in state:
        assert np.float64(v[k]).view(np.uint64) == np.float64(state[k].v).view(np.uint64), k
    eng.close()


def test_plain_engine_has_class_zero_only(engine_lib, gpu):
    from distributedratelimiting.redis_amd import TokenBucketEngine, _capi
    eng = TokenBucketEngine(100, *CLASSES[0], device=0)
    assert eng.classes() == [CLASSES[0]]
    eng.set_class([1, 2], [0, 0])
    assert eng.get_class([1, 2, 99]).tolist() == [0, 0, 0]
    with pytest.raises(_capi.TbeError) as ei:
        eng.set_class([1, 2], [0, 1])
    assert ei.value.status == _capi.TBE_EINVAL
    eng.set_class_device(_dev(np.array([1], np.uint64), gpu), _dev(np.array([1], np.uint8), gpu))
    with pytest.raises(_capi.TbeError):
        eng.synchronize()
    eng.close()


# ---------------------------------------------------------------- 5. maintenance calls
def test_maintenance_calls_judge_by_class(engine_lib, gpu):
    import torch
    n = 5_000
    ts = T0 + 100_000_000 + 123
    rng = np.random.default_rng(55)
    cls = _mix_cls(n)
    v = rng.uniform(0.0, 3.0, n)
    t = ts - rng.integers(0, 12_000_000, n)            # ages up to 12 s: around every class's TTL
    t[rng.random(n) < 0.15] = ABSENT
    ttl = TTL_MS[cls]
    dead = (t == ABSENT) | (t < 1000 * (ts // 1000 - ttl))
    age = np.where(t == ABSENT, -1, ts - t)
    mid = (age > 2_000_000) & (age < 8_000_000)        # lapsed for classes 2 and 3 only
    assert dead[mid & (cls >= 2)].all() and not dead[mid & (cls < 2)].any()
    assert (mid & (cls >= 2)).sum() > 100 and (mid & (cls < 2)).sum() > 100
    eng = _engine(n)
    _set_all(eng, cls)
    eng.import_state(v, t)
    first, count = 3, 4_001
    buf = torch.full((count + 64,), 0xAA, dtype=torch.uint8, device=gpu)
    buf2 = torch.full((count,), 0xAA, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()                           # (no stream given: the buffers are complete)
    eng.expired_device(ts, buf[:count], first=first)
    eng.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[:count], dead[first:first + count].astype(np.uint8))
    assert (got[count:] == 0xAA).all()
    for k in rng.choice(n, 48, replace=False).tolist() + np.nonzero(mid)[0][:16].tolist():
        q = eng.query(k, ts)
        assert (q is None) == bool(dead[k]), k
        if q is not None:
            assert q[0] == v[k]
        assert (eng.query(k) is None) == (t[k] == ABSENT)
    d_ids, d_v, d_t = eng.export_live(ts)
    live = np.nonzero(~dead)[0]
    assert np.array_equal(d_ids.cpu().numpy(), live)
    assert np.array_equal(d_v.cpu().numpy().view(np.uint64), v[live].view(np.uint64))
    assert np.array_equal(d_t.cpu().numpy(), t[live])
    d_ids, _, _ = eng.export_live(-1)                  # no lapse test: every present row
    assert np.array_equal(d_ids.cpu().numpy(), np.nonzero(t != ABSENT)[0])
    # clear: the lapsed rows of the range become absent, the others and the classes stay
    eng.expired_device(ts, buf2, first=first, clear=True)
    eng.synchronize()
    assert np.array_equal(buf2.cpu().numpy(), got[:count])
    v2, t2 = eng.export_state()
    cleared = np.zeros(n, dtype=bool)
    cleared[first:first + count] = dead[first:first + count]
    assert (t2[cleared] == ABSENT).all()
    assert np.array_equal(t2[~cleared], t[~cleared])
    assert np.array_equal(v2[~cleared & (t != ABSENT)].view(np.uint64), v[~cleared & (t != ABSENT)].view(np.uint64))
    assert np.array_equal(eng.get_class(np.arange(n, dtype=np.uint64)), cls)
    eng.close()


# ---------------------------------------------------------------- 6. directory reuse
def test_reused_id_starts_from_its_new_class(engine_lib, gpu):
    from distributedratelimiting.redis_amd.strdir import StringDirectory
    eng = _engine(64)
    sd = StringDirectory(64, 4096, prefix="rl:", device=0)
    ids = sd.assign_host(["alpha", "beta"])
    eng.set_class(ids, [2, 0])                         # alpha: TokenLimit 100, TTL 1 s; beta: 10, 10 s
    g, r = eng.acquire_batch(ids, [30, 4], [T0, T0])
    assert g.tolist() == [1, 1] and r.tolist() == [70, 6]
    later = T0 + 3_000_000                             # alpha's bucket is gone, beta's is not
    assert sd.reclaim(eng, later) == 1
    new = sd.assign_host(["gamma"])
    assert new[0] == ids[0], "the reclaimed id goes to the next new name"
    assert eng.get_class(new).tolist() == [2]          # the reclaim leaves the class alone
    eng.set_class(new, [3])                            # gamma's plan: TokenLimit 5
    g, r = eng.acquire_batch([new[0], ids[1]], [1, 1], [later, later])
    assert g.tolist() == [1, 1]
    assert r.tolist() == [4, 8], "gamma starts from class 3's full bucket; beta refilled 3 tokens"
    sd.close()
    eng.close()


# ---------------------------------------------------------------- 7. layout and refusals
def test_layout_snapshot_refusal_and_recreate(engine_lib, gpu, tmp_path):
    from distributedratelimiting.redis_amd import snapshot
    n = 70_000
    eng = _engine(n)
    lay = eng.layout()
    assert not lay["packed"] and not lay["hot"] and not lay["narrow"]     # tbe_layout bits 0, 1, 3
    with pytest.raises(ValueError, match="classes"):
        snapshot.save(str(tmp_path / "classed.npz"), eng, T0)
    assert not (tmp_path / "classed.npz").exists()
    _set_all(eng, np.full(n, 3, dtype=np.uint8))
    eng.close()
    eng = _engine(n)                                   # most likely over the same device memory
    assert not eng.get_class(np.arange(n, dtype=np.uint64)).any()
    g, r = eng.acquire_batch([5, n - 1], [1, 1], [T0, T0])
    assert r.tolist() == [9, 9]                        # class 0's TokenLimit 10
    eng.close()
