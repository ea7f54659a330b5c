"""Portable snapshots of the approximate kind's {v, p, t} tier on the GPU:
tbe_approx_export_live_device against the numpy rule (snapshot.approx_live_rows), with and
without the skip mask, over 1024 tiles plus one row; tbe_approx_import_rows_device, whose
bad row leaves the tier untouched; and snapshot.save -> fresh engine and directory -> load,
which must decide as the uninterrupted oracle does through the later syncs."""
import ctypes

import numpy as np
import pytest

from oracle.semantics import ApproxClient, ApproxGlobalTable, approx_refresh_all

pytestmark = pytest.mark.gpu

ABSENT = np.iinfo(np.int64).min
T0 = 1_760_572_800 * 1_000_000
DAY_US = 86_400 * 1_000_000
LIMIT, TOKENS, TICKS = 5, 2, 10_000_000


def _cur(gpu):
    import torch
    return torch.cuda.current_stream(gpu).cuda_stream


def _export(eng, ts, gpu, first=0, count=None, skip=None, capacity=None, pad=0):
    """One device call into sentinel-filled buffers of capacity + pad rows."""
    import torch
    count = eng.n_keys - first if count is None else count
    cap = count if capacity is None else capacity
    ids = torch.full((cap + pad,), -7, dtype=torch.int64, device=gpu)
    v = torch.full((cap + pad,), -7.0, dtype=torch.float64, device=gpu)
    p = torch.full((cap + pad,), -7.0, dtype=torch.float64, device=gpu)
    t = torch.full((cap + pad,), -7, dtype=torch.int64, device=gpu)
    n = torch.full((1,), -7, dtype=torch.int64, device=gpu)
    d_skip = None if skip is None else torch.from_numpy(skip).to(gpu)
    if cap == 0:
        eng.export_live_device(ts, None, None, None, n, first, count, 0, _cur(gpu), d_skip=d_skip, tier=True)
    else:
        eng.export_live_device(ts, ids, v, t, n, first, count, cap, _cur(gpu), d_p=p, d_skip=d_skip)
    torch.cuda.synchronize()
    return int(n.item()), ids.cpu().numpy(), v.cpu().numpy(), p.cpu().numpy(), t.cpu().numpy()


def test_export_over_two_scan_rounds(engine_lib, gpu):
    import torch
    from distributedratelimiting.redis_amd import ApproximateEngine, snapshot
    n = 2_097_153                                   # 1024 tiles of 2048 rows, and one row
    rng = np.random.default_rng(7)
    kind = rng.integers(0, 4, n)
    t = np.where(kind == 0, ABSENT, np.where(kind == 1, T0 - DAY_US - rng.integers(1_000, 10 ** 9, n),
                                             T0 - rng.integers(0, DAY_US - 1_000, n)))
    t[[0, n - 1, 2047, 2048]] = T0 - 5                # live rows on the tile edges and in the last tile
    v = rng.uniform(0.0, 5.0, n)
    p = rng.uniform(0.0, 2.0, n)
    with torch.cuda.stream(torch.cuda.Stream(gpu)):
        eng = ApproximateEngine(n, LIMIT, TOKENS, TICKS, 1, zero_wait_slots=1, device=0)
        eng.import_global(v, p, t)
        live = snapshot.approx_live_rows(t, T0)
        assert 0.4 * n < live.shape[0] < 0.6 * n and live[-1] == n - 1
        got_n, ids, gv, gp, gt = _export(eng, T0, gpu)
        assert got_n == live.shape[0]
        assert np.array_equal(ids[:got_n], live) and (ids[got_n:] == -7).all()
        for got, src in ((gv, v), (gp, p), (gt, t)):
            assert np.array_equal(got[:got_n].view(np.uint64), src[live].view(np.uint64))
            assert (got[got_n:] == -7).all()
        # with a skip mask
        skip = (rng.integers(0, 3, n) == 0).astype(np.uint8)
        skip[n - 1] = 1
        want = snapshot.approx_live_rows(t, T0, skip=skip)
        got_n, ids, gv, gp, gt = _export(eng, T0, gpu, skip=skip)
        assert got_n == want.shape[0] and np.array_equal(ids[:got_n], want)
        assert np.array_equal(gp[:got_n].view(np.uint64), p[want].view(np.uint64))
        # capacity 0 only counts; capacity < n_live fills exactly capacity rows
        assert _export(eng, T0, gpu, capacity=0)[0] == live.shape[0]
        assert _export(eng, T0, gpu, capacity=0, skip=skip)[0] == want.shape[0]
        cap = 1_000_001
        got_n, ids, gv, gp, gt = _export(eng, T0, gpu, capacity=cap, pad=4096)
        assert got_n == live.shape[0] and np.array_equal(ids[:cap], live[:cap])
        assert np.array_equal(gt[:cap], t[live[:cap]]) and np.array_equal(gv[:cap].view(np.uint64),
                                                                          v[live[:cap]].view(np.uint64))
        assert (ids[cap:] == -7).all() and (gv[cap:] == -7).all() and (gp[cap:] == -7).all() and (gt[cap:] == -7).all()
        # ts_us < 0: every present row; a sub-range that starts and ends inside tiles
        assert _export(eng, -1, gpu, capacity=0)[0] == int((t != ABSENT).sum())
        first, count = 2047, 4099
        sub = snapshot.approx_live_rows(t[first:first + count], T0, skip=skip[first:first + count]) + first
        got_n, ids, *_ = _export(eng, T0, gpu, first=first, count=count, skip=skip[first:first + count].copy())
        assert got_n == sub.shape[0] and np.array_equal(ids[:got_n], sub)
        # the host form
        hn = ctypes.c_uint64()
        hi, hv, hp, ht = (np.zeros(3000, dtype=d) for d in (np.uint64, np.float64, np.float64, np.int64))
        hskip = skip[:5000].copy()
        eng._check(eng._lib.tbe_approx_export_live(eng.handle, T0, 0, 5000, hskip.ctypes.data, hi.ctypes.data,
                                                   hv.ctypes.data, hp.ctypes.data, ht.ctypes.data, 3000,
                                                   ctypes.byref(hn)))
        w = snapshot.approx_live_rows(t[:5000], T0, skip=hskip)
        m = min(hn.value, 3000)
        assert hn.value == w.shape[0] and np.array_equal(hi[:m].astype(np.int64), w[:m])
        assert np.array_equal(hp[:m], p[w[:m]])
        eng.close()


def test_import_rows_and_bad_rows(engine_lib, gpu):
    import torch
    from distributedratelimiting.redis_amd import ApproximateEngine, TokenBucketEngine, _capi
    n = 5_000
    rng = np.random.default_rng(9)
    with torch.cuda.stream(torch.cuda.Stream(gpu)):
        eng = ApproximateEngine(n, LIMIT, TOKENS, TICKS, 4, device=0)
        torch.cuda.synchronize()
        eng.acquire_batch(rng.integers(0, n, 6000).astype(np.uint64), np.ones(6000, np.int32), wait=False)
        eng.refresh(T0)                                # one client: the views are derived
        v0, p0, t0 = eng.export_global()
        ids = rng.permutation(n)[:3000].astype(np.int64)
        watch = ids[1:4].tolist()                      # rows the import rewrites (none of them absent)
        view0 = [eng.local_state(k) for k in watch]
        v = rng.uniform(0.0, 5.0, 3000)
        p = rng.uniform(0.0, 2.0, 3000)
        t = T0 - rng.integers(0, 9_000_000, 3000)
        t[::5] = ABSENT
        dev = lambda a: torch.from_numpy(a).to(gpu)
        # a bad row (id out of range; then a negative time) voids the whole call
        for bad_ids, bad_t in ((np.concatenate([ids[:-1], [n]]), t), (ids, np.concatenate([t[:-1], [-5]]))):
            eng.import_rows(dev(bad_ids), dev(v), dev(bad_t), stream=_cur(gpu), d_p=dev(p))
            with pytest.raises(_capi.TbeError) as ei:
                eng.synchronize()
            assert ei.value.status == _capi.TBE_EINVAL
            for a, b in zip(eng.export_global(), (v0, p0, t0)):
                assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
            eng.synchronize()                          # the flag is cleared
        eng.refresh(T0)                                # (derived views again)
        v0, p0, t0 = eng.export_global()
        eng.import_rows(dev(ids), dev(v), dev(t), stream=_cur(gpu), d_p=dev(p))
        eng.synchronize()
        v1, p1, t1 = eng.export_global()
        ev, ep, et = v0.copy(), p0.copy(), t0.copy()
        ev[ids], ep[ids], et[ids] = np.where(t == ABSENT, 0.0, v), np.where(t == ABSENT, 0.0, p), t
        for a, b in zip((v1, p1, t1), (ev, ep, et)):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        # the client views are in-process state: the import does not touch them
        assert [eng.local_state(k) for k in watch] == view0
        # host form: TBE_EINVAL at once, nothing written; and a good call
        hid = np.array([3, n], dtype=np.uint64)
        two = np.zeros(2)
        st = eng._lib.tbe_approx_import_rows(eng.handle, hid.ctypes.data, two.ctypes.data, two.ctypes.data,
                                             np.array([T0, T0], dtype=np.int64).ctypes.data, 2)
        assert st == _capi.TBE_EINVAL
        assert eng.export_global(3, 1)[2][0] == et[3]
        hid[1] = 4
        ht = np.array([T0 + 1, ABSENT], dtype=np.int64)
        hv, hp = np.array([1.25, 9.0]), np.array([0.5, 9.0])
        eng._check(eng._lib.tbe_approx_import_rows(eng.handle, hid.ctypes.data, hv.ctypes.data, hp.ctypes.data,
                                                   ht.ctypes.data, 2))
        gv, gp, gt = eng.export_global(3, 2)
        assert (gv.tolist(), gp.tolist(), gt.tolist()) == ([1.25, 0.0], [0.5, 0.0], [T0 + 1, ABSENT])
        # another kind of engine refuses both calls
        tb = TokenBucketEngine(64, LIMIT, TOKENS, TICKS, device=0)
        cnt = torch.full((1,), -7, dtype=torch.int64, device=gpu)
        assert tb._lib.tbe_approx_export_live_device(tb.handle, T0, 0, 64, None, None, None, None, None, 0,
                                                     cnt.data_ptr(), _cur(gpu)) == _capi.TBE_EINVAL
        assert tb._lib.tbe_approx_import_rows_device(tb.handle, dev(ids).data_ptr(), dev(v).data_ptr(),
                                                     dev(p).data_ptr(), dev(t).data_ptr(), 8,
                                                     _cur(gpu)) == _capi.TBE_EINVAL
        torch.cuda.synchronize()
        assert int(cnt.item()) == -7
        tb.close()
        eng.close()


def test_save_load_continues_as_the_uninterrupted_oracle(engine_lib, gpu, tmp_path):
    import torch
    from distributedratelimiting.redis_amd import ApproximateEngine, _capi, snapshot
    from distributedratelimiting.redis_amd.strdir import StringDirectory, to_device
    cap, n_names = 64, 40
    rng = np.random.default_rng(13)
    client = ApproxClient(LIMIT, TOKENS, TICKS, 4, 0)
    table = ApproxGlobalTable(client.decay_rate)
    pool = list(range(n_names))

    def batch(eng, sd):
        req = pool + rng.choice(pool, 200).tolist()
        rng.shuffle(req)
        permits = rng.choice([0, 1, 1, 2, 3], len(req)).astype(np.int32)
        buf, offs, nb = to_device([f"user-{x}" for x in req], gpu)
        ids = sd.assign(buf, offs, nb).cpu().numpy()
        st, av, _ = eng.acquire_batch(ids.astype(np.uint64), permits, wait=False)
        exp = [(client.acquire(nm, p), client.available(client.st(nm))) for nm, p in zip(req, permits.tolist())]
        assert st.tolist() == [e[0] for e in exp] and av.tolist() == [e[1] for e in exp]
        return dict(zip(req, ids.tolist()))

    def sync(eng, held, ts):
        eng.refresh(ts)
        approx_refresh_all([client], table, ts, 0, sorted(held))
        v, p, t = eng.export_global()
        for nm, i in held.items():
            s = client.st(nm)
            assert eng.local_state(i) == (s.local, s.global_, s.est, client.available(s), 0), nm
            row = table.state[f"approx:{nm}"]
            assert (v[i], p[i], t[i]) == (row.v, row.p, row.t_us), nm

    with torch.cuda.stream(torch.cuda.Stream(gpu)):
        eng = ApproximateEngine(cap, LIMIT, TOKENS, TICKS, 4, device=0)
        sd = StringDirectory(cap, 1 << 16, prefix="inst:", device=0)
        held = batch(eng, sd)
        sync(eng, held, T0)
        sync(eng, held, T0 + 900_000)
        held = batch(eng, sd)
        sync(eng, held, T0 + 2_000_000)                # every local score is 0 again: nothing unsaved
        path = tmp_path / "approx.npz"
        assert snapshot.save(path, eng, T0 + 2_000_000, directory=sd) == n_names    # not the 24 unheld ids
        s = snapshot.read(path)
        assert s["form"] == "text" and s["meta"]["kind"] == _capi.TBE_KIND_APPROXIMATE
        assert s["meta"]["ttl_ms"] == 86_400_000 and s["p"].shape == (n_names,)
        ids_path = tmp_path / "ids.npz"
        assert snapshot.save(ids_path, eng, -1) == cap                              # by id: every synced row
        eng.close()
        sd.close()

        # a fresh engine behind a fresh directory, names met in another order
        eng2 = ApproximateEngine(cap, LIMIT, TOKENS, TICKS, 4, device=0)
        sd2 = StringDirectory(cap, 1 << 16, prefix="inst:", device=0)
        buf, offs, nb = to_device(["user-39", "someone-else"], gpu)
        sd2.assign(buf, offs, nb)
        with pytest.raises(ValueError):
            snapshot.load(path, eng2, directory=sd2, owner=(0, 2, None))
        tb_like = ApproximateEngine(cap, LIMIT, TOKENS + 1, TICKS, 4, device=0)
        with pytest.raises(ValueError):
            snapshot.load(path, tb_like, directory=sd2)
        tb_like.close()
        assert snapshot.load(path, eng2, directory=sd2) == n_names
        eng2.synchronize()
        buf, offs, nb = to_device([f"user-{x}" for x in pool], gpu)
        held2 = dict(zip(pool, sd2.lookup(buf, offs, nb).cpu().numpy().tolist()))
        assert held2 != held
        v, p, t = eng2.export_global()
        for nm, i in held2.items():
            row = table.state[f"approx:{nm}"]
            assert (v[i], p[i], t[i]) == (row.v, row.p, row.t_us), nm
        # the views are rebuilt by the next sync; from then on it decides as the oracle that never stopped
        sync(eng2, held2, T0 + 3_000_000)
        assert batch(eng2, sd2) == held2
        sync(eng2, held2, T0 + 4_100_000)
        batch(eng2, sd2)
        sync(eng2, held2, T0 + 5_000_000)
        eng2.close()
        sd2.close()
