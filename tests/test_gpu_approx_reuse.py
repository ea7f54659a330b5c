"""Key reuse of the approximate limiter behind a directory, against the oracle keyed by name.

A trace runs over a directory of 64 ids: 64 names take requests and syncs, most go idle,
``reclaim_idle`` frees them, and new names reuse their ids through two more syncs and
batches.  The oracle (oracle.semantics ApproxClient + ApproxGlobalTable) knows no ids: its
state is keyed by name, a reclaimed name is dropped, and a new name gets a fresh ApproxLocal
over an absent bucket -- what the reference has for a new resourceID.  Replies, available
tokens, drain logs, client state and tier rows must be equal throughout."""
import numpy as np
import pytest

from oracle.semantics import ApproxClient, ApproxGlobalTable, approx_refresh_all, lua_max, new_t_of, wrap32

pytestmark = pytest.mark.gpu

ABSENT = np.iinfo(np.int64).min
T0 = 1_760_572_800 * 1_000_000
LIMIT, TOKENS, TICKS, QLIMIT = 5, 2, 10_000_000, 4
CAP = 64


class _Names:
    """name (an int) -> id through a StringDirectory or a DeviceDirectory."""

    def __init__(self, kind, gpu):
        from distributedratelimiting.redis_amd.cluster import DeviceDirectory
        from distributedratelimiting.redis_amd.strdir import StringDirectory
        self.kind, self.gpu = kind, gpu
        self.d = StringDirectory(CAP, 1 << 16, prefix="inst:", device=0) if kind == "string" else \
            DeviceDirectory(CAP, device=0)

    def _call(self, fn, names):
        import torch
        from distributedratelimiting.redis_amd.strdir import to_device
        if self.kind == "string":
            buf, offs, nb = to_device([f"user-{n}" for n in names], self.gpu)
            return fn(buf, offs, nb).cpu().numpy()
        keys = (np.asarray(names, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)
        return fn(torch.from_numpy(keys).to(self.gpu)).cpu().numpy()

    def assign(self, names):
        return self._call(self.d.assign, names)

    def lookup(self, names):
        return self._call(self.d.lookup, names)


def _oracle_idle(client, table, name, ts_us):
    s = client.st(name)
    if s.queue or wrap32(s.global_ + s.local) != 0:
        return False
    row = table.load(f"approx:{name}", ts_us)
    if row is None:
        return True
    return lua_max(0.0, row.v - lua_max(0.0, new_t_of(ts_us) - new_t_of(row.t_us)) * table.rate) == 0.0


@pytest.mark.parametrize("kind", ["string", "u64"])
def test_reused_ids_decide_as_new_names(engine_lib, gpu, kind):
    import torch
    from distributedratelimiting.redis_amd import ApproximateEngine
    rng = np.random.default_rng(41)
    with torch.cuda.stream(torch.cuda.Stream(gpu)):
        eng = ApproximateEngine(CAP, LIMIT, TOKENS, TICKS, QLIMIT, device=0)
        names = _Names(kind, gpu)
        client = ApproxClient(LIMIT, TOKENS, TICKS, QLIMIT, 0)
        table = ApproxGlobalTable(client.decay_rate)
        held = {}                                             # name -> id
        rid = [0]

        def batch(pool, n):
            req = list(pool) + rng.choice(pool, n - len(pool)).tolist()   # every name of the pool, then random
            rng.shuffle(req)
            permits = rng.choice([0, 1, 1, 2, 3], n).astype(np.int32)
            ids = names.assign(req)
            torch.cuda.synchronize()
            assert (ids >= 0).all() and (ids < CAP).all()
            for nm, i in zip(req, ids.tolist()):
                assert held.setdefault(nm, i) == i
            st, av, (cause, ev) = eng.acquire_batch(ids.astype(np.uint64), permits, wait=True, id_base=rid[0])
            exp_st, exp_av, exp_ev = [], [], []
            for j, (nm, p) in enumerate(zip(req, permits.tolist())):
                status, evd = client.wait(nm, p, rid[0] + j)
                exp_st.append(status)
                exp_av.append(-1 if status == 3 else client.available(client.st(nm)))
                exp_ev += [(j, x) for x in evd]
            assert st.tolist() == exp_st and av.tolist() == exp_av
            assert list(zip(cause.tolist(), ev.tolist())) == exp_ev
            rid[0] += n

        def sync(ts):
            k, i, rem = eng.refresh(ts)
            for nm in held:
                client.st(nm)                                 # (a held name is a constructed limiter)
            exp = approx_refresh_all([client], table, ts, 0, sorted(held))[0]
            name_of = {i_: nm for nm, i_ in held.items()}
            got = sorted(((name_of[kk], seq, ii) for seq, (kk, ii) in enumerate(zip(k.tolist(), i.tolist()))))
            assert [(nm, ii) for nm, _, ii in got] == exp
            v, p, t = eng.export_global()
            for nm, i_ in held.items():
                s = client.st(nm)
                assert eng.local_state(i_) == (s.local, s.global_, s.est, client.available(s), len(s.queue)), nm
                row = table.state[f"approx:{nm}"]
                assert (v[i_], p[i_], t[i_]) == (row.v, row.p, row.t_us), nm
                assert eng.queue_of(i_) == [(e.request_id, e.permits) for e in s.queue]

        first = list(range(CAP))
        batch(first, 400)
        assert len(held) == CAP
        sync(T0)
        batch(first[:16], 150)                                # the estimate is infinite: these queue
        sync(T0 + 1_300_000)
        batch(first[:24], 100)
        sync(T0 + 2_600_000)
        for s_ in (6, 10, 14, 18, 22):                        # the queues drain, then the rows decay to nothing
            sync(T0 + s_ * 1_000_000)
        batch(first[:8], 30)                                  # eight names are in use again
        ts = T0 + 22_000_000
        idle = sorted(nm for nm in held if _oracle_idle(client, table, nm, ts))
        assert len(idle) >= CAP // 4 and len(idle) < CAP      # some names stay (queued waits, tokens held)
        count, flags = names.d.reclaim_idle(eng, ts)
        torch.cuda.synchronize()
        assert int(count.item()) == len(idle)
        assert sorted(np.flatnonzero(flags.cpu().numpy()).tolist()) == sorted(held[nm] for nm in idle)
        assert (names.lookup(idle) == -1).all()
        stay = sorted(set(held) - set(idle))
        assert names.lookup(stay).tolist() == [held[nm] for nm in stay]
        freed = {held[nm] for nm in idle}
        for nm in idle:                                       # the reference: the limiter is disposed, the key gone
            del held[nm], client.keys[nm]
            table.state.pop(f"approx:{nm}", None)
        # new names reuse the ids
        fresh = list(range(100, 100 + len(idle)))
        batch(fresh + stay, 300)
        assert {held[nm] for nm in fresh} == freed
        sync(T0 + 23_000_000)
        batch(fresh + stay, 300)
        sync(T0 + 24_200_000)
        batch(fresh + stay, 200)
        assert sorted(held.values()) == list(range(CAP))
        eng.close()
        names.d.close()
