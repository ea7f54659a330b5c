"""Host half of the approximate limiter's idle-key reclaim and tier snapshots
(distributedratelimiting.redis_amd/snapshot.py): ``approx_idle_rows`` and
``approx_live_rows`` against the CPU restatement of the reference (oracle.semantics), the
.npz layout with the ``p`` array, and what ``load`` refuses before it touches a device.
No GPU."""
import copy
import types

import numpy as np
import pytest

from distributedratelimiting.redis_amd import _capi, snapshot
from oracle.semantics import (ApproxGlobalState, ApproxGlobalTable, ApproxLocal, QueueEntry, fill_rate_per_second,
                              lua_max, new_t_of, wrap32)

ABSENT = np.iinfo(np.int64).min
TS = 1_760_000_100_000_123
DAY_MS = 86_400_000
RATE = fill_rate_per_second(2, 10_000_000)          # 2 tokens per second


def _oracle_idle(local: ApproxLocal, row, ts_us: int, rate: float) -> bool:
    """The three clauses on the oracle's own objects: the client's state (A:36, A:503-506)
    and what one more sync call with LocalCount 0 at ts_us would leave in the hash (A:241-268)."""
    if local.queue:
        return False
    if wrap32(local.global_ + local.local) != 0:
        return False
    if row is None:
        return True
    table = ApproxGlobalTable(rate)
    table.state["k"] = copy.copy(row)
    if table.load("k", ts_us) is None:                 # lapsed: EXPIRE 86400 (A:268)
        return True
    dt = lua_max(0.0, new_t_of(ts_us) - new_t_of(row.t_us))
    worth = lua_max(0.0, row.v - (dt * rate))
    table.sync("k", 0, ts_us)                          # the same through the script itself
    assert table.state["k"].v == worth
    return worth == 0.0


def _arrays(rows):
    loc = np.array([r[0].local for r in rows], dtype=np.int32)
    glo = np.array([r[0].global_ for r in rows], dtype=np.int32)
    que = np.array([len(r[0].queue) for r in rows], dtype=np.uint32)
    v = np.array([0.0 if r[1] is None else r[1].v for r in rows], dtype=np.float64)
    t = np.array([ABSENT if r[1] is None else r[1].t_us for r in rows], dtype=np.int64)
    return loc, glo, que, v, t


def _row(v, t_us, p=0.25):
    return ApproxGlobalState(v, p, t_us)


def test_idle_rows_on_both_sides_of_every_clause():
    ms = TS // 1000
    full = TS - 3_000_000                              # 3 s before TS: 6 tokens decay at 2 per second
    v_full = (new_t_of(TS) - new_t_of(full)) * RATE    # exactly the decay: worth 0.0
    rows = [
        (ApproxLocal(), None),                                               # 0 fresh key: idle
        (ApproxLocal(queue=[QueueEntry(7, 0)]), None),                       # 1 queued zero-permit wait
        (ApproxLocal(queue=[QueueEntry(8, 2)], qcount=2), None),             # 2 queued wait
        (ApproxLocal(local=1), None),                                        # 3 local > 0
        (ApproxLocal(global_=1), _row(0.0, full)),                           # 4 global > 0
        (ApproxLocal(local=-3, global_=3), _row(0.0, full)),                 # 5 they cancel: ConsumedTokens 0
        (ApproxLocal(local=-2 ** 31, global_=-2 ** 31), _row(0.0, full)),    # 6 and in wrapped int32
        (ApproxLocal(), _row(np.nextafter(v_full, np.inf), full)),           # 7 v just above full decay
        (ApproxLocal(), _row(v_full, full)),                                 # 8 v exactly at full decay
        (ApproxLocal(), _row(np.nextafter(v_full, 0.0), full)),              # 9 below
        (ApproxLocal(), _row(0.5, TS + 1_000_000)),                          # 10 ts_us before t: no decay
        (ApproxLocal(), _row(0.0, TS + 1_000_000)),                          # 11 ... and nothing to decay
        (ApproxLocal(), _row(1e9, (ms - DAY_MS) * 1000)),                    # 12 last live millisecond
        (ApproxLocal(), _row(1e9, (ms - DAY_MS - 1) * 1000 + 999)),          # 13 one microsecond earlier: lapsed
        (ApproxLocal(), _row(1e9, (ms - DAY_MS) * 1000 - 1000)),             # 14 lapsed by one millisecond
        (ApproxLocal(), _row(-0.0, TS)),                                     # 15 v = -0.0 at dt 0
        (ApproxLocal(local=1), _row(1e9, (ms - DAY_MS - 1) * 1000)),         # 16 lapsed row, local > 0
    ]
    want = [True, False, False, False, False, True, True, False, True, True, False, True, False, True, True, True,
            False]
    got = snapshot.approx_idle_rows(*_arrays(rows), TS, RATE)
    assert got.dtype == np.bool_ and got.tolist() == want
    assert [_oracle_idle(loc, row, TS, RATE) for loc, row in rows] == want
    # rows 12-14: the same edge through approx_live_rows (ids of the exported rows)
    t = _arrays(rows)[4]
    live = snapshot.approx_live_rows(t, TS)
    assert live.dtype == np.int64
    assert [i in live.tolist() for i in (0, 12, 13, 14, 10)] == [False, True, False, False, True]
    with pytest.raises(ValueError):
        snapshot.approx_idle_rows(*_arrays(rows), -1, RATE)


def test_idle_and_live_rows_follow_the_oracle_row_for_row():
    rng = np.random.default_rng(11)
    n = 4_000
    for rate in (RATE, fill_rate_per_second(7, 3_000_001), fill_rate_per_second(1, 864_000_000_000)):
        rows = []
        for i in range(n):
            kind = rng.integers(0, 8)
            loc = ApproxLocal()
            if kind == 0:
                loc.queue = [QueueEntry(int(i), int(rng.integers(0, 3)))]
            if kind == 1:
                loc.local = int(rng.integers(-2, 3))
            if kind == 2:
                loc.global_ = int(rng.integers(-2, 3))
                loc.local = -loc.global_ if rng.integers(0, 2) else 0
            row = None
            if rng.integers(0, 6):
                age = int(rng.choice([0, 1, 999, 1_000_000, 3_000_000, 7_654_321, DAY_MS * 1000 - 1_000_000,
                                      DAY_MS * 1000 + 122, DAY_MS * 1000 + 123, DAY_MS * 1000 + 124,
                                      DAY_MS * 1000 + 5_000_000, -2_000_000]))
                age += int(rng.integers(0, 3)) if 0 < age < DAY_MS * 1000 - 1_000_000 else 0
                t_us = TS - age
                dt = lua_max(0.0, new_t_of(TS) - new_t_of(t_us))
                v = float(rng.choice([0.0, dt * rate, np.nextafter(dt * rate, np.inf), dt * rate * 0.5,
                                      dt * rate + 1.0, 3.0]))
                row = ApproxGlobalState(v, float(rng.uniform(0, 2)), t_us)
            rows.append((loc, row))
        got = snapshot.approx_idle_rows(*_arrays(rows), TS, rate)
        want = np.array([_oracle_idle(loc, row, TS, rate) for loc, row in rows])
        assert np.array_equal(got, want)
        assert 0.1 * n < int(want.sum()) < 0.9 * n
        # live rows: the oracle's passive expiry on load
        t = _arrays(rows)[4]
        table = ApproxGlobalTable(rate)
        for i, (_, row) in enumerate(rows):
            if row is not None:
                table.state[str(i)] = copy.copy(row)
        want_live = [i for i in range(n) if table.load(str(i), TS) is not None]
        assert snapshot.approx_live_rows(t, TS).tolist() == want_live
        skip = (rng.integers(0, 3, n) == 0).astype(np.uint8)
        assert snapshot.approx_live_rows(t, TS, skip=skip).tolist() == [i for i in want_live if not skip[i]]
        assert snapshot.approx_live_rows(t, -1).tolist() == [i for i in range(n) if rows[i][1] is not None]


def _engine(token_limit=5, tokens=2, ticks=10_000_000, kind=_capi.TBE_KIND_APPROXIMATE):
    return types.SimpleNamespace(config=_capi.make_config(1 << 12, token_limit, tokens, ticks, kind=kind, device=0))


def test_option_meta_of_the_approximate_kind():
    m = dict(zip(snapshot.META_FIELDS, snapshot.option_meta(_engine().config, TS).tolist()))
    assert m == {"version": snapshot.FORMAT_VERSION, "kind": _capi.TBE_KIND_APPROXIMATE, "token_limit": 5,
                 "fill_rate_bits": int(np.array([RATE]).view(np.int64)[0]), "ttl_ms": DAY_MS, "ts_us": TS}


def test_npz_round_trip_with_p(tmp_path):
    rng = np.random.default_rng(3)
    n = 500
    v = rng.uniform(0.0, 5.0, n)
    p = rng.uniform(0.0, 2.0, n)
    v[:2] = [-0.0, np.nextafter(5.0, 0.0)]
    p[:2] = [np.nextafter(0.0, 1.0), -0.0]             # bit patterns must survive
    t = TS - rng.integers(0, 2_000_000, n)
    keys = rng.permutation(10 * n)[:n].astype(np.uint64)
    meta = snapshot.option_meta(_engine().config, TS)
    a, b = tmp_path / "a.npz", tmp_path / "b.npz"
    h = n // 2
    snapshot.write(a, meta, v[:h], t[:h], keys=keys[:h], p=p[:h])
    snapshot.write(b, meta, v[h:], t[h:], keys=keys[h:], p=p[h:])
    with np.load(a, allow_pickle=False) as z:
        assert sorted(z.files) == ["keys", "meta", "p", "t_us", "v"] and z["p"].dtype == np.uint64
    s = snapshot.read(a)
    assert s["form"] == "keys" and s["meta"]["kind"] == _capi.TBE_KIND_APPROXIMATE and s["meta"]["ttl_ms"] == DAY_MS
    assert np.array_equal(s["p"].view(np.uint64), p[:h].view(np.uint64))
    rows = snapshot.merge([a, b], _engine().config, "keys")
    assert np.array_equal(rows["keys"], keys) and np.array_equal(rows["t_us"], t)
    assert np.array_equal(rows["v"].view(np.uint64), v.view(np.uint64))
    assert np.array_equal(rows["p"].view(np.uint64), p.view(np.uint64))
    with pytest.raises(ValueError):
        snapshot.write(tmp_path / "c.npz", meta, v, t, keys=keys, p=p[:-1])
    # a token-bucket file keeps its exact format
    tb = _engine(kind=_capi.TBE_KIND_TOKEN_BUCKET)
    snapshot.write(tmp_path / "tb.npz", snapshot.option_meta(tb.config, TS), v, t, keys=keys)
    with np.load(tmp_path / "tb.npz", allow_pickle=False) as z:
        assert sorted(z.files) == ["keys", "meta", "t_us", "v"]
    assert "p" not in snapshot.read(tmp_path / "tb.npz")
    assert "p" not in snapshot.merge(tmp_path / "tb.npz", tb.config, "keys")


def test_load_refusals(tmp_path):
    n = 8
    v, p, t = np.full(n, 1.5), np.full(n, 0.5), np.full(n, TS, dtype=np.int64)
    keys = np.arange(n, dtype=np.uint64)
    apx = _engine()
    f = tmp_path / "apx.npz"
    snapshot.write(f, snapshot.option_meta(apx.config, TS), v, t, keys=keys, p=p)
    # kind mismatch, both ways
    tb = _engine(kind=_capi.TBE_KIND_TOKEN_BUCKET)
    g = tmp_path / "tb.npz"
    snapshot.write(g, snapshot.option_meta(tb.config, TS), v, t, keys=keys)
    with pytest.raises(ValueError, match="kind"):
        snapshot.merge(f, tb.config, "keys")
    with pytest.raises(ValueError, match="kind"):
        snapshot.merge(g, apx.config, "keys")
    # rate mismatch (the decay rate's bits) and limit mismatch
    with pytest.raises(ValueError, match="fill-rate"):
        snapshot.merge(f, _engine(tokens=3).config, "keys")
    with pytest.raises(ValueError):
        snapshot.merge(f, _engine(token_limit=6).config, "keys")
    # the tier is replicated: no owner filter
    with pytest.raises(ValueError, match="replicated"):
        snapshot.merge(f, apx.config, "keys", owner=(0, 2, None))
    with pytest.raises(ValueError, match="replicated"):
        snapshot.load(f, apx, directory=types.SimpleNamespace(), owner=(0, 2, None))
    # a key twice across the shards
    with pytest.raises(ValueError, match="twice"):
        snapshot.merge([f, f], apx.config, "keys")
    # key form mismatch
    with pytest.raises(ValueError):
        snapshot.merge(f, apx.config, "ids")
    assert snapshot.merge(f, apx.config, "keys")["p"].tolist() == p.tolist()
