"""Host half of the portable snapshots (distributedratelimiting.redis_amd/snapshot.py): the
live rule in numpy, the .npz layout, and the checks ``load`` makes before it touches a
device -- option mismatch, duplicate keys across shards, the owner filter.  No GPU."""
import types

import numpy as np
import pytest

from distributedratelimiting.redis_amd import _capi, snapshot
from distributedratelimiting.redis_amd.cluster import balanced_owner_map, key_owner

ABSENT = np.iinfo(np.int64).min
TS = 1_760_000_100_000_123
TTL_MS = 3_000                      # limit 5 at 2 tokens per second: ceil(2.5) s


def _engine(token_limit=5, tokens=2, ticks=10_000_000, kind=_capi.TBE_KIND_TOKEN_BUCKET):
    """What ``load`` reads of an engine before any device work: its config."""
    return types.SimpleNamespace(config=_capi.make_config(1 << 20, token_limit, tokens, ticks, kind=kind, device=0))


def test_live_rows_on_the_edges():
    ms = TS // 1000
    t = np.array([ABSENT,                              # 0 absent
                  (ms - TTL_MS) * 1000,                # 1 first microsecond of the last live millisecond
                  (ms - TTL_MS) * 1000 + 7,            # 2 same millisecond: live
                  (ms - TTL_MS - 1) * 1000 + 999,      # 3 one microsecond earlier: lapsed
                  TS + 5_000_000,                      # 4 t_us > ts_us: live
                  0,                                   # 5 the epoch: lapsed
                  TS], dtype=np.int64)                 # 6 granted at ts_us itself
    v = np.arange(t.shape[0], dtype=np.float64)
    got = snapshot.live_rows(v, t, TS, TTL_MS)
    assert got.dtype == np.int64 and got.tolist() == [1, 2, 4, 6]
    # the complement of the dead rule of tbe_expired_device, row for row
    dead = (t == ABSENT) | (t < 1000 * (TS // 1000 - TTL_MS))
    assert np.array_equal(got, np.flatnonzero(~dead))
    # ts_us < 0: every present row, the lapse test is skipped
    assert snapshot.live_rows(v, t, -1, TTL_MS).tolist() == [1, 2, 3, 4, 5, 6]
    # a timestamp inside the same millisecond decides the same
    assert snapshot.live_rows(v, t, ms * 1000, TTL_MS).tolist() == [1, 2, 4, 6]
    assert snapshot.live_rows(v, t, ms * 1000 + 1000, TTL_MS).tolist() == [4, 6]
    assert snapshot.live_rows(v[:0], t[:0], TS, TTL_MS).shape == (0,)


def test_option_meta_states_the_engine_options():
    m = dict(zip(snapshot.META_FIELDS, snapshot.option_meta(_engine().config, TS).tolist()))
    assert m == {"version": snapshot.FORMAT_VERSION, "kind": 0, "token_limit": 5,
                 "fill_rate_bits": int(np.array([2.0]).view(np.int64)[0]), "ttl_ms": TTL_MS, "ts_us": TS}
    from oracle.semantics import fill_rate_per_second, tb_ttl_seconds
    for limit, tokens, ticks in [(1, 1, 10_000_000), (20, 10, 1_000_000), (7, 3, 70_000_001), (1000, 7, 1)]:
        mm = snapshot.option_meta(_engine(limit, tokens, ticks).config, 0)
        rate = fill_rate_per_second(tokens, ticks)
        assert int(mm[3]) == int(np.array([rate]).view(np.int64)[0])
        assert int(mm[4]) == tb_ttl_seconds(limit, rate) * 1000


def test_npz_round_trip_without_pickle(tmp_path):
    rng = np.random.default_rng(5)
    n = 1_000
    v = rng.uniform(0.0, 5.0, n)
    v[:3] = [0.0, -0.0, np.nextafter(5.0, 0.0)]         # bit patterns, not values, must survive
    t = TS - rng.integers(0, 2_000_000, n)
    meta = snapshot.option_meta(_engine().config, TS)
    keys = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    p = tmp_path / "keys.npz"
    snapshot.write(p, meta, v, t, keys=keys)
    with np.load(p, allow_pickle=False) as z:
        assert sorted(z.files) == ["keys", "meta", "t_us", "v"]
        assert z["v"].dtype == np.uint64 and z["t_us"].dtype == np.int64 and z["keys"].dtype == np.uint64
        assert z["meta"].dtype == np.int64 and z["meta"].shape == (len(snapshot.META_FIELDS),)
    s = snapshot.read(p)
    assert s["form"] == "keys" and s["meta"]["ts_us"] == TS and s["meta"]["ttl_ms"] == TTL_MS
    assert np.array_equal(s["v"].view(np.uint64), v.view(np.uint64))
    assert np.array_equal(s["t_us"], t) and np.array_equal(s["keys"], keys)
    # text form: Arrow layout, bytes trimmed to the last offset
    from distributedratelimiting.redis_amd.strdir import pack_strings
    names = [f"user-{i}" for i in range(n)]
    names[7] = ""
    buf, offs = pack_strings(names)
    p2 = tmp_path / "text.npz"
    snapshot.write(p2, meta, v, t, text=(buf, offs))
    s2 = snapshot.read(p2)
    b2, o2 = s2["text"]
    assert s2["form"] == "text" and b2.shape[0] == int(offs[-1]) and np.array_equal(o2, offs)
    assert [b2[int(o2[i]):int(o2[i + 1])].tobytes().decode() for i in (0, 7, 8, n - 1)] == \
        [names[0], "", names[8], names[-1]]
    # id form
    p3 = tmp_path / "ids"                                # a bare name is written as given
    snapshot.write(p3, meta, v, t, ids=np.arange(n))
    s3 = snapshot.read(p3)
    assert s3["form"] == "ids" and np.array_equal(s3["ids"], np.arange(n, dtype=np.uint64))
    with pytest.raises(ValueError):
        snapshot.write(tmp_path / "bad.npz", meta, v, t, keys=keys, ids=np.arange(n))
    with pytest.raises(ValueError):
        snapshot.write(tmp_path / "bad.npz", meta, v, t, keys=keys[:-1])


def _shard(tmp_path, name, keys, engine=None, **kw):
    keys = np.asarray(keys, dtype=np.uint64)
    n = keys.shape[0]
    meta = snapshot.option_meta((engine or _engine()).config, TS)
    v = np.linspace(0.0, 5.0, n)
    t = np.full(n, TS, dtype=np.int64) - np.arange(n)
    p = tmp_path / name
    if kw.get("form") == "ids":
        snapshot.write(p, meta, v, t, ids=keys)
    else:
        snapshot.write(p, meta, v, t, keys=keys)
    return p, v, t


def test_option_mismatch_raises(tmp_path):
    p, _, _ = _shard(tmp_path, "a.npz", [1, 2, 3])
    directory = types.SimpleNamespace()                  # a u64-key directory (no text_of)
    for other in (_engine(token_limit=6), _engine(tokens=3), _engine(ticks=10_000_001)):
        with pytest.raises(ValueError):
            snapshot.load([p], other, directory)
    # the key form must match the directory: u64 keys into no directory, ids into a key directory,
    # u64 keys into a string directory
    with pytest.raises(ValueError):
        snapshot.load([p], _engine(), None)
    q, _, _ = _shard(tmp_path, "ids.npz", [1, 2, 3], form="ids")
    with pytest.raises(ValueError):
        snapshot.load([q], _engine(), directory)
    with pytest.raises(ValueError):
        snapshot.load([p], _engine(), types.SimpleNamespace(text_of=None))
    # the same options pass the host checks (the queueing kind shares the rows)
    rows = snapshot.merge([p], _engine(kind=_capi.TBE_KIND_QUEUEING).config, "keys")
    assert rows["keys"].tolist() == [1, 2, 3]


def test_duplicate_key_across_shards_raises(tmp_path):
    a, _, _ = _shard(tmp_path, "a.npz", [10, 11, 12])
    b, _, _ = _shard(tmp_path, "b.npz", [20, 11, 21])
    c, _, _ = _shard(tmp_path, "c.npz", [30, 31])
    with pytest.raises(ValueError):
        snapshot.load([a, b], _engine(), types.SimpleNamespace())
    with pytest.raises(ValueError):
        snapshot.merge([a, c, a], _engine().config, "keys")
    rows = snapshot.merge([c, a], _engine().config, "keys")          # file order, then row order
    assert rows["keys"].tolist() == [30, 31, 10, 11, 12]
    # text keys are compared byte for byte
    from distributedratelimiting.redis_amd.strdir import pack_strings
    meta = snapshot.option_meta(_engine().config, TS)
    for name, strings in (("t1.npz", ["a", "bc", ""]), ("t2.npz", ["ab", "c"]), ("t3.npz", ["x", "bc"])):
        snapshot.write(tmp_path / name, meta, np.zeros(len(strings)), np.full(len(strings), TS),
                       text=pack_strings(strings))
    rows = snapshot.merge([tmp_path / "t1.npz", tmp_path / "t2.npz"], _engine().config, "text")
    blob, offs = rows["text"]
    assert blob.tobytes() == b"abcabc" and offs.tolist() == [0, 1, 3, 3, 5, 6]
    with pytest.raises(ValueError):
        snapshot.merge([tmp_path / "t1.npz", tmp_path / "t3.npz"], _engine().config, "text")


def test_owner_filter_equals_key_owner(tmp_path):
    rng = np.random.default_rng(23)
    k1 = rng.integers(0, 1 << 62, 3_000, dtype=np.uint64)
    k2 = rng.integers(1 << 62, 1 << 63, 2_000, dtype=np.uint64)
    (a, va, ta), (b, vb, tb) = _shard(tmp_path, "a.npz", k1), _shard(tmp_path, "b.npz", k2)
    keys, v, t = np.concatenate([k1, k2]), np.concatenate([va, vb]), np.concatenate([ta, tb])
    omap = balanced_owner_map(rng.integers(0, 50, 4096), 3)
    for world, owner_map in ((1, None), (2, None), (3, None), (3, omap)):
        seen = 0
        for rank in range(world):
            rows = snapshot.merge([a, b], _engine().config, "keys", owner=(rank, world, owner_map))
            keep = key_owner(keys, world, owner_map) == rank
            assert np.array_equal(rows["keys"], keys[keep])             # file order kept
            assert np.array_equal(rows["v"].view(np.uint64), v[keep].view(np.uint64))
            assert np.array_equal(rows["t_us"], t[keep])
            seen += rows["keys"].shape[0]
        assert seen == keys.shape[0]                                    # every key has exactly one owner
    with pytest.raises(ValueError):                                     # the filter needs u64 keys
        q, _, _ = _shard(tmp_path, "ids.npz", [1, 2, 3], form="ids")
        snapshot.merge([q], _engine().config, "ids", owner=(0, 2, None))
