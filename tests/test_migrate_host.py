"""cluster.plan_migration on the host: the rule tbe_migrate_out_device implements, on
hand-built tables and on a random one (no GPU, no engine library)."""
import numpy as np
import pytest

from distributedratelimiting.redis_amd import cluster

NO = np.uint64(cluster.MASK64)
ABSENT = cluster.ABSENT
T0 = 1_760_000_000_000_000


def _keys_for(world, owner_map, rank, n, start=0):
    """The first n keys >= start that `owner_map` gives to `rank`."""
    k = np.arange(start, start + 64 * n * world, dtype=np.uint64)
    k = k[cluster.key_owner(k, world, owner_map) == rank]
    assert k.size >= n
    return k[:n]


def _map_b(world):
    m = cluster.hash_owner_map(world).astype(np.int64)
    m[1::2] = (m[1::2] + 1) % world
    return m.astype(np.uint8)


def _plan(keys, v=None, t=None, cls=None, live=None, owner_map=None, world=2, rank=0):
    n = len(keys)
    v = np.arange(n, dtype=np.float64) + 0.5 if v is None else v
    t = np.full(n, T0, dtype=np.int64) if t is None else t
    live = cluster.rows_live(t, -1, 0) if live is None else live
    return cluster.plan_migration(keys, v, t, cls, live, owner_map, world, rank)


def test_nothing_leaves():
    keys = _keys_for(2, None, 0, 10)
    rows, counts, leaving = _plan(keys)
    assert rows.shape == (0, 4) and counts.tolist() == [0, 0, 0, 0] and not leaving.any()
    # a single owner keeps everything, whatever the map
    rows, counts, leaving = _plan(np.arange(20, dtype=np.uint64), owner_map=np.zeros(4096, np.uint8), world=1)
    assert rows.shape == (0, 4) and counts.tolist() == [0, 0, 0] and not leaving.any()


def test_everything_leaves():
    keys = _keys_for(2, None, 1, 7)
    v = np.arange(7, dtype=np.float64) * 1.25
    t = T0 + np.arange(7, dtype=np.int64)
    rows, counts, leaving = _plan(keys, v=v, t=t, cls=np.arange(7, dtype=np.uint8))
    assert leaving.tolist() == [1] * 7 and counts.tolist() == [0, 7, 7, 0]
    assert np.array_equal(rows[:, 0].view(np.uint64), keys)
    assert np.array_equal(rows[:, 1], v.view(np.int64)) and np.array_equal(rows[:, 2], t)
    assert rows[:, 3].tolist() == list(range(7))


def test_unheld_ids_absent_and_lapsed_rows():
    stay, go = _keys_for(2, None, 0, 2), _keys_for(2, None, 1, 4)
    keys = np.array([go[0], NO, stay[0], go[1], go[2], NO, stay[1], go[3]], dtype=np.uint64)
    ttl_ms = 5000
    t = np.full(8, T0, dtype=np.int64)
    t[3] = ABSENT                      # leaving, absent
    t[4] = T0 - 6_000_000              # leaving, lapsed at T0
    t[1] = ABSENT                      # unheld, absent: no orphan
    t[5] = ABSENT
    live = cluster.rows_live(t, T0, ttl_ms)
    assert live.tolist() == [True, False, True, False, False, False, True, True]
    rows, counts, leaving = _plan(keys, t=t, live=live)
    assert leaving.tolist() == [1, 0, 0, 1, 1, 0, 0, 1]          # flagged ...
    assert rows[:, 0].view(np.uint64).tolist() == [go[0], go[3]]   # ... not sent
    assert counts.tolist() == [0, 2, 4, 0]
    # without the lapse test the lapsed row travels, the absent one still does not
    rows, counts, _ = _plan(keys, t=t, live=cluster.rows_live(t, -1, ttl_ms))
    assert rows[:, 0].view(np.uint64).tolist() == [go[0], go[2], go[3]] and counts.tolist() == [0, 3, 4, 0]


def test_orphan_row_is_counted_not_sent():
    go = _keys_for(2, None, 1, 2)
    keys = np.array([go[0], NO, go[1]], dtype=np.uint64)
    rows, counts, leaving = _plan(keys)            # every row live, the unheld id's too
    assert counts.tolist() == [0, 2, 2, 1] and leaving.tolist() == [1, 0, 1]
    assert rows[:, 0].view(np.uint64).tolist() == go.tolist()


def test_bad_map_and_arguments_are_refused():
    keys = np.arange(10, dtype=np.uint64)
    bad = cluster.hash_owner_map(2).copy()
    bad[17] = 2
    with pytest.raises(ValueError):
        _plan(keys, owner_map=bad)
    with pytest.raises(ValueError):
        _plan(keys, owner_map=bad[:100])
    with pytest.raises(ValueError):
        _plan(keys, world=2, rank=2)
    with pytest.raises(ValueError):
        _plan(keys, world=257, rank=0)
    with pytest.raises(ValueError):
        cluster.plan_migration(keys, np.zeros(9), np.zeros(10, np.int64), None, np.ones(10, bool), None, 2, 0)


def test_row_order_destination_major_id_ascending():
    world, rank = 4, 2
    rng = np.random.default_rng(5)
    keys = rng.permutation(np.arange(400, dtype=np.uint64))
    rows, counts, leaving = _plan(keys, owner_map=_map_b(world), world=world, rank=rank)
    dest = cluster.key_owner(rows[:, 0].view(np.uint64), world, _map_b(world))
    assert np.all(np.diff(dest) >= 0) and rank not in dest.tolist() and len(set(dest.tolist())) == world - 1
    ids = {int(k): i for i, k in enumerate(keys.tolist())}
    for o in range(world):
        got = [ids[int(k)] for k in rows[dest == o, 0].view(np.uint64).tolist()]
        assert got == sorted(got) and len(got) == counts[o]
    assert counts[rank] == 0 and counts[world] == leaving.sum() == rows.shape[0]


@pytest.mark.parametrize("world", [2, 8])
def test_conservation_on_a_random_table(world):
    """`world` simulated ranks hold a random key set under the hash partition; after every
    rank's plan is applied, each live key sits on exactly the rank the new map names, with
    bit-identical {v, t_us, cls}, and the union of live keys is unchanged."""
    rng = np.random.default_rng(11 + world)
    new_map = _map_b(world)
    all_keys = rng.choice(1 << 40, 6000, replace=False).astype(np.uint64)
    cap, ttl_ms = 1500 if world == 8 else 4000, np.array([5000, 9000, 2000])
    ranks, truth = [], {}
    for r in range(world):
        mine = all_keys[cluster.key_owner(all_keys, world) == r]
        ids = rng.permutation(cap)[: mine.size]
        keys_of_id = np.full(cap, NO, dtype=np.uint64)
        keys_of_id[ids] = mine
        v = rng.integers(0, 1 << 62, cap).view(np.float64)
        cls = rng.integers(0, 3, cap).astype(np.uint8)
        t = T0 - rng.integers(0, 12_000_000, cap)
        t[rng.random(cap) < 0.2] = ABSENT
        t[keys_of_id == NO] = ABSENT                        # no orphans
        live = cluster.rows_live(t, T0, ttl_ms[cls])
        for i in np.flatnonzero(live & (keys_of_id != NO)).tolist():
            truth[int(keys_of_id[i])] = (int(v[i:i + 1].view(np.int64)[0]), int(t[i]), int(cls[i]))
        ranks.append(dict(keys=keys_of_id, v=v, t=t, cls=cls, live=live))
    assert len(truth) > 2000
    held = [dict() for _ in range(world)]      # rank -> key -> row, after the migration
    moved = 0
    for r, s in enumerate(ranks):
        rows, counts, leaving = cluster.plan_migration(s["keys"], s["v"], s["t"], s["cls"], s["live"], new_map,
                                                       world, r)
        assert counts[world + 1] == 0 and counts[:world].sum() == rows.shape[0]
        for i in np.flatnonzero((leaving == 0) & s["live"] & (s["keys"] != NO)).tolist():   # what stays
            held[r][int(s["keys"][i])] = (int(s["v"][i:i + 1].view(np.int64)[0]), int(s["t"][i]), int(s["cls"][i]))
        at = np.concatenate([[0], np.cumsum(counts[:world])])
        for o in range(world):
            for k, vb, tt, c in rows[at[o]:at[o + 1]].tolist():
                key = int(np.int64(k).view(np.uint64)) if k < 0 else k
                assert key not in held[o]
                held[o][key] = (vb, tt, c)
                moved += 1
    assert moved > 800
    seen = {}
    for r in range(world):
        for key, row in held[r].items():
            assert key not in seen and int(cluster.key_owner(np.array([key], np.uint64), world, new_map)[0]) == r
            seen[key] = row
    assert seen == truth
