"""cluster.plan_text_migration on the host: the rule of a text-keyed owner-map change
(tbe_sdir_route_keys_device + tbe_migrate_out_ids_device + the text pack), against a loop
written directly from the rule."""
import numpy as np
import pytest

from distributedratelimiting.redis_amd import cluster

ABSENT = np.iinfo(np.int64).min
GAMMA = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def mix64(z: int) -> int:
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    return z ^ (z >> 31)


def py_key(text: bytes, seed: int) -> int:
    h = mix64((seed ^ len(text) * GAMMA) & M64)
    for k in range(0, len(text), 8):
        h = mix64(h ^ int.from_bytes(text[k:k + 8], "little"))
    return h


def case(world: int, rank: int, seed: int, n: int = 400):
    """Ids with unheld slots, live / lapsed / absent rows, two classes, the empty string."""
    rng = np.random.default_rng(11)
    text = [None if rng.random() < 0.2 else b"name-%d" % i + b"x" * int(rng.integers(0, 21)) for i in range(n)]
    text[3] = b""                                  # the empty string is a key like any other
    text[7] = None
    t = np.where(rng.random(n) < 0.3, ABSENT, 1_000_000 + rng.integers(0, 1000, n)).astype(np.int64)
    v = rng.random(n) * 5
    cls = rng.integers(0, 2, n).astype(np.uint8)
    live = (t != ABSENT) & (rng.random(n) < 0.7)   # some present rows have lapsed
    t[7], live[7] = 1_000_500, True                # an orphan: a live row whose id holds no text
    live[3] = True
    t[3] = 1_000_001
    omap = rng.integers(0, world, 4096).astype(np.uint8)
    return text, v, t, cls, live, omap


@pytest.mark.parametrize("world,rank,seed", [(3, 1, 0), (2, 0, 0xDEADBEEFCAFEF00D), (5, 4, 5)])
def test_plan_text_migration_matches_the_rule(world, rank, seed):
    text, v, t, cls, live, omap = case(world, rank, seed)
    p = cluster.plan_text_migration(text, v, t, cls, live, omap, world, rank, seed)
    # the rule, id by id
    per_dest = [[] for _ in range(world)]
    leaving = np.zeros(len(text), dtype=np.uint8)
    orphans = 0
    kinds = set()
    for i, s in enumerate(text):
        if s is None:
            orphans += bool(live[i])
            continue
        key = py_key(s, seed)
        d = int(omap[mix64(key) >> 52])
        if d == rank:
            continue
        leaving[i] = 1
        kinds.add("live" if live[i] else ("absent" if t[i] == ABSENT else "lapsed"))
        if live[i]:
            per_dest[d].append((i, key))
    assert kinds == {"live", "absent", "lapsed"} and orphans >= 1      # the case holds what it claims
    order = [x for d in range(world) for x in per_dest[d]]          # destination, then id
    ids = np.array([i for i, _ in order], dtype=np.int64)
    assert np.array_equal(p["row_ids"], ids)
    assert np.array_equal(p["rows"][:, 0].view(np.uint64), np.array([k for _, k in order], dtype=np.uint64))
    assert np.array_equal(p["rows"][:, 1], v[ids].view(np.int64))
    assert np.array_equal(p["rows"][:, 2], t[ids])
    assert np.array_equal(p["rows"][:, 3], cls[ids].astype(np.int64))
    assert np.array_equal(p["lens"], np.array([len(text[i]) for i in ids], dtype=np.int64))
    assert p["out_bytes"].tobytes() == b"".join(text[i] for i in ids)
    assert np.array_equal(p["leaving"], leaving)
    assert p["counts"].tolist() == [len(x) for x in per_dest] + [int(leaving.sum()), orphans]
    assert p["counts"][rank] == 0
    assert p["byte_counts"].tolist() == [sum(len(text[i]) for i, _ in x) for x in per_dest]
    assert p["arena_counts"].tolist() == [sum((len(text[i]) + 7) & ~7 for i, _ in x) for x in per_dest]
    assert p["arena_freed"] == sum((len(text[i]) + 7) & ~7 for i in np.flatnonzero(leaving))
    assert len({len(text[i]) % 8 for i in ids}) > 1      # lengths on and off the word boundary


def test_empty_string_is_routed_like_any_key():
    """The empty string alone: held, so it leaves exactly when its key's owner is another rank."""
    seed = 9
    d = int(cluster.key_owner(np.array([py_key(b"", seed)], dtype=np.uint64), 2)[0])
    for rank in (0, 1):
        p = cluster.plan_text_migration([b"", None], np.array([1.5, 5.0]), np.array([77, ABSENT]), None,
                                        np.array([True, False]), None, 2, rank, seed)
        assert p["counts"].tolist() == ([0, 0, 0, 0] if d == rank else [int(d == 0), int(d == 1), 1, 0])
        assert p["lens"].tolist() == ([] if d == rank else [0]) and p["out_bytes"].size == 0
        assert p["arena_freed"] == 0


def test_map_entry_out_of_range_raises():
    bad = np.zeros(4096, dtype=np.uint8)
    bad[100] = 2
    with pytest.raises(ValueError):
        cluster.plan_text_migration([b"a"], np.zeros(1), np.full(1, ABSENT), None, np.zeros(1, dtype=bool), bad, 2, 0)
