"""The id rule of a reclaimed string directory on its host mirror (include/tbe_strdir.h):
freed ids are pushed in ascending order and popped before fresh counters, kept ids
survive, size() is the live count, and a mirror that is never reclaimed hands out the
ids it always did."""
import numpy as np

from distributedratelimiting.redis_amd.cluster import MASK64, scramble_walk
from distributedratelimiting.redis_amd.strdir import HostStringDirectory


def _walk(lo, hi, cap):
    return scramble_walk(np.arange(lo, hi, dtype=np.uint64), cap)


def test_never_reclaimed_ids_are_the_counter_walk():
    rng = np.random.default_rng(1)
    cap = 1_000
    h = HostStringDirectory(cap)
    first = {}
    for _ in range(5):
        s = [b"k%d" % k for k in rng.integers(0, 700, 400)]
        got = h.assign(s)
        for k in s:
            first.setdefault(k, len(first))
        want = scramble_walk(np.array([first[k] for k in s], dtype=np.uint64), cap)
        assert np.array_equal(got, want)
    assert h.size() == len(first) == h.fresh and h.free == []


def test_freed_ids_pushed_ascending_popped_lifo_before_fresh():
    cap = 64
    h = HostStringDirectory(cap)
    ids = h.assign([b"s%d" % k for k in range(10)])
    assert np.array_equal(ids, _walk(0, 10, cap))
    dead = [int(ids[7]), int(ids[2]), int(ids[5]), 9_999]     # unordered, one id never assigned
    assert h.reclaim(dead) == 3
    assert h.free == sorted(int(ids[k]) for k in (2, 5, 7))
    assert h.size() == 7
    assert np.array_equal(h.lookup([b"s2", b"s5", b"s7"]), np.full(3, MASK64, dtype=np.uint64))
    assert np.array_equal(h.lookup([b"s0", b"s9"]), ids[[0, 9]])
    # five new strings (one repeated, one known): the three freed ids from the top of the
    # stack, then fresh counters 10 and 11
    got = h.assign([b"n0", b"s0", b"n1", b"n0", b"n2", b"n3", b"n4"])
    top = sorted((int(ids[k]) for k in (2, 5, 7)), reverse=True)
    fresh = _walk(10, 12, cap).tolist()
    assert got.tolist() == [top[0], int(ids[0]), top[1], top[0], top[2], fresh[0], fresh[1]]
    assert h.free == [] and h.fresh == 12 and h.size() == 12
    # a removed string that comes back is a new string
    assert h.assign([b"s5"])[0] == _walk(12, 13, cap)[0]


def test_keep_ids_survive_until_not_kept():
    cap = 32
    h = HostStringDirectory(cap)
    ids = h.assign([b"a", b"b", b"c"])
    assert h.reclaim(ids.tolist(), keep_ids=[int(ids[1])]) == 2
    assert h.lookup([b"b"])[0] == ids[1] and h.size() == 1
    assert h.reclaim(ids.tolist()) == 1
    assert h.size() == 0 and h.free == sorted(int(ids[k]) for k in (0, 2)) + [int(ids[1])]


def test_room_counts_the_free_stack():
    cap = 8
    h = HostStringDirectory(cap)
    ids = h.assign([b"k%d" % k for k in range(8)])
    assert h.size() == 8 and not h.overflow
    assert h.reclaim([int(ids[3]), int(ids[6])]) == 2
    got = h.assign([b"x", b"y", b"z"])                  # room for two only
    assert h.overflow
    assert sorted(got[:2].tolist()) == sorted([int(ids[3]), int(ids[6])]) and got[2] == MASK64
    assert h.size() == 8


def test_reclaim_of_nothing_changes_nothing():
    h = HostStringDirectory(16)
    assert h.reclaim([0, 1, 2]) == 0 and h.size() == 0
    ids = h.assign([b"p", b"q"])
    assert h.reclaim([]) == 0
    assert np.array_equal(h.assign([b"q", b"p", b"r"]), np.concatenate([ids[::-1], _walk(2, 3, 16)]))


def test_stack_then_counter_and_overflow_same_rule_as_u64_directory():
    """Reclaim, a batch that empties the stack and goes on with the counter, an overflow and
    another reclaim: strings and u64 keys get the same ids at every step (one HostIdPool)."""
    from distributedratelimiting.redis_amd.cluster import HostDirectory
    cap = 4_096
    rng = np.random.default_rng(5)
    hs, hu = HostStringDirectory(cap), HostDirectory(cap)

    def both(nums):
        ids = hu.assign(np.asarray(nums, dtype=np.uint64))
        assert np.array_equal(hs.assign([b"user-%d" % k for k in nums]), ids)
        return ids

    ids = both(list(range(1_500)))
    vid = rng.permutation(ids.astype(np.int64))[:700].tolist()
    assert hs.reclaim(vid) == hu.reclaim(vid) == 700 and hs.free == hu.free
    surv = [k for k in range(1_500) if k in hu.ids]
    batch = rng.permutation(list(range(10_000, 12_000)) + list(range(10_000, 10_600)) + surv[:400]).tolist()
    both(batch)
    assert hs.free == [] and hs.fresh == hu.fresh == 2_800 and hs.size() == hu.size() == 2_800
    over = both(list(range(20_000, 21_297)))
    assert hs.overflow and hu.overflow and over[1_295] != MASK64 and over[1_296] == MASK64
    vid = over[:50].astype(np.int64).tolist()
    assert hs.reclaim(vid) == hu.reclaim(vid) == 50 and hs.free == hu.free
    both([21_296, 21_295, 21_294])
