"""The id rule of a reclaimed u64 key directory on its host mirror (include/tbe_cluster.h,
cluster.HostDirectory): freed ids are pushed in ascending order and popped before fresh
counters, kept ids survive, room counts the free stack, the overflow state is sticky, and a
mirror that is never reclaimed hands out the ids it always did."""
import numpy as np
import pytest

from distributedratelimiting.redis_amd import _capi
from distributedratelimiting.redis_amd.cluster import MASK64, HostDirectory, scramble_walk


def _walk(lo, hi, cap):
    return scramble_walk(np.arange(lo, hi, dtype=np.uint64), cap)


def _keys(*ks):
    return np.array(ks, dtype=np.uint64)


def test_never_reclaimed_ids_are_the_counter_walk():
    rng = np.random.default_rng(1)
    cap = 1_000
    h = HostDirectory(cap)
    first = {}
    for _ in range(5):
        keys = rng.integers(0, 700, 400).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        got = h.assign(keys)
        for k in keys.tolist():
            first.setdefault(k, len(first))
        want = scramble_walk(np.array([first[k] for k in keys.tolist()], dtype=np.uint64), cap)
        assert np.array_equal(got, want)
    assert h.size() == len(first) == h.fresh and h.free == [] and not h.overflow
    # counters 0..n-1 through the bijection, each id once
    assert sorted(h.ids.values()) == sorted(_walk(0, len(first), cap).tolist())


def test_never_reclaimed_overflow_is_at_capacity():
    cap = 8
    h = HostDirectory(cap)
    assert np.array_equal(h.assign(np.arange(100, 106, dtype=np.uint64)), _walk(0, 6, cap))
    got = h.assign(_keys(200, 100, 201, 202))            # two ids remain
    assert h.overflow and got.tolist() == [int(_walk(6, 7, cap)[0]), int(_walk(0, 1, cap)[0]),
                                           int(_walk(7, 8, cap)[0]), MASK64]
    assert h.size() == 8 and h.fresh == 8
    with pytest.raises(_capi.TbeError) as ei:
        h.check()
    assert ei.value.status == _capi.TBE_ERANGE


def test_freed_ids_pushed_ascending_popped_lifo_before_fresh():
    cap = 64
    h = HostDirectory(cap)
    ids = h.assign(np.arange(1_000, 1_010, dtype=np.uint64))
    assert np.array_equal(ids, _walk(0, 10, cap))
    dead = [int(ids[7]), int(ids[2]), int(ids[5]), 9_999]     # unordered, one id never assigned
    assert h.reclaim(dead) == 3
    assert h.free == sorted(int(ids[k]) for k in (2, 5, 7))
    assert h.size() == 7 and h.fresh == 10
    assert np.array_equal(h.lookup(_keys(1_002, 1_005, 1_007)), np.full(3, MASK64, dtype=np.uint64))
    assert np.array_equal(h.lookup(_keys(1_000, 1_009)), ids[[0, 9]])
    # five new keys (one repeated, one known) in one batch: the three freed ids from the top
    # of the stack, then fresh counters 10 and 11
    got = h.assign(_keys(50, 1_000, 51, 50, 52, 53, 54))
    top = sorted((int(ids[k]) for k in (2, 5, 7)), reverse=True)
    fresh = _walk(10, 12, cap).tolist()
    assert got.tolist() == [top[0], int(ids[0]), top[1], top[0], top[2], fresh[0], fresh[1]]
    assert h.free == [] and h.fresh == 12 and h.size() == 12
    # a removed key that comes back is a new key
    assert h.assign(_keys(1_005))[0] == _walk(12, 13, cap)[0]


def test_second_reclaim_stacks_on_the_first():
    cap = 32
    h = HostDirectory(cap)
    ids = h.assign(np.arange(6, dtype=np.uint64)).tolist()
    assert h.reclaim([ids[4]]) == 1
    assert h.reclaim([ids[1], ids[3]]) == 2
    assert h.free == [ids[4]] + sorted([ids[1], ids[3]])
    got = h.assign(_keys(70, 71)).tolist()                 # the later reclaim's ids first, highest first
    assert got == sorted([ids[1], ids[3]], reverse=True) and h.free == [ids[4]]


def test_keep_ids_survive_until_not_kept():
    cap = 32
    h = HostDirectory(cap)
    ids = h.assign(_keys(7, 8, 9))
    assert h.reclaim(ids.tolist(), keep_ids=[int(ids[1]), int(ids[1]), 10**6]) == 2
    assert h.lookup(_keys(8))[0] == ids[1] and h.size() == 1
    assert h.reclaim(ids.tolist()) == 1
    assert h.size() == 0 and h.free == sorted(int(ids[k]) for k in (0, 2)) + [int(ids[1])]


def test_room_counts_the_free_stack_and_overflow_is_exactly_past_it():
    cap = 8
    h = HostDirectory(cap)
    ids = h.assign(np.arange(10, 16, dtype=np.uint64))    # fresh = 6
    assert h.reclaim([int(ids[3]), int(ids[1]), int(ids[4])]) == 3
    # room = nfree + capacity - fresh = 3 + 8 - 6 = 5: five new keys fit exactly
    got = h.assign(np.arange(20, 25, dtype=np.uint64))
    assert not h.overflow and h.size() == 8 and h.free == [] and h.fresh == 8
    stack = sorted((int(ids[k]) for k in (1, 3, 4)), reverse=True)
    assert got.tolist() == stack + _walk(6, 8, cap).tolist()
    # no room: known keys still resolve, one new key overflows
    assert np.array_equal(h.assign(np.arange(20, 25, dtype=np.uint64)), got) and not h.overflow
    assert h.reclaim([int(got[0]), int(got[4])]) == 2      # room = 2 + 8 - 8 = 2
    more = h.assign(_keys(30, 31, 32))
    assert h.overflow
    assert more[:2].tolist() == sorted([int(got[0]), int(got[4])], reverse=True) and more[2] == MASK64
    assert h.size() == 8


def test_reclaim_does_not_clear_overflow():
    cap = 4
    h = HostDirectory(cap)
    ids = h.assign(np.arange(5, dtype=np.uint64))
    assert h.overflow and ids[4] == MASK64
    assert h.reclaim(ids[:4].tolist()) == 4
    assert h.overflow and h.size() == 0
    with pytest.raises(_capi.TbeError):
        h.check()
    # the freed ids are still handed out by the rule
    assert h.assign(_keys(9))[0] == max(int(i) for i in ids[:4])


def test_reclaim_of_nothing_changes_nothing():
    h = HostDirectory(16)
    assert h.reclaim([0, 1, 2]) == 0 and h.size() == 0
    ids = h.assign(_keys(3, 4))
    assert h.reclaim([]) == 0
    assert np.array_equal(h.assign(_keys(4, 3, 5)), np.concatenate([ids[::-1], _walk(2, 3, 16)]))
