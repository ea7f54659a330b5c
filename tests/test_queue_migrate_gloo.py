"""cluster.migrate_queueing over gloo on the CPU (worlds 2 and 8): two routed wait steps with a
tick each under the hash partition, a live change to map B that takes the queued waits along,
a routed cancel of requests queued before the move, two more steps under B.  The ranks'
engines are oracle stand-ins (tests/_queue_migrate_workers.py); the protocol is the code the
HIP engines run.

Expected: the serial reference is one oracle.semantics.QueueingTokenBucketTable per class over
global keys, which knows nothing about owners: per step rank 0's batch, then rank 1's, ...,
fed the request ids the ranks reported, then one tick.  Compared: every status and remaining,
every cancel hit, every tick log per key in drain order, the final rows and queues through the
directories, and that every key is held by exactly the owner map B names.
"""
import numpy as np
import pytest
import torch.multiprocessing as mp

from tests import _migrate_workers as M
from tests import _queue_migrate_workers as Q
from tests import test_dist_gloo as G

ABSENT = Q.ABSENT


def _spawn(fn, *args, world: int):
    mp.start_processes(fn, args=(world, G._port()) + args, nprocs=world, join=True, start_method="spawn")


class Reference:
    """The serial reference; `ids`: per (rank, step) the request ids the ranks reported, or
    None to mint its own (the decisions do not depend on the ids' values)."""

    def __init__(self, world: int, classed: bool):
        from oracle.semantics import QueueingTokenBucketTable, TokenBucketConfig
        self.world, self.classes = world, Q.classes_of(classed)
        self.nc = len(self.classes)
        self.tabs = [QueueingTokenBucketTable(TokenBucketConfig.from_options(*c[:3]), c[3], c[4]) for c in self.classes]
        self.minted = 0

    def tab(self, k):
        return self.tabs[k % self.nc]

    def step(self, s, ids=None):
        """[(status, remaining, ids)] per rank, and the tick's log [(key, id, remaining)]."""
        out = []
        for r in range(self.world):
            k, p, t = Q.batch(r, s)
            rid = np.arange(self.minted, self.minted + Q.N, dtype=np.int64) if ids is None else ids[r]
            self.minted += Q.N
            st, rem = [], []
            for kk, pp, tt, ii in zip(k.tolist(), p.tolist(), t.tolist(), rid.tolist()):
                a, b, _ = self.tab(kk).acquire(kk, pp, tt, ii)
                st.append(a)
                rem.append(b)
            out.append((np.array(st, dtype=np.uint8), np.array(rem, dtype=np.int32), rid))
        log = sorted((e for tab in self.tabs for e in tab.refresh(Q.tick_ts(s))), key=lambda e: e[0])
        return out, np.array(log, dtype=np.int64).reshape(-1, 3)

    def queue_len(self):
        return np.array([len(self.tab(k).queue_of(k)) for k in range(Q.N_KEYS)], dtype=np.int64)


def shape(world: int, classed: bool = False):
    """What the move carries, from the oracle alone: (moved keys with a non-empty queue, staying
    keys with one, entries sent per rank, entries received per rank) at migration time."""
    from distributedratelimiting.redis_amd import cluster
    ref = Reference(world, classed)
    ref.step(0)
    ref.step(1)
    qlen = ref.queue_len()
    keys = np.arange(Q.N_KEYS, dtype=np.uint64)
    old, new = cluster.key_owner(keys, world), cluster.key_owner(keys, world, M.map_b(world))
    moved = old != new
    sent = np.bincount(old[moved], weights=qlen[moved], minlength=world).astype(np.int64)
    recv = np.bincount(new[moved], weights=qlen[moved], minlength=world).astype(np.int64)
    return int((moved & (qlen > 0)).sum()), int((~moved & (qlen > 0)).sum()), sent, recv


def check_queue_migrate(res, classed: bool = False):
    from distributedratelimiting.redis_amd import cluster
    world = len(res)
    ref = Reference(world, classed)
    mb = M.map_b(world)
    keys = np.arange(Q.N_KEYS, dtype=np.uint64)
    old, new = cluster.key_owner(keys, world), cluster.key_owner(keys, world, mb)
    qlen_at_move = None
    for s in range(Q.STEPS):
        if s == 2:
            qlen_at_move = ref.queue_len()
            hits_on_moved = 0
            for r in range(world):   # the cancels of requests queued before the move
                ck, ci = [], []
                for s0 in (0, 1):
                    pick = Q.cancel_pick(res[r][f"st{s0}"])
                    ck.append(Q.batch(r, s0)[0][pick])
                    ci.append(res[r][f"ids{s0}"][pick])
                ck, ci = np.concatenate(ck), np.concatenate(ci)
                want = np.array([int(ref.tab(k).cancel(k, i)) for k, i in zip(ck.tolist(), ci.tolist())], dtype=np.uint8)
                assert np.array_equal(res[r]["hit"], want), r
                hits_on_moved += int(want[old[ck.astype(np.int64)] != new[ck.astype(np.int64)]].sum())
            assert hits_on_moved >= 50          # entries that were cancelled on their new owner
        replies, log = ref.step(s, [res[r][f"ids{s}"] for r in range(world)])
        for r in range(world):
            assert np.array_equal(res[r][f"st{s}"], replies[r][0]), (s, r)
            assert np.array_equal(res[r][f"rem{s}"], replies[r][1]), (s, r)
        got = np.concatenate([res[r][f"log{s}"] for r in range(world)])
        got = got[np.argsort(got[:, 0], kind="stable")]                # per key in drain order
        assert np.array_equal(got, log), s
        if s >= 2:
            assert len(log) >= 100
    # ids stayed unique across owners
    all_ids = np.concatenate([res[r][f"ids{s}"] for r in range(world) for s in range(Q.STEPS)])
    assert np.unique(all_ids).size == all_ids.size
    # what moved
    moved = old != new
    sent = np.array([int(x["moved"][2]) for x in res])
    recv = np.array([int(x["moved"][3]) for x in res])
    assert np.array_equal(sent, np.bincount(old[moved], weights=qlen_at_move[moved], minlength=world).astype(np.int64))
    assert np.array_equal(recv, np.bincount(new[moved], weights=qlen_at_move[moved], minlength=world).astype(np.int64))
    assert sum(int(x["moved"][0]) for x in res) == sum(int(x["moved"][1]) for x in res)
    # final rows and queues, through the directories
    seen = []
    for r in range(world):
        dk, di = res[r]["dir_keys"].astype(np.int64), res[r]["dir_ids"].astype(np.int64)
        assert np.all(cluster.key_owner(dk.astype(np.uint64), world, mb) == r)   # the new owner's keys only
        starts = np.concatenate([[0], np.cumsum(res[r]["q_count"].astype(np.int64))])
        for j, (k, i) in enumerate(zip(dk.tolist(), di.tolist())):
            st = ref.tab(k).tb.state.get(k)
            if st is None:
                assert res[r]["t"][i] == ABSENT, (r, k)
            else:
                assert res[r]["t"][i] == st.t_us and res[r]["v"][i] == st.v, (r, k)
            q = res[r]["q_entries"][starts[j]:starts[j + 1]].tolist()
            assert q == [(a << 16) | b for a, b in ref.tab(k).queue_of(k)], (r, k)
        seen.append(dk)
    seen = np.concatenate(seen)
    assert seen.size == np.unique(seen).size == Q.N_KEYS                 # every key once, none held twice
    return qlen_at_move


def check_refused(res):
    """Every rank raised, and nothing changed on any of them, queues included."""
    for r, x in enumerate(res):
        assert int(x["raised"]) == 1, r
        for name in ("v", "t", "dir_keys", "dir_ids", "dir_size", "q_count", "q_entries"):
            a, b = x[f"before_{name}"], x[f"after_{name}"]
            assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a,
                                  b.view(np.int64) if b.dtype == np.float64 else b), (r, name)
        assert x["before_q_count"].sum() > 0


SHAPES = {  # (world, classed): moved keys with a queue, staying keys with one
    (2, False): (483, 504), (8, False): (494, 506), (2, True): (473, 497),
}


@pytest.mark.parametrize("world,classed", [(2, False), (8, False), (2, True)])
def test_the_move_carries_queues(world, classed):
    """The shape of the case, from the oracle alone: at least 200 keys that change owner and
    at least 200 that stay hold queued waits at migration time, and every rank both sends and
    receives entries."""
    moved_q, stay_q, sent, recv = shape(world, classed)
    print(world, classed, moved_q, stay_q, sent.tolist(), recv.tolist())
    assert moved_q >= 200 and stay_q >= 200
    assert sent.min() > 0 and recv.min() > 0
    assert (moved_q, stay_q) == SHAPES[(world, classed)]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 8])
def test_migrate_queueing_matches_serial_reference(tmp_path, world):
    _spawn(Q.queue_migrate_worker, str(tmp_path), "ok", "plain", world=world)
    check_queue_migrate([np.load(tmp_path / f"qmig_{r}.npz") for r in range(world)])


def test_migrate_queueing_classed_matches_serial_reference(tmp_path):
    _spawn(Q.queue_migrate_worker, str(tmp_path), "ok", "classed", world=2)
    check_queue_migrate([np.load(tmp_path / f"qmig_{r}.npz") for r in range(2)], classed=True)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 8])
def test_preflight_failure_raises_everywhere_and_changes_nothing(tmp_path, world):
    _spawn(Q.queue_migrate_worker, str(tmp_path), "tight", "plain", world=world)
    check_refused([np.load(tmp_path / f"qmig_{r}.npz") for r in range(world)])


def test_migrate_queueing_refuses_what_it_does_not_cover():
    from distributedratelimiting.redis_amd import _capi, cluster
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory

    class Fake:
        KIND = _capi.TBE_KIND_TOKEN_BUCKET
    with pytest.raises(ValueError, match="cluster.migrate"):
        cluster.migrate_queueing(Fake(), cluster.HostDirectory(4), None, 0)
    Fake.KIND = _capi.TBE_KIND_APPROXIMATE
    with pytest.raises(ValueError, match="nothing to move"):
        cluster.migrate_queueing(Fake(), cluster.HostDirectory(4), None, 0)
    Fake.KIND = _capi.TBE_KIND_QUEUEING
    with pytest.raises(ValueError, match="text-keyed"):
        cluster.migrate_queueing(Fake(), HostStringDirectory(4), None, 0)


def test_plan_queue_migration_sends_queued_keys_whatever_their_row():
    from distributedratelimiting.redis_amd import cluster
    keys = np.array([10, 11, 12, 13, Q.NO, Q.NO], dtype=np.uint64)
    v = np.arange(6, dtype=np.float64)
    t = np.array([5, ABSENT, 7, ABSENT, ABSENT, 9], dtype=np.int64)
    live = np.array([1, 0, 0, 0, 0, 0], dtype=bool)          # row 2 has lapsed
    qcount = np.array([0, 2, 3, 0, 1, 0])
    omap = np.full(4096, 1, dtype=np.uint8)                    # everything leaves rank 0
    rows, counts, leaving, row_ids = cluster.plan_queue_migration(keys, v, t, np.array([0, 1, 2, 0, 0, 0]), live, qcount,
                                                                  omap, 2, 0)
    assert row_ids.tolist() == [0, 1, 2] and leaving.tolist() == [1, 1, 1, 1, 0, 0]
    assert rows[:, 3].tolist() == [0, 1 | (2 << 8), 2 | (3 << 8)] and rows[:, 2].tolist() == [5, ABSENT, 7]
    assert counts.tolist() == [0, 3, 4, 1]                     # the orphan: an unheld id with a queue
