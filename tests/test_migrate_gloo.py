"""cluster.migrate over gloo on the CPU (worlds 2 and 8): two routed steps under the hash
partition, a live change to map B, two routed steps under B.  The ranks' engines are oracle
stand-ins (tests/_migrate_workers.py); the protocol is the code the HIP engines run.

Expected: every reply equals the serial reference of test_dist_gloo.check_tb_route (one table,
per step rank 0's batch, then rank 1's, ...), which knows nothing about owners; afterwards
every touched key's row sits, through the directory, on exactly the rank map B names.
"""
import numpy as np
import pytest
import torch.multiprocessing as mp

from tests import _dist_workers as W
from tests import _migrate_workers as M
from tests import test_dist_gloo as G


def _spawn(fn, *args, world: int):
    mp.start_processes(fn, args=(world, G._port()) + args, nprocs=world, join=True, start_method="spawn")


def moved_and_staying(world: int):
    """(keys that change owner, keys that stay) among the keys steps 0-1 touch."""
    from distributedratelimiting.redis_amd import cluster
    keys = M.touched(world, (0, 1))
    old, new = cluster.key_owner(keys, world), cluster.key_owner(keys, world, M.map_b(world))
    return keys[old != new], keys[old == new]


def check_migrate(res, classed: bool = False, shift: int = 0, device_path: bool = False):
    """Replies of all four steps and the final rows against the serial reference (one
    CTokenBucket per class, class of key k = k % 3 when classed)."""
    from oracle import cref
    from oracle.semantics import fill_rate_per_second
    from distributedratelimiting.redis_amd import cluster
    world = len(res)
    classes = M.CLASSES if classed else M.CLASSES[:1]
    nc = len(classes)
    refs = [cref.CTokenBucket(W.TB["n_keys"], c[0], fill_rate_per_second(c[1], c[2])) for c in classes]
    for s in range(W.TB_STEPS):
        batches = [M.batch(r, s, shift) for r in range(world)]
        k, p, t = (np.concatenate([b[i] for b in batches]) for i in range(3))
        g, rem = np.empty(k.size, np.uint8), np.empty(k.size, np.int32)
        for c, ref in enumerate(refs):
            sel = (k % np.uint64(nc)) == c
            g[sel], rem[sel] = ref.acquire_batch(k[sel], p[sel], t[sel])
        for r in range(world):
            sl = slice(r * W.TB_N, (r + 1) * W.TB_N)
            assert np.array_equal(res[r][f"g{s}"], g[sl]), (s, r)
            assert np.array_equal(res[r][f"r{s}"], rem[sl]), (s, r)
    # the move was real: at least 400 keys change owner and at least 400 stay
    moved, stay = moved_and_staying(world)
    assert moved.size >= 400 and stay.size >= 400
    mb = M.map_b(world)
    state = [ref.export_state() for ref in refs]
    all_keys = M.touched(world, range(W.TB_STEPS))
    seen = []
    for r in range(world):
        keys, ids = res[r]["dir_keys"].astype(np.int64), res[r]["dir_ids"].astype(np.int64)
        assert np.all(cluster.key_owner(keys.astype(np.uint64), world, mb) == r)   # the new owner's keys only
        for c in range(nc):
            sel = keys % nc == c
            assert np.array_equal(res[r]["t"][ids[sel]], state[c][1][keys[sel]])
            assert np.array_equal(res[r]["v"][ids[sel]].view(np.int64), state[c][0][keys[sel]].view(np.int64))
        seen.append(keys)
        if device_path:
            assert int(res[r]["dir_size"]) == int((cluster.key_owner(all_keys, world, mb) == r).sum())
    seen = np.concatenate(seen)
    assert seen.size == np.unique(seen).size == all_keys.size      # every key once, none held twice
    sent, recv = sum(int(x["sent"]) for x in res), sum(int(x["recv"]) for x in res)
    assert sent == recv == (0 if shift else moved.size)
    if not shift:
        assert all(int(x["sent"]) > 0 and int(x["recv"]) > 0 for x in res)
    for ref in refs:
        ref.close()


def check_refused(res):
    """Every rank raised, and nothing changed on any of them."""
    for r, x in enumerate(res):
        assert int(x["raised"]) == 1, r
        for name in ("v", "t", "dir_keys", "dir_ids", "dir_size"):
            a, b = x[f"before_{name}"], x[f"after_{name}"]
            assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a,
                                  b.view(np.int64) if b.dtype == np.float64 else b), (r, name)


def test_map_b_moves_half_of_the_keys():
    """The shape of the case: of the 1000 keys, all touched by steps 0-1, 494 change owner."""
    from distributedratelimiting.redis_amd import cluster
    for world in (2, 8):
        moved, stay = moved_and_staying(world)
        assert (moved.size, stay.size) == (494, 506)
        left = np.bincount(cluster.key_owner(moved, world), minlength=world)
        assert left.tolist() == [249, 245] if world == 2 else (left.min() >= 51 and left.max() <= 77)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 8])
def test_migrate_matches_serial_reference(oracle_lib, tmp_path, world):
    _spawn(M.migrate_worker, str(tmp_path), "ok", "plain", world=world)
    check_migrate([np.load(tmp_path / f"mig_{r}.npz") for r in range(world)])


def test_migrate_classed_matches_serial_reference(oracle_lib, tmp_path):
    _spawn(M.migrate_worker, str(tmp_path), "ok", "classed", world=2)
    check_migrate([np.load(tmp_path / f"mig_{r}.npz") for r in range(2)], classed=True)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 8])
def test_preflight_failure_raises_everywhere_and_changes_nothing(tmp_path, world):
    _spawn(M.migrate_worker, str(tmp_path), "tight", "plain", world=world)
    check_refused([np.load(tmp_path / f"mig_{r}.npz") for r in range(world)])


def test_migrate_refuses_other_kinds():
    from distributedratelimiting.redis_amd import _capi, cluster

    class Fake:
        KIND = _capi.TBE_KIND_QUEUEING
    with pytest.raises(ValueError, match="queueing"):
        cluster.migrate(Fake(), cluster.HostDirectory(4), None, 0)
    Fake.KIND = _capi.TBE_KIND_APPROXIMATE
    with pytest.raises(ValueError, match="nothing to move"):
        cluster.migrate(Fake(), cluster.HostDirectory(4), None, 0)
