"""cluster.migrate for text-keyed buckets over gloo on the CPU (worlds 2 and 8): two steps
routed by text under the hash partition, a live change to map B, two steps under B.  The
ranks' engines are oracle stand-ins behind a HostStringDirectory
(tests/_text_migrate_workers.py); the protocol is the code the HIP engines run.

Expected: every reply equals the serial reference (one table behind one string directory,
per step rank 0's batch, then rank 1's, ...), which knows nothing about owners; afterwards
every name's row sits, through the directory, on exactly the rank map B names for the name's
routing key.
"""
import numpy as np
import pytest
import torch.multiprocessing as mp

from tests import _text_migrate_workers as T
from tests import test_dist_gloo as G


def _spawn(fn, *args, world: int):
    mp.start_processes(fn, args=(world, G._port()) + args, nprocs=world, join=True, start_method="spawn")


def _load(tmp_path, world):
    return [np.load(tmp_path / f"tmig_{r}.npz") for r in range(world)]


def test_map_b_moves_half_of_the_names():
    """The shape of the case: all 1000 names are touched by steps 0-1; under seed 0 516 change
    owner, under seed 5 504, for worlds 2 and 8 alike."""
    for world in (2, 8):
        for seed, moved in ((0, 516), (5, 504)):
            old, new = T.owners(world, seed)
            assert (int((old != new).sum()), int((old == new).sum())) == (moved, 1000 - moved)
    old, new = T.owners(2, 0)
    assert np.bincount(old, minlength=2).tolist() == [505, 495]
    assert int((new == 0).sum() - (old == 0).sum()) == 4
    assert T.tight_rank(2, 0) == (0, 505)
    assert {len(s) for s in T.NAMES} == set(range(2, 23))   # across the 8- and 16-byte word boundaries
    # some rank's padded key text grows under map B (the tight-arena case of the GPU test)
    r, used = T.tight_arena_rank(2, 0)
    assert used == int(T.ROOM[old == r].sum()) > 0


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 8])
def test_text_migrate_matches_serial_reference(oracle_lib, tmp_path, world):
    _spawn(T.text_migrate_worker, str(tmp_path), "ok", "plain", world=world)
    T.check_text_migrate(_load(tmp_path, world), moved=516)


def test_text_migrate_classed_matches_serial_reference(oracle_lib, tmp_path):
    _spawn(T.text_migrate_worker, str(tmp_path), "ok", "classed", world=2)
    T.check_text_migrate(_load(tmp_path, 2), classed=True, moved=516)


def test_text_migrate_under_another_seed(oracle_lib, tmp_path):
    """Seed 5 for routing and migration alike: other owners, 504 names move."""
    _spawn(T.text_migrate_worker, str(tmp_path), "ok", "plain", 5, world=2)
    T.check_text_migrate(_load(tmp_path, 2), seed=5, moved=504)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 8])
def test_preflight_failure_raises_everywhere_and_changes_nothing(tmp_path, world):
    _spawn(T.text_migrate_worker, str(tmp_path), "tight", "plain", world=world)
    T.check_refused(_load(tmp_path, world))
