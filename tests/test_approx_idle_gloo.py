"""cluster.approx_idle_epoch at world size 2 with gloo on CPU: each rank scans its own
engine, the "not idle" flags are summed, and a key stays flagged only where every client of
the replicated tier found it idle -- so every rank reclaims and resets the same ids."""
import socket

import numpy as np
import torch.multiprocessing as mp

from tests import _approx_idle_worker as W

WORLD = 2


def _port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_ranks_agree_on_the_idle_keys(tmp_path):
    from distributedratelimiting.redis_amd import snapshot
    mp.start_processes(W.idle_epoch_worker, args=(WORLD, _port(), str(tmp_path)), nprocs=WORLD, join=True,
                       start_method="spawn")
    got = [np.load(tmp_path / f"idle_{r}.npy") for r in range(WORLD)]
    own = [snapshot.approx_idle_rows(*W.rank_state(r), W.TS, W.RATE) for r in range(WORLD)]
    want = own[0] & own[1]
    for r in range(WORLD):
        assert got[r].dtype == np.uint8 and np.array_equal(got[r], want.astype(np.uint8))
    # the case the agreement exists for: idle for one client, in use by the other
    assert int((own[0] & ~own[1]).sum()) > 0 and int((own[1] & ~own[0]).sum()) > 0
    assert 0 < int(want.sum()) < min(int(own[0].sum()), int(own[1].sum()))


def test_single_process_is_the_scan_alone():
    import torch
    from distributedratelimiting.redis_amd import cluster, snapshot
    d_idle = torch.zeros(W.N_KEYS, dtype=torch.uint8)
    cluster.approx_idle_epoch(W.StandInEngine(0), W.TS, d_idle)
    assert np.array_equal(d_idle.numpy(), snapshot.approx_idle_rows(*W.rank_state(0), W.TS, W.RATE).astype(np.uint8))
