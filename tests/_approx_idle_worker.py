"""Rank body for tests/test_approx_idle_gloo.py (world_size 2, gloo on CPU).

The engine is a stand-in whose scan is the numpy statement of the idle rule
(snapshot.approx_idle_rows) over per-rank local tiers and one shared tier table; the point
is cluster.approx_idle_epoch, the same code that combines the flags of HIP engines over
RCCL on a GPU node.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_KEYS = 300
TS = 1_760_000_100_000_123
RATE = 2.0


def rank_state(rank: int):
    """(local, global, queued, v, t_us): the tier replica is the same on every rank, local
    scores and queues are the rank's own."""
    shared = np.random.default_rng(5)
    t_us = TS - shared.integers(0, 4_000_000, N_KEYS)
    t_us[shared.integers(0, 4, N_KEYS) == 0] = np.iinfo(np.int64).min
    v = np.where(shared.integers(0, 2, N_KEYS) == 0, 0.0, shared.uniform(0.0, 6.0, N_KEYS))
    glob = np.where(shared.integers(0, 5, N_KEYS) == 0, 1, 0).astype(np.int32)
    own = np.random.default_rng(100 + rank)
    local = np.where(own.integers(0, 4, N_KEYS) == 0, 1, 0).astype(np.int32)
    queued = np.where(own.integers(0, 6, N_KEYS) == 0, 1, 0).astype(np.uint32)
    return local, glob, queued, v, t_us


class StandInEngine:
    def __init__(self, rank: int):
        self.state = rank_state(rank)
        self.n_keys = N_KEYS

    def idle_device(self, ts_us: int, d_idle, first: int = 0, stream=None) -> None:
        import torch
        from distributedratelimiting.redis_amd import snapshot
        flags = snapshot.approx_idle_rows(*self.state, ts_us, RATE)[first:first + d_idle.numel()]
        d_idle.copy_(torch.from_numpy(flags.astype(np.uint8)))


def idle_epoch_worker(rank: int, world: int, port: int, out_dir: str):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from distributedratelimiting.redis_amd import cluster

    d_idle = torch.full((N_KEYS,), 0xAA, dtype=torch.uint8)
    out = cluster.approx_idle_epoch(StandInEngine(rank), TS, d_idle)
    assert out is d_idle
    np.save(os.path.join(out_dir, f"idle_{rank}.npy"), d_idle.numpy())
    dist.destroy_process_group()
