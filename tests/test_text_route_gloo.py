"""Routing batches keyed by resourceID text to their owners (cluster.route_text_batch), host
path over gloo on the CPU: worlds 2 and 8, the hash partition and a balanced owner map,
several steps with names that recur across steps and ranks.  Expected = the serial reference
of tests/test_dist_gloo.py's check_tb_route keyed by text (tests/_text_route_workers.py): one
table behind one HostStringDirectory, per step rank 0's batch, then rank 1's, ...; replies
bit-equal.  The ranks are child processes."""
import numpy as np
import pytest
import torch.multiprocessing as mp

from tests import _text_route_workers as T
from tests.test_dist_gloo import _port


def _spawn(world: int, *args):
    mp.start_processes(T.tx_route_worker, args=(world, _port()) + args, nprocs=world, join=True, start_method="spawn")


def test_every_owner_gets_names():
    """The names resource-<i>, i < 300, seed 0: every owner holds at least 30 of them at
    worlds 2, 3 and 8 (so the routed tests below cannot pass by leaving a rank idle)."""
    from distributedratelimiting.redis_amd import cluster
    from distributedratelimiting.redis_amd.strdir import pack_strings
    buf, offs = pack_strings([b"resource-%d" % i for i in range(T.N_NAMES)])
    keys = cluster.text_route_keys(buf, offs, 0, int(offs[-1]))
    for world in (2, 3, 8):
        assert np.bincount(cluster.key_owner(keys, world), minlength=world).min() >= 30


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("map_kind", ["hash", "balanced"])
def test_route_text_batch_matches_serial_reference(oracle_lib, tmp_path, world, map_kind):
    _spawn(world, str(tmp_path), map_kind)
    T.check_text_route([np.load(tmp_path / f"tx_{r}.npz") for r in range(world)])


def test_error_plan_gives_empty_columns(oracle_lib, tmp_path):
    """route_text_requests + route_replies called directly: the malformed rank's plan carries
    the ValueError and describes an empty batch (n = 0, no order, zero send counts), and
    route_replies on it returns empty columns; the other rank's replies are those of its own
    batch alone."""
    mp.start_processes(T.tx_error_plan_worker, args=(2, _port(), str(tmp_path)), nprocs=2, join=True,
                       start_method="spawn")
    good, bad = (np.load(tmp_path / f"ep_{r}.npz") for r in range(2))
    assert bool(bad["is_value_error"]) and "malformed offsets" in str(bad["error"])
    assert int(bad["n"]) == 0 and int(bad["order_len"]) == 0 and not bad["send"].any()
    assert bad["g"].shape == (0,) and bad["r"].shape == (0,)
    assert int(bad["received"]) > 0                      # it still decided what rank 0 sent it
    assert str(good["error"]) == "" and int(good["n"]) == T.TX_N
    from oracle import cref
    from oracle.semantics import fill_rate_per_second
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory
    ref = cref.CTokenBucket(T.N_NAMES, T.OPTS["token_limit"],
                            fill_rate_per_second(T.OPTS["tokens_per_period"], T.OPTS["period_ticks"]))
    names, p, t, _ = T.tx_batch(0, 0)
    g, r = ref.acquire_batch(HostStringDirectory(T.N_NAMES).assign(names), p, t)
    ref.close()
    assert np.array_equal(good["g"], g) and np.array_equal(good["r"], r)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 8])
def test_malformed_batch_on_one_rank(oracle_lib, tmp_path, world):
    """Rank 1's batch of one step has malformed offsets: rank 1 raises ValueError for it, every
    other rank finishes, and all replies equal the reference without that batch."""
    _spawn(world, str(tmp_path), "hash", 1)
    res = [np.load(tmp_path / f"tx_{r}.npz") for r in range(world)]
    assert int(res[1]["raised"]) == T.BAD_STEP
    T.check_text_route(res, bad_rank=1)
