"""Rank bodies and the serial reference of the text-routing tests (tests/test_text_route_gloo.py,
tests/test_gpu_text_route_dist.py): batches keyed by resourceID text, routed to their owners
by cluster.route_text_batch.

Every rank's batch names some of the 300 strings ``resource-<i>``; names recur across steps
and across ranks.  Expected = one serial table behind ONE string directory: per step, rank
0's batch, then rank 1's, ... (the per-key order route_text_batch promises: source rank, then
arrival).
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests._dist_workers import _hip_setup, _init  # noqa: E402

N_NAMES = 300
OPTS = dict(token_limit=5, tokens_per_period=1, period_ticks=10_000_000)
TX_STEPS, TX_N = 3, 400
BAD_STEP = 1                     # the step at which `bad_rank` sends malformed offsets


def tx_batch(rank: int, step: int):
    """(names, permits, ts_us, name numbers) of one rank's batch."""
    rng = np.random.default_rng(7000 + 100 * rank + step)
    idx = rng.integers(0, N_NAMES, TX_N)
    permits = rng.integers(0, 4, TX_N, dtype=np.int32)
    ts = 1_760_000_000_000_000 + step * 700_000 + np.sort(rng.integers(0, 700_000, TX_N))
    return [b"resource-%d" % i for i in idx.tolist()], permits, ts.astype(np.int64), idx


def tx_owner_map(world: int, kind: str):
    """None (hash partition) or the balanced owner map of the whole stream's routing keys."""
    from distributedratelimiting.redis_amd import cluster
    from distributedratelimiting.redis_amd.strdir import pack_strings
    if kind != "balanced":
        return None
    names = [n for r in range(world) for s in range(TX_STEPS) for n in tx_batch(r, s)[0]]
    buf, offs = pack_strings(names)
    keys = cluster.text_route_keys(buf, offs, 0, int(offs[-1]))
    return cluster.balanced_owner_map(np.bincount(cluster.key_vnode(keys), minlength=cluster.OWNER_MAP_SIZE), world)


def _malform(offs: np.ndarray) -> np.ndarray:
    """Offsets whose string 5 ends in front of its start."""
    offs = offs.copy()
    offs[5] = offs[6] + np.uint64(1)
    return offs


def expected(world: int, bad_rank: int = -1):
    """{(rank, step): (granted, remaining)} of the serial reference; `bad_rank`'s batch of
    BAD_STEP is never decided."""
    from oracle import cref
    from oracle.semantics import fill_rate_per_second
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory
    rate = fill_rate_per_second(OPTS["tokens_per_period"], OPTS["period_ticks"])
    ref = cref.CTokenBucket(N_NAMES, OPTS["token_limit"], rate)
    directory = HostStringDirectory(N_NAMES)
    out = {}
    for s in range(TX_STEPS):
        for r in range(world):
            if r == bad_rank and s == BAD_STEP:
                continue
            names, p, t, _ = tx_batch(r, s)
            out[(r, s)] = ref.acquire_batch(directory.assign(names), p, t)
    ref.close()
    return out


def check_text_route(res, bad_rank: int = -1) -> None:
    world = len(res)
    exp = expected(world, bad_rank)
    for r in range(world):
        for s in range(TX_STEPS):
            if (r, s) not in exp:
                assert int(res[r]["raised"]) == s and f"g{s}" not in res[r]
                continue
            assert np.array_equal(res[r][f"g{s}"], exp[(r, s)][0]), (r, s)
            assert np.array_equal(res[r][f"r{s}"], exp[(r, s)][1]), (r, s)
        if r != bad_rank:
            assert int(res[r]["raised"]) == -1
        assert int(res[r]["held"]) > 0, r          # every rank received rows: nothing passes by routing nothing
    # every name is held by exactly one owner's directory
    assert sum(int(x["held"]) for x in res) == len({n for r, s in exp for n in tx_batch(r, s)[0]})


def _steps(rank, bad_rank, route, out):
    """The steps of one rank: route(names, offsets or None, permits, ts) -> (granted, remaining)."""
    from distributedratelimiting.redis_amd.strdir import pack_strings
    out["raised"] = -1
    for s in range(TX_STEPS):
        names, p, t, _ = tx_batch(rank, s)
        buf, offs = pack_strings(names)
        if rank == bad_rank and s == BAD_STEP:
            offs = _malform(offs)
        try:
            out[f"g{s}"], out[f"r{s}"] = route(buf, offs, p, t)
        except ValueError as e:
            # the designed refusal, raised after the reply exchange -- not some other ValueError
            assert "malformed offsets" in str(e) and "1 strings" in str(e), e
            out["raised"] = s


def tx_route_worker(rank: int, world: int, port: int, out_dir: str, map_kind: str = "hash", bad_rank: int = -1):
    """gloo on the CPU: numpy batches, HostStringDirectory, the oracle deciding."""
    dist = _init(rank, world, port)
    from oracle import cref
    from oracle.semantics import fill_rate_per_second
    from distributedratelimiting.redis_amd import cluster
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory

    omap = tx_owner_map(world, map_kind)
    directory = HostStringDirectory(N_NAMES)
    ref = cref.CTokenBucket(N_NAMES, OPTS["token_limit"], fill_rate_per_second(OPTS["tokens_per_period"],
                                                                                OPTS["period_ticks"]))
    out = {}
    _steps(rank, int(bad_rank), lambda buf, offs, p, t: cluster.route_text_batch(
        lambda lk, lp, lt: ref.acquire_batch(lk, lp, lt), buf, offs, p, t, directory, owner_map=omap,
        n_bytes=int(offs[-1])), out)
    out["held"] = directory.size()
    np.savez(os.path.join(out_dir, f"tx_{rank}.npz"), **out)
    ref.close()
    dist.barrier()
    dist.destroy_process_group()


def tx_error_plan_worker(rank: int, world: int, port: int, out_dir: str):
    """route_text_requests and route_replies called directly, rank 1's batch malformed: its
    plan carries the error and describes an empty batch, so route_replies returns empty
    columns there; rank 0 gets the replies of its own requests alone."""
    dist = _init(rank, world, port)
    from oracle import cref
    from oracle.semantics import fill_rate_per_second
    from distributedratelimiting.redis_amd import cluster
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory, pack_strings

    directory = HostStringDirectory(N_NAMES)
    ref = cref.CTokenBucket(N_NAMES, OPTS["token_limit"], fill_rate_per_second(OPTS["tokens_per_period"],
                                                                                OPTS["period_ticks"]))
    names, p, t, _ = tx_batch(rank, 0)
    buf, offs = pack_strings(names)
    if rank == 1:
        offs = _malform(offs)
    (lk, lp, lt), plan = cluster.route_text_requests(buf, offs, p, t, directory, n_bytes=int(offs[-1]))
    cols = cluster.route_replies(plan, ref.acquire_batch(lk, lp, lt))
    np.savez(os.path.join(out_dir, f"ep_{rank}.npz"), error="" if plan.error is None else str(plan.error),
             is_value_error=isinstance(plan.error, ValueError), n=plan.n, order_len=len(plan.order),
             send=np.array(plan.send_counts), received=lk.shape[0], g=cols[0], r=cols[1])
    ref.close()
    dist.barrier()
    dist.destroy_process_group()


def tx_route_worker_hip(rank: int, world: int, port: int, out_dir: str, path: str, map_kind: str = "hash",
                        bad_rank: int = -1):
    """The HIP engine deciding on cuda:0, over gloo.  path "host": numpy batches and a
    HostStringDirectory; path "device": CUDA tensors end to end -- tbe_route_text_* kernels and
    a StringDirectory.  The device path with the hash partition also routes one batch of
    ``synthetic_key_text`` names and the u64 keys they were made from (arrays x*)."""
    dist = _init(rank, world, port)
    torch, dev, stream = _hip_setup()
    from distributedratelimiting.redis_amd import TokenBucketEngine, cluster
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory, StringDirectory, synthetic_key_text

    omap = tx_owner_map(world, map_kind)
    opts = (OPTS["token_limit"], OPTS["tokens_per_period"], OPTS["period_ticks"])
    eng = TokenBucketEngine(N_NAMES, *opts, device=0)

    def decide_on(engine):
        def decide(lk, lp, lt):
            g = torch.empty(lk.numel(), dtype=torch.uint8, device=dev)
            r = torch.empty(lk.numel(), dtype=torch.int32, device=dev)
            engine.acquire_batch_device(lk, lp, lt, g, r, stream=stream.cuda_stream)
            return g, r
        return decide

    out = {}
    if path == "device":
        directory = StringDirectory(N_NAMES, 1 << 16, device=0)

        def route(buf, offs, p, t):
            g, r = cluster.route_text_batch(decide_on(eng), torch.from_numpy(buf).to(dev),
                                            torch.from_numpy(offs.view(np.int64)).to(dev), torch.from_numpy(p).to(dev),
                                            torch.from_numpy(t).to(dev), directory, owner_map=omap, n_bytes=int(offs[-1]))
            return g.cpu().numpy(), r.cpu().numpy()
    else:
        directory = HostStringDirectory(N_NAMES)

        def route(buf, offs, p, t):
            return cluster.route_text_batch(lambda lk, lp, lt: eng.acquire_batch(lk, lp, lt), buf, offs, p, t,
                                            directory, owner_map=omap, n_bytes=int(offs[-1]))
    _steps(rank, int(bad_rank), route, out)
    eng.synchronize()
    out["held"] = directory.size()
    if path == "device" and map_kind == "hash":
        # the same requests by text and by the u64 keys the text was made from: the owners
        # differ, the per-key order (source rank, arrival) does not
        _, p, t, idx = tx_batch(rank, 0)
        k, p, t = (torch.from_numpy(x).to(dev) for x in (idx.astype(np.int64), p, t))
        buf, offs, nb = synthetic_key_text(k)
        eng_t, eng_u = TokenBucketEngine(N_NAMES, *opts, device=0), TokenBucketEngine(N_NAMES, *opts, device=0)
        dir_t, dir_u = StringDirectory(N_NAMES, 1 << 16, device=0), cluster.DeviceDirectory(N_NAMES, device=0)
        gt, rt = cluster.route_text_batch(decide_on(eng_t), buf, offs, p, t, dir_t, n_bytes=nb)
        gu, ru = cluster.route_batch(decide_on(eng_u), k, p, t, dir_u)
        out.update(xkeys=idx, xt_g=gt.cpu().numpy(), xt_r=rt.cpu().numpy(), xu_g=gu.cpu().numpy(),
                   xu_r=ru.cpu().numpy())
        for e in (eng_t, eng_u):
            e.synchronize()
            e.close()
    np.savez(os.path.join(out_dir, f"tx_{rank}.npz"), **out)
    eng.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    # python tests/_text_route_workers.py <worker> <rank> <world> <port> <out_dir> [args]
    fn = globals()[sys.argv[1]]
    fn(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), *sys.argv[5:])
