"""k_hist's key loads and its request-to-lane map against the C restatement: a histogram that
counted a key twice, skipped one or took the wrong request's digit puts replies at wrong
positions.  Written for the 16-byte loads of TBE_HIST_LOAD16 (two consecutive keys per lane in a
full, 16-byte aligned tile; off by default, CHANGELOG), whose map differs between full and
partial tiles and between aligned and unaligned key arrays; the cases hold for either
form.  Full tiles beside the batch's partial tile,
key arrays 8 bytes past a 16-byte boundary (the element-wise loads), the hot instantiation, the
digit bytes a re-ranking engine reads back, key validation by request index, and a batch of more
than 1024 tiles (several tiles per workgroup, the next tile's keys in flight)."""
import numpy as np
import pytest

from tests import _partition_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hot", [True, False])
def test_full_and_partial_tiles(engine_lib, gpu, hot):
    rg = C.rig(hot=hot)
    C.run(rg, C.few_keys(41), device=gpu)
    C.run(rg, C.stairs(rg), device=gpu)


@pytest.mark.parametrize("hot", [True, False])
def test_keys_at_odd_offset(engine_lib, gpu, hot):
    rg = C.rig(hot=hot)
    C.run(rg, C.few_keys(43), device=gpu, key_offset=True)
    C.run(rg, C.cycling(rg, 256), device=gpu, key_offset=True)


def test_hot_runs(engine_lib, gpu):
    rg = C.rig()
    C.run(rg, C.hot_and_random(47), sizes=[3 * 4096 + 17] * 4, device=gpu)


@pytest.mark.parametrize("key_offset", [False, True])
def test_rerank_reads_the_digit_bytes(engine_lib, gpu, key_offset):
    rg = C.rig(rerank=True)
    C.run(rg, C.few_keys(53), device=gpu, key_offset=key_offset)
    C.run(rg, C.stairs(rg), device=gpu, key_offset=key_offset)


@pytest.mark.parametrize("key_offset", [False, True])
def test_many_tiles_per_workgroup(engine_lib, gpu, key_offset):
    C.run(C.rig(), C.random_keys(59), sizes=[C.BIG], device=gpu, key_offset=key_offset)


@pytest.mark.parametrize("where", [0, 1, 4095, 4096, 8191, 8192 + 16])
def test_invalid_key_is_reported(engine_lib, gpu, where):
    """One key >= n_keys at either slot of a lane's pair, in a full tile or the partial one: the
    batch fails with the engine's invalid-key error, wherever the key sits."""
    import torch
    from distributedratelimiting.redis_amd import TbeError, TokenBucketEngine
    n = 2 * 4096 + 17
    keys = np.arange(n, dtype=np.int64) % 1000
    n_keys = 200_000
    keys[where] = n_keys
    with TokenBucketEngine(n_keys, 3, 1, 10_000_000, device=0) as eng:
        d_k = torch.from_numpy(keys).to(gpu)
        d_p = torch.ones(n, dtype=torch.int32, device=gpu)
        d_t = torch.full((n,), 1_700_000_000_000_000, dtype=torch.int64, device=gpu)
        d_g = torch.zeros(n, dtype=torch.uint8, device=gpu)
        d_r = torch.zeros(n, dtype=torch.int32, device=gpu)
        eng.acquire_batch_device(d_k, d_p, d_t, d_g, d_r)
        with pytest.raises(TbeError) as ei:
            eng.synchronize()
        assert ei.value.status == 1
