"""The partition passes (k_hist, k_hist_dig, k_scatter_rec's wave match and full-tile body) and
the final un-partition (k_unscatter, element-wise and 4 elements per access) against the C
restatement, reply for reply and table row for row, on batch sizes at the wave, partition-tile
and un-partition-tile edges and on key patterns that make each match round of each pass decide.

TokenLimit 3 at one token per 10 s with one permit per request: a key's first three requests of
a batch (arrival order) are granted with 2, 1, 0 remaining and the rest denied, so a ranking that
is not stable among equal digits flips replies.  Batches lie 60 s apart (the key's TTL is 30 s):
every batch finds its keys full again."""
import numpy as np
import pytest

from oracle import cref, trace

pytestmark = pytest.mark.gpu

N_KEYS = 3_000_000
ABSENT = np.iinfo(np.int64).min
SIZES = [1, 63, 64, 65, 511, 4095, 4096, 4097, 3 * 4096 + 17, 2 * 8192 + 1]
_rigs = {}


class Rig:
    """One engine and its reference, shared by the cases that use the same settings."""

    def __init__(self, token_limit, hot):
        from distributedratelimiting.redis_amd import TokenBucketEngine, fill_rate
        self.eng = TokenBucketEngine(N_KEYS, token_limit, 1, 10_000_000, device=0, hot=hot)
        self.ref = cref.CTokenBucket(N_KEYS, token_limit, fill_rate(1, 10_000_000))
        self.batch = 0
        lay = self.eng.layout()
        assert lay["passes"] == 2, lay
        self.r_bits = lay["r_bits"]
        self.top = (N_KEYS - 1) >> self.r_bits       # the largest bucket id

    def times(self, n):
        i = np.arange(n, dtype=np.int64)
        t = trace.T0_US + self.batch * 60_000_000 + (i * 10_000) // n
        self.batch += 1
        return t

    def check_batch(self, keys, device=None):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        n = keys.shape[0]
        p = np.ones(n, np.int32)
        t = self.times(n)
        if device is None:
            g, r = self.eng.acquire_batch(keys, p, t)
        else:
            import torch
            # outputs one element into their allocations: granted is not 4-byte and remaining
            # not 16-byte aligned, so the final un-partition takes the element-wise kernel
            d_g = torch.zeros(n + 1, dtype=torch.uint8, device=device)[1:]
            d_r = torch.zeros(n + 1, dtype=torch.int32, device=device)[1:]
            assert d_g.data_ptr() % 4 != 0 and d_r.data_ptr() % 16 != 0
            d_k = torch.from_numpy(keys.view(np.int64)).to(device)
            d_p = torch.from_numpy(p).to(device)
            d_t = torch.from_numpy(t).to(device)
            self.eng.acquire_batch_device(d_k, d_p, d_t, d_g, d_r)
            self.eng.synchronize()
            g, r = d_g.cpu().numpy(), d_r.cpu().numpy()
        g_ref, r_ref = self.ref.acquire_batch(keys, p, t)
        bad = np.flatnonzero((g != g_ref) | (r != r_ref))
        assert bad.size == 0, (n, bad[:5], g[bad[:5]], r[bad[:5]], g_ref[bad[:5]], r_ref[bad[:5]])
        return g, r

    def check_table(self):
        v, t_us = self.eng.export_state()
        v_ref, t_ref = self.ref.export_state()
        assert np.array_equal(t_us, t_ref)
        touched = t_ref != ABSENT
        assert np.array_equal(v[touched].view(np.uint64), v_ref[touched].view(np.uint64))


def rig(token_limit=3, hot=True):
    key = (token_limit, hot)
    if key not in _rigs:
        _rigs[key] = Rig(token_limit, hot)
    return _rigs[key]


def run(rg, make_keys, device=None):
    outs = []
    for n in SIZES:
        outs.append(rg.check_batch(make_keys(n), device))
    rg.check_table()
    return outs


def test_random(engine_lib, gpu):
    rng = np.random.default_rng(7)
    run(rig(), lambda n: rng.integers(0, N_KEYS, n))


@pytest.mark.parametrize("hot", [False, True])
def test_one_key(engine_lib, gpu, hot):
    outs = run(rig(hot=hot), lambda n: np.full(n, 1_234_567))
    for n, (g, r) in zip(SIZES, outs):   # arrival order decides: the first three, and only they
        m = min(n, 3)
        assert g[:m].tolist() == [1] * m and r[:m].tolist() == [2, 1, 0][:m]
        assert not g[m:].any() and not r[m:].any()


@pytest.mark.parametrize("bit", range(16))
def test_two_keys_one_bit_apart(engine_lib, gpu, bit):
    """Two keys alternating whose bucket ids differ in bit `bit` alone: match round bit % 8 of
    pass bit // 8 is the only one that tells them apart."""
    rg = rig()
    a = 5
    b = a ^ ((1 << bit) << rg.r_bits)
    if b >= N_KEYS:
        # no valid key has this bucket bit set (bucket ids end at rg.top): the round never
        # decides in this engine, and both of its ballots are empty in every case above
        assert (1 << bit) > rg.top
        return
    outs = run(rg, lambda n: np.where(np.arange(n) % 2 == 0, a, b))
    for n, (g, r) in zip(SIZES, outs):
        m = min(n, 6)
        assert g[:m].tolist() == [1] * m and r[:m].tolist() == [2, 2, 1, 1, 0, 0][:m]
        assert not g[m:].any()


@pytest.mark.parametrize("mod", [256, 3])
def test_digits_cycling(engine_lib, gpu, mod):
    """key = (i % 256) << r_bits: every lane of a wave on another digit (four to a digit per
    wave); i % 3: three large digit groups per wave."""
    rg = rig()
    run(rg, lambda n: (np.arange(n, dtype=np.uint64) % mod) << np.uint64(rg.r_bits))


def test_buckets_descending(engine_lib, gpu):
    rg = rig()
    run(rg, lambda n: (np.uint64(rg.top) - np.arange(n, dtype=np.uint64) % np.uint64(rg.top + 1)) << np.uint64(rg.r_bits))


def test_four_byte_replies(engine_lib, gpu):
    rg = rig(token_limit=1000)
    assert not rg.eng.layout()["narrow"]
    rng = np.random.default_rng(11)
    run(rg, lambda n: rng.integers(0, N_KEYS, n))


def test_unaligned_outputs(engine_lib, gpu):
    rng = np.random.default_rng(13)
    # few keys: most requests share a key, so the replies depend on arrival order
    run(rig(), lambda n: rng.integers(0, 1000, n) * 2999, device=gpu)
