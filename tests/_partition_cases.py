"""Engines, references and key patterns shared by tests/test_gpu_unpartition_runs.py and
tests/test_gpu_hist_loads.py (the scheme of tests/test_gpu_partition_shapes.py).

TokenLimit L at one token per 10 s with one permit per request: a key's first L requests of a
batch (arrival order) are granted with L-1, ..., 0 remaining and the rest denied, so a reply
taken from another position, or a ranking that is not stable among equal digits, flips replies.
Batches lie 60 s apart: at TokenLimit 3 (TTL 30 s) every batch finds its keys full again; at
larger limits rows live on between batches, which the reference follows.  Pass 0's digit of a
key is the low 8 bits of its bucket id, (key >> r_bits) & 255."""
import numpy as np

from oracle import cref, trace

N_KEYS = 3_000_000
ABSENT = np.iinfo(np.int64).min
# wave, workgroup and partition-tile edges (4096 requests per tile, 512 threads)
SIZES = [1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 2 * 4096 + 1, 3 * 4096 + 17]
# more than 1024 tiles: a histogram block then walks several tiles, and the count of a block's
# last tile comes from the block's total
BIG = 2 * 1024 * 4096 + 4097
_rigs = {}


class Rig:
    """One engine and its reference, shared by the cases that use the same settings."""

    def __init__(self, token_limit=3, **kw):
        from distributedratelimiting.redis_amd import TokenBucketEngine, fill_rate
        self.eng = TokenBucketEngine(N_KEYS, token_limit, 1, 10_000_000, device=0, **kw)
        self.ref = cref.CTokenBucket(N_KEYS, token_limit, fill_rate(1, 10_000_000))
        self.batch = 0
        self.lay = self.eng.layout()
        assert self.lay["passes"] == 2 and self.lay["packed"], self.lay
        self.r_bits = self.lay["r_bits"]
        self.top = (N_KEYS - 1) >> self.r_bits       # the largest bucket id
        assert self.top >= 255

    def digits(self, d):
        """Keys whose pass-0 digits are `d` (bucket d: the key's first row)."""
        return np.asarray(d, dtype=np.uint64) << np.uint64(self.r_bits)

    def times(self, n, escapes):
        i = np.arange(n, dtype=np.int64)
        t = trace.T0_US + self.batch * 60_000_000 + (i * 10_000) // n
        if escapes and n >= 63:
            # +-40 ms inside the batch: these times leave the narrow record's field and travel
            # in the side array, which pass 0 indexes by the request's global position
            j = np.random.default_rng(n + self.batch).choice(np.arange(1, n), 6, replace=False)
            t[j[:3]] += 40_000
            t[j[3:]] -= 40_000
        self.batch += 1
        return t

    def check_batch(self, keys, device=None, escapes=False, key_offset=False):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        n = keys.shape[0]
        p = np.ones(n, np.int32)
        t = self.times(n, escapes)
        if device is None:
            g, r = self.eng.acquire_batch(keys, p, t)
        else:
            import torch
            # outputs one element into their allocations: granted not 4-byte aligned, remaining
            # not 16-byte aligned; keys (key_offset) 8 bytes past a 16-byte boundary
            d_g = torch.zeros(n + 1, dtype=torch.uint8, device=device)[1:]
            d_r = torch.zeros(n + 1, dtype=torch.int32, device=device)[1:]
            assert d_g.data_ptr() % 4 != 0 and d_r.data_ptr() % 16 != 0
            off = 1 if key_offset else 0
            d_k = torch.zeros(n + off, dtype=torch.int64, device=device)[off:]
            d_k.copy_(torch.from_numpy(keys.view(np.int64)))
            assert d_k.data_ptr() % 16 == 8 * off
            d_p = torch.from_numpy(p).to(device)
            d_t = torch.from_numpy(t).to(device)
            self.eng.acquire_batch_device(d_k, d_p, d_t, d_g, d_r)
            self.eng.synchronize()
            g, r = d_g.cpu().numpy(), d_r.cpu().numpy()
        g_ref, r_ref = self.ref.acquire_batch(keys, p, t)
        bad = np.flatnonzero((g != g_ref) | (r != r_ref))
        if bad.size:
            self.retire()
        assert bad.size == 0, (n, bad.size, bad[:5], g[bad[:5]], r[bad[:5]], g_ref[bad[:5]], r_ref[bad[:5]])
        return g, r

    def check_table(self):
        v, t_us = self.eng.export_state()
        v_ref, t_ref = self.ref.export_state()
        touched = t_ref != ABSENT
        same = np.array_equal(t_us, t_ref) and np.array_equal(v[touched].view(np.uint64), v_ref[touched].view(np.uint64))
        if not same:
            self.retire()
        assert np.array_equal(t_us, t_ref)
        assert np.array_equal(v[touched].view(np.uint64), v_ref[touched].view(np.uint64))

    def retire(self):
        """After a mismatch the engine and its reference no longer agree: the next test that asks
        for these settings gets a fresh pair, so one failure does not fail the tests after it."""
        for k in [k for k, v in _rigs.items() if v is self]:
            del _rigs[k]


def rig(token_limit=3, **kw):
    key = (token_limit,) + tuple(sorted(kw.items()))
    if key not in _rigs:
        _rigs[key] = Rig(token_limit, **kw)
    return _rigs[key]


def run(rg, make_keys, sizes=SIZES, **kw):
    outs = [rg.check_batch(make_keys(n), **kw) for n in sizes]
    rg.check_table()
    return outs


# ---------------------------------------------------------------- digit patterns (n -> keys)
def one_digit(rg, d):
    """Every request on one key of digit d: a tile is one run of 4096 replies."""
    return lambda n: np.full(n, int(rg.digits(d)) + 1, dtype=np.uint64)


def one_bucket(rg, d, seed):
    """Every request in bucket d (digit d), on random keys of its 2^r_bits: a tile is one run of
    4096 replies again, but keys repeat a few times each, so the replies inside the run differ
    (granted 2, 1, 0 and denied by arrival order) and a wrong staged index shows."""
    rng = np.random.default_rng(seed)
    lo = int(rg.digits(d))
    return lambda n: np.uint64(lo) + rng.integers(0, 1 << rg.r_bits, n).astype(np.uint64)


def cycling(rg, mod):
    """Digits i % mod: mod = 256 makes every run of a full tile 16 long."""
    return lambda n: rg.digits(np.arange(n) % mod)


def gaps(rg):
    """Only every 7th digit present: the empty digits between share their run start with the
    next present one."""
    return lambda n: rg.digits(7 * (np.arange(n) % 37))


_STAIRS = np.repeat(np.arange(256), np.arange(1, 257))   # digit d, d + 1 times: 32896 entries


def stairs(rg):
    """Digit counts 1, 2, 3, ... over every 32896 requests, spread by a stride coprime to that
    length: a tile's runs have all lengths, start at every byte alignment modulo 16 and cross
    128-byte lines."""
    return lambda n: rg.digits(_STAIRS[(np.arange(n) * 7919) % _STAIRS.size])


def random_keys(seed, hi=N_KEYS):
    rng = np.random.default_rng(seed)
    return lambda n: rng.integers(0, hi, n)


def descending(rg):
    top = np.uint64(rg.top)
    return lambda n: (top - np.arange(n, dtype=np.uint64) % (top + np.uint64(1))) << np.uint64(rg.r_bits)


def two_keys(rg, bit):
    """Two keys alternating whose bucket ids differ in bit `bit` alone."""
    a = 5
    b = a ^ ((1 << bit) << rg.r_bits)
    assert b < N_KEYS
    return lambda n: np.where(np.arange(n) % 2 == 0, a, b)


def few_keys(seed):
    """Few keys: most requests share a key, so the replies depend on arrival order."""
    rng = np.random.default_rng(seed)
    return lambda n: rng.integers(0, 1000, n) * 2999


def hot_and_random(seed, hot_key=1_234_567):
    """Two thirds of the requests on one key (hot from the second batch on: more than 2048 of
    a 3 * 4096 + 17 batch), the rest random."""
    rng = np.random.default_rng(seed)
    return lambda n: np.where(rng.random(n) < 2 / 3, hot_key, rng.integers(0, N_KEYS, n))
