"""The record formats end to end: every family the last partition pass and the folds are built
for (fold records over narrow pass-0 records, over 8-byte pass-0 records, plain records), with
the permit, position and time fields at their edges, against the C restatement -- every reply
and every exported table row, exactly.

600,000 keys: 586 buckets of 1024 rows, two partition passes.  At TokenLimit 20 the row, permit
code and escape bit take 16 bits (at TokenLimit 10: 15), so the batch sizes below put the fold
record's time field at bit 28 (straddling the 32-bit halves), at bit 32 and at bit 33, and the
position field inside the low half or across it.  One token per 1,000 s: the TTL (TokenLimit /
rate, 10,000 s at TokenLimit 10) outlasts a 40-minute gap, and a 3.5-hour gap outlasts the TTL.

The families: narrow pass-0 records under fold records (TokenLimit 1 .. 128); 8-byte pass-0
records under fold records (no digit stream: with one, a two-pass engine whose records pack
always has room for a narrow record's >= 8 time bits); plain records (fold_records=False).
TokenLimit 100,000 needs 17 permit bits, which leave a 600,000-key record no 32-bit time:
that engine does not pack at all and runs the column passes.

Each engine takes its batches one after another on one clock, with gaps of 1 s (rows granted in
the previous batch), 40 minutes (rows alive but older than the 32-bit time window) and 3.5 hours
(rows past their TTL: expiry on access, also by requests that are then denied).  Inside a batch
most times lie within 10 ms; a few lie 40 ms after and before the first (outside a 16-bit narrow
window, inside the fold window) and a few 40 minutes after it (outside every window)."""
import numpy as np
import pytest

from oracle import cref, trace

pytestmark = pytest.mark.gpu

N_KEYS = 600_000
PERIOD_TICKS = 10_000_000_000            # one token per 1,000 s
ABSENT = np.iinfo(np.int64).min
SIZES = [1, 63, 64, 65, 4095, 4096, 4097, 65_535, 65_536, 65_537, 131_073]
DENSE_FROM = 75_008                      # buckets * rows / 8: uniform keys make the batch dense
GAPS = [1_000_000, 40 * 60_000_000, 210 * 60_000_000]
THREADS = 8
_rigs = {}


def ceil_log2(n):
    return max(1, int(n - 1).bit_length())


class Rig:
    """One engine and its reference on one clock, shared by the cases with the same settings."""

    def __init__(self, token_limit, fold_records=True, digit_stream=True):
        from distributedratelimiting.redis_amd import TokenBucketEngine, fill_rate
        self.tl = token_limit
        self.eng = TokenBucketEngine(N_KEYS, token_limit, 1, PERIOD_TICKS, device=0, fold_records=fold_records,
                                     digit_stream=digit_stream)
        self.ref = cref.CTokenBucket(N_KEYS, token_limit, fill_rate(1, PERIOD_TICKS))
        self.now = trace.T0_US
        self.batch = 0
        self.rng = np.random.default_rng(1000 * token_limit + fold_records)
        lay = self.eng.layout()
        assert lay["passes"] == 2, lay
        self.rb = lay["r_bits"]
        assert ((N_KEYS - 1) >> self.rb) + 1 == 586 and 586 * (1 << self.rb) // 8 == DENSE_FROM
        self.pb = int(token_limit + 1).bit_length()          # permit codes 0 .. TokenLimit + 1
        self.w0 = 32 - self.rb - self.pb - 1
        self.packed = lay["packed"]
        assert self.packed == (token_limit <= 128), lay
        self.fold_records = fold_records and self.packed
        self.narrow0 = self.fold_records and digit_stream and self.w0 >= 8
        assert lay["narrow_pass0"] == self.narrow0, lay
        assert lay["narrow"] == (self.packed and token_limit <= 127), lay    # one-byte replies

    def check_format(self, n, sparse):
        f = self.eng.batch_format(n)
        assert f["passes"] == 2 and f["r_bits"] == self.rb, f
        assert f["sparse"] == sparse, (n, f)
        assert f["fold_records"] == self.fold_records, f
        if self.packed:
            assert f["permit_bits"] == self.pb, f
        if self.fold_records:
            assert f["position_bits"] == ceil_log2(n), (n, f)
            assert f["fold_time_bits"] == 64 - self.rb - self.pb - 1 - ceil_log2(n), (n, f)
            if self.narrow0:
                assert f["pass0_time_bits"] == self.w0, f    # narrow pass-0 records
            else:
                assert f["pass0_time_bits"] >= 32, f         # 8-byte pass-0 records

    def keys(self, n, mode):
        rng = self.rng
        if mode == "four_buckets":
            # 48 rows in each of four buckets: these buckets are dense even in a small batch,
            # and a key meets several requests per chunk
            b = np.array([0, 1, 150, 292], dtype=np.uint64)[rng.integers(0, 4, n)]
            return (b << np.uint64(self.rb)) + rng.integers(0, 48, n).astype(np.uint64) * np.uint64(21)
        k = rng.integers(0, N_KEYS, n).astype(np.uint64)
        busy = rng.random(n) < 0.1                           # a tenth of the requests on 100 keys
        k[busy] = rng.integers(0, 100, int(busy.sum())).astype(np.uint64) * np.uint64(5_987)
        return k

    def times(self, n, gap):
        rng = self.rng
        self.now += gap
        t = self.now + np.sort(rng.integers(0, 10_000, n)).astype(np.int64)
        t[0] = self.now
        if n >= 63:
            i = rng.choice(np.arange(1, n), 9, replace=False)
            t[i[0:3]] = self.now + 40_000 + np.arange(3)
            t[i[3:6]] = self.now - 40_000 + np.arange(3)
            t[i[6:9]] = self.now + 40 * 60_000_000 + np.arange(3)
        return t

    def run_batch(self, n, mode, gap, permits=None):
        sparse = n < DENSE_FROM
        assert sparse or mode == "uniform"
        self.check_format(n, sparse)
        keys = self.keys(n, mode)
        if permits is None:
            permits = self.rng.integers(0, min(self.tl, 3) + 2, n).astype(np.int32)
            over = self.rng.random(n) < 0.05                 # above TokenLimit: denied whatever the row holds
            permits[over] = self.tl + 1 + self.rng.integers(0, 3, int(over.sum()))
        t = self.times(n, gap)
        g, r = self.eng.acquire_batch(keys, permits, t)
        g_ref, r_ref = self.ref.acquire_batch(keys, permits, t, threads=THREADS)
        bad = np.flatnonzero((g != g_ref) | (r != r_ref))
        assert bad.size == 0, (self.tl, n, mode, gap, bad.size, bad[:5], keys[bad[:5]], t[bad[:5]] - self.now,
                               g[bad[:5]], r[bad[:5]], g_ref[bad[:5]], r_ref[bad[:5]])
        self.batch += 1
        return keys, permits, g

    def check_table(self):
        v, t_us = self.eng.export_state()
        v_ref, t_ref = self.ref.export_state()
        assert np.array_equal(t_us, t_ref), np.flatnonzero(t_us != t_ref)[:10]
        touched = t_ref != ABSENT
        assert np.array_equal(v[touched].view(np.uint64), v_ref[touched].view(np.uint64))


def rig(*key):
    if key not in _rigs:
        _rigs[key] = Rig(*key)
    return _rigs[key]


# (TokenLimit, fold records, digit stream)
FAMILIES = [(1, True, True), (10, True, True), (20, True, True), (127, True, True), (128, True, True),
            (100_000, True, True), (10, False, True), (10, True, False)]


@pytest.mark.parametrize("token_limit,fold_records,digit_stream", FAMILIES)
def test_batch_sizes_dense_buckets(engine_lib, gpu, token_limit, fold_records, digit_stream):
    """Every batch size with its buckets dense (k_fold_wide): four buckets' keys below 75,008
    requests, uniform keys from there on."""
    rg = rig(token_limit, fold_records, digit_stream)
    for i, n in enumerate(SIZES):
        rg.run_batch(n, "uniform" if n >= DENSE_FROM else "four_buckets", GAPS[i % 3])
    rg.check_table()


@pytest.mark.parametrize("token_limit,fold_records,digit_stream", FAMILIES)
def test_batch_sizes_sparse_buckets(engine_lib, gpu, token_limit, fold_records, digit_stream):
    """The same sizes with uniform keys: below 75,008 requests every bucket goes to k_fold_sparse."""
    rg = rig(token_limit, fold_records, digit_stream)
    for i, n in enumerate(SIZES):
        rg.run_batch(n, "uniform", GAPS[(i + 1) % 3])
    rg.check_table()


@pytest.mark.parametrize("n,mode", [(131_073, "uniform"), (4_097, "four_buckets"), (4_097, "uniform")])
def test_rows_a_batch_meets(engine_lib, gpu, n, mode):
    """Absent rows, rows granted a second ago, rows granted 40 minutes ago and still alive, and
    rows past their TTL met by requests for more than TokenLimit: denied, and the row is still
    deleted (expiry on access)."""
    rg = Rig(10)
    one = np.ones(n, np.int32)
    assert not (rg.eng.export_state()[1] != ABSENT).any()
    keys, _, g = rg.run_batch(n, mode, 0, one)                       # absent rows
    assert g.any()
    rg.run_batch(n, mode, GAPS[0])                                   # granted in the previous batch
    rg.run_batch(n, mode, GAPS[1])                                   # 40 minutes old, alive
    rg.check_table()
    live = rg.ref.export_state()[1] != ABSENT
    rg.rng = np.random.default_rng(1000 * 10 + 1)                    # (Rig's seed) the first batch's keys again
    k2, _, g2 = rg.run_batch(n, mode, GAPS[2], np.full(n, 11, np.int32))   # past the TTL, all denied
    assert np.array_equal(k2, keys) and not g2.any()
    rg.check_table()
    t_after = rg.ref.export_state()[1]
    hit = np.zeros(N_KEYS, bool)
    hit[k2] = True
    assert (live & hit).any() and (t_after[live & hit] == ABSENT).all()   # denied, yet deleted
    rg.eng.close()
