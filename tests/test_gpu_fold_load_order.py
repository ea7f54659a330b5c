"""The wide fold's prologue and the final un-partition with their independent memory operations
issued back to back (TBE_FOLD_EARLY_LOADS, TBE_UNPART_STRAIGHT), against the C restatement: every
reply and every exported table row, bit for bit.  The cases hold for either value of either
switch (the fold's early form is built and off by default, CHANGELOG.md).

What the reordering can break, and the case that would show it:
 - the slice DMA goes out before the bucket's bounds are known, so a workgroup that then finds
   its bucket empty, or the batch in error, leaves with a DMA issued: empty buckets in a dense
   launch, and a batch holding a key past n_keys (nothing written, the next batch right);
 - out-of-range record slots read a clamped index: buckets of exactly 1, 511, 512, 513, 1024,
   1025, 1536 and 1537 requests (slot and chunk edges), the last of them ending at the end of
   the record array and lying in the table's partial last bucket;
 - every decoder (the three packed record families, wide records, a classed engine), one-byte
   and four-byte replies;
 - escaped times, fetched in a second phase, in the same bucket as ordinary ones;
 - the prefetch target's bounds loaded in the prologue, also in a launch over listed buckets;
 - the un-partition's straight-line body for full tiles beside the masked one for the partial
   tile: batches of whole tiles, whole tiles plus one request, 4095 requests and one."""
import numpy as np
import pytest

from oracle import cref, trace
from tests import _partition_cases as C

pytestmark = pytest.mark.gpu

N_DENSE = 600_000            # R = 1024: 586 buckets, the last one of 960 rows; two 8-bit passes
ABSENT = np.iinfo(np.int64).min
EDGES = [1, 511, 512, 513, 1024, 1025, 1536, 1537]   # 512 threads x 3 slots = chunks of 1536
CLASSES = [(5, 10, 10_000_000)]                      # class 1 of the classed engine
VARIANTS = {
    "default": {},
    "family2": {"digit_stream": False},
    "family0": {"fold_records": False},
    "wide_records": {"pack": False},
    "classed": {"classes": CLASSES},
}
_pairs = {}


class Pair:
    """An engine over N_DENSE keys and its reference; batches lie 60 s apart."""

    def __init__(self, limit, **kw):
        from distributedratelimiting.redis_amd import TokenBucketEngine, fill_rate
        self.n_keys = N_DENSE
        self.eng = TokenBucketEngine(N_DENSE, limit, 1, 10_000_000, device=0, **kw)
        self.lay = self.eng.layout()
        self.R = 1 << self.lay["r_bits"]
        assert self.R == 1024 and self.lay["passes"] == 2 and N_DENSE % self.R != 0, self.lay
        self.nb = (N_DENSE + self.R - 1) // self.R
        self.cls = None
        limits = [(limit, 1, 10_000_000)]
        if kw.get("classes"):
            limits += list(kw["classes"])
            self.cls = (trace.mix64(np.arange(N_DENSE, dtype=np.uint64)) % np.uint64(len(limits))).astype(np.uint8)
            self.eng.set_class(np.arange(N_DENSE, dtype=np.uint64), self.cls)
        self.refs = [cref.CTokenBucket(N_DENSE, c[0], fill_rate(c[1], c[2])) for c in limits]
        self.batch = 0

    def times(self, n, jitter=0):
        i = np.arange(n, dtype=np.int64)
        t = trace.T0_US + self.batch * 60_000_000 + 50_000 + (i * 10_000) // max(n, 1)
        if jitter:   # one request in 64 moved 40 ms forward or back
            rng = np.random.default_rng(1000 + self.batch)
            j = rng.choice(n, n // 64, replace=False)
            t[j] += np.where(rng.random(j.size) < 0.5, jitter, -jitter)
        self.batch += 1
        return t

    def ref_acquire(self, keys, p, t):
        if self.cls is None:
            return self.refs[0].acquire_batch(keys, p, t)
        g = np.empty(len(keys), np.uint8)
        r = np.empty(len(keys), np.int32)
        kc = self.cls[keys.astype(np.int64)]
        for c, ref in enumerate(self.refs):
            m = kc == c
            if m.any():
                g[m], r[m] = ref.acquire_batch(keys[m], p[m], t[m])
        return g, r

    def ref_state(self):
        v, t = self.refs[0].export_state()
        for c, ref in enumerate(self.refs[1:], 1):
            vc, tc = ref.export_state()
            m = self.cls == c
            v[m], t[m] = vc[m], tc[m]
        return v, t

    def check_batch(self, keys, jitter=0, dense=None):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        n = keys.shape[0]
        if dense is not None:
            assert self.eng.batch_format(n)["sparse"] == (not dense)
        p = np.ones(n, np.int32)
        t = self.times(n, jitter)
        g, r = self.eng.acquire_batch(keys, p, t)
        g_ref, r_ref = self.ref_acquire(keys, p, t)
        bad = np.flatnonzero((g != g_ref) | (r != r_ref))
        if bad.size:
            self.retire()
        assert bad.size == 0, (n, bad.size, bad[:5], keys[bad[:5]], g[bad[:5]], r[bad[:5]], g_ref[bad[:5]], r_ref[bad[:5]])
        return g, r

    def check_table(self):
        v, t_us = self.eng.export_state()
        v_ref, t_ref = self.ref_state()
        present = t_ref != ABSENT
        same = np.array_equal(t_us, t_ref) and np.array_equal(v[present].view(np.uint64), v_ref[present].view(np.uint64))
        if not same:
            self.retire()
        assert np.array_equal(t_us, t_ref), int((t_us != t_ref).sum())
        assert np.array_equal(v[present].view(np.uint64), v_ref[present].view(np.uint64))

    def retire(self):
        for k in [k for k, v in _pairs.items() if v is self]:
            del _pairs[k]


def pair(limit=3, variant="default"):
    if (limit, variant) not in _pairs:
        _pairs[(limit, variant)] = Pair(limit, **VARIANTS[variant])
    return _pairs[(limit, variant)]


def keys_in_buckets(rng, pr, buckets, n):
    """n requests on random rows of the given buckets (the partial last bucket's rows exist)."""
    b = np.asarray(buckets, dtype=np.int64)[rng.integers(0, len(buckets), n)]
    rows = np.minimum(pr.n_keys - b * pr.R, pr.R)
    return (b * pr.R + (rng.random(n) * rows).astype(np.int64)).astype(np.uint64)


# ---------------------------------------------------------------- a DMA issued, then an exit
def test_empty_buckets_in_a_dense_launch(engine_lib, oracle_lib, gpu):
    pr = pair()
    assert pr.lay["packed"] and pr.lay["narrow"] and pr.lay["fold_records"] and pr.lay["digit_stream"]
    rng = np.random.default_rng(41)
    used = [b for b in range(pr.nb) if b % 3 != 2]
    for _ in range(2):   # the second batch finds the first one's rows
        g, _r = pr.check_batch(keys_in_buckets(rng, pr, used, 1 << 19), dense=True)
        assert g.min() == 0 and g.max() == 1   # 1.3 requests per key at TokenLimit 3: grants, and some denials
    pr.check_table()
    v, t_us = pr.eng.export_state()
    idle = (np.arange(N_DENSE) // pr.R) % 3 == 2
    assert (t_us[idle] == ABSENT).all()   # the slices that were read for nothing stayed as they were


def test_error_batch_writes_nothing(engine_lib, oracle_lib, gpu):
    from distributedratelimiting.redis_amd import TbeError
    pr = pair()
    rng = np.random.default_rng(43)
    pr.check_batch(rng.integers(0, N_DENSE, 1 << 19), dense=True)
    pr.check_table()
    bad = rng.integers(0, N_DENSE, 1 << 19).astype(np.uint64)
    bad[len(bad) // 3] = N_DENSE
    with pytest.raises(TbeError) as ei:
        pr.eng.acquire_batch(bad, np.ones(len(bad), np.int32), pr.times(len(bad)))
    assert ei.value.status == 1
    pr.check_table()                      # the state before the batch
    pr.check_batch(rng.integers(0, N_DENSE, 1 << 19), dense=True)
    pr.check_table()


# ---------------------------------------------------------------- slot, chunk and array edges
@pytest.mark.parametrize("limit", [3, 128], ids=["one_byte", "four_byte"])
def test_bucket_sizes_at_slot_and_chunk_edges(engine_lib, oracle_lib, gpu, limit):
    """Buckets of exactly EDGES requests inside a dense launch.  The bucket of 1537 is the
    table's last (960 rows), so its records are the last of the record array: the clamped slots
    of its second chunk read the array's final record, and nothing past it."""
    pr = pair(limit)
    rng = np.random.default_rng(47 + limit)
    last = pr.nb - 1
    edge_b = [5, 100, 101, 102, 300, 301, 584, last]
    fill_b = [b for b in range(pr.nb) if b not in edge_b]
    for _ in range(2):
        parts = [keys_in_buckets(rng, pr, [b], m) for b, m in zip(edge_b, EDGES)]
        parts.append(keys_in_buckets(rng, pr, fill_b, 1 << 17))
        keys = np.concatenate(parts)
        rng.shuffle(keys)
        counts = np.bincount((keys // np.uint64(pr.R)).astype(np.int64), minlength=pr.nb)
        assert counts[edge_b].tolist() == EDGES and (keys // np.uint64(pr.R)).max() == last
        pr.check_batch(keys, dense=True)
    pr.check_table()


# ---------------------------------------------------------------- every decoder, both widths
@pytest.mark.parametrize("limit", [3, 128], ids=["one_byte", "four_byte"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_fold_variant(engine_lib, oracle_lib, gpu, variant, limit):
    pr = pair(limit, variant)
    lay = pr.lay
    want = {"default": (True, True, True), "family2": (True, True, False), "family0": (True, False, None),
            "wide_records": (False, None, None), "classed": (False, None, None)}[variant]
    assert lay["packed"] == want[0]
    if want[1] is not None:
        assert lay["fold_records"] == want[1]
    if want[2] is not None:
        assert lay["digit_stream"] == want[2] and lay["narrow_pass0"] == want[2]
    if variant in ("default", "family2", "family0"):
        assert lay["narrow"] == (limit == 3)
    rng = np.random.default_rng(53 + limit)
    for _ in range(2):   # about 900 requests per bucket: most buckets fill more than one slot
        pr.check_batch(rng.integers(0, N_DENSE, 1 << 19), dense=True)
    pr.check_table()


# ---------------------------------------------------------------- escaped times
@pytest.mark.parametrize("variant", ["default", "family2", "family0"])
def test_escaped_times_beside_ordinary_ones(engine_lib, oracle_lib, gpu, variant):
    """+-40 ms on one request in 64: about 14 of a bucket's 900 requests take the escape path,
    in every slot of the chunk, the others the record's own field."""
    pr = pair(3, variant)
    rng = np.random.default_rng(59)
    for _ in range(2):
        pr.check_batch(rng.integers(0, N_DENSE, 1 << 19), jitter=40_000, dense=True)
    pr.check_table()


# ---------------------------------------------------------------- listed dense buckets
@pytest.mark.parametrize("limit", [3, 128], ids=["one_byte", "four_byte"])
def test_sparse_batch_with_listed_dense_buckets(engine_lib, oracle_lib, gpu, limit):
    rg = C.rig(limit)
    assert rg.eng.batch_format(1 << 16)["sparse"]
    R = 1 << rg.r_bits
    rng = np.random.default_rng(61 + limit)
    dense_b = [0, 77, 700, rg.top]                      # the partial last bucket among them
    sizes = [300, 1537, 3100, 600]

    def make(n):
        parts = []
        for b, m in zip(dense_b, sizes):
            rows = min(R, C.N_KEYS - b * R)
            parts.append(b * R + rng.integers(0, rows, m))
        parts.append(rng.integers(0, C.N_KEYS, n - sum(sizes)))
        keys = np.concatenate(parts).astype(np.uint64)
        rng.shuffle(keys)
        return keys

    C.run(rg, make, sizes=[1 << 16] * 2)


# ---------------------------------------------------------------- un-partition tiles
@pytest.mark.parametrize("limit", [3, 128], ids=["one_byte", "four_byte"])
def test_unpartition_full_and_partial_tiles(engine_lib, oracle_lib, gpu, limit):
    """Whole tiles only (every workgroup takes the straight-line body), whole tiles and one
    request (the last workgroup the masked one), one short tile, one request."""
    rg = C.rig(limit)
    sizes = [4096, 3 * 4096, 3 * 4096 + 1, 4095, 1]
    C.run(rg, C.random_keys(67 + limit), sizes=sizes)
    C.run(rg, C.stairs(rg), sizes=sizes)
    C.run(rg, C.few_keys(71 + limit), sizes=sizes)


@pytest.mark.parametrize("limit", [3, 128], ids=["one_byte", "four_byte"])
def test_partial_tile_stores_nothing_past_n(engine_lib, oracle_lib, gpu, limit):
    """The outputs are followed by a whole tile of guard elements: a partial tile that took the
    full tile's body, or a wrong count of valid elements, would overwrite them."""
    import torch
    rg = C.rig(limit)
    rng = np.random.default_rng(73 + limit)
    for n in [1, 4095, 4097, 3 * 4096 + 1]:
        keys = rng.integers(0, 1000, n).astype(np.uint64) * np.uint64(2999)
        p = np.ones(n, np.int32)
        t = rg.times(n, False)
        d_g = torch.full((n + 4096,), 0xEE, dtype=torch.uint8, device=gpu)
        d_r = torch.full((n + 4096,), -7, dtype=torch.int32, device=gpu)
        torch.cuda.synchronize()
        rg.eng.acquire_batch_device(torch.from_numpy(keys.view(np.int64)).to(gpu), torch.from_numpy(p).to(gpu),
                                    torch.from_numpy(t).to(gpu), d_g, d_r)
        rg.eng.synchronize()
        g, r = d_g.cpu().numpy(), d_r.cpu().numpy()
        g_ref, r_ref = rg.ref.acquire_batch(keys, p, t)
        ok = np.array_equal(g[:n], g_ref) and np.array_equal(r[:n], r_ref)
        if not ok:
            rg.retire()
        assert ok, n
        assert (g[n:] == 0xEE).all() and (r[n:] == -7).all(), (n, np.flatnonzero(g[n:] != 0xEE)[:4], np.flatnonzero(r[n:] != -7)[:4])
