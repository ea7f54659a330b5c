"""Reclaiming expired keys in the device string directory (include/tbe_strdir.h:
tbe_sdir_reclaim, tbe_sdir_reclaim_device) against the host mirror's id rule and against
what Redis would answer: one bucket per key string, dropped at its EXPIRE (TB:232-235)."""
import numpy as np
import pytest

from oracle import cref

pytestmark = pytest.mark.gpu

NONE = np.uint64(2**64 - 1)
ABSENT = np.iinfo(np.int64).min
T0 = 1_760_000_000_000_000
TTL_MS = 3_000                      # limit 5 at 2 tokens per second: ceil(2.5) s


def _side_stream(gpu):
    import torch
    return torch.cuda.stream(torch.cuda.Stream(gpu))


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _decide(eng, ids, permits, ts, gpu):
    """One engine batch on device ids, on the current stream; (granted, remaining)."""
    import torch
    n = ids.numel()
    g = torch.empty(n, dtype=torch.uint8, device=gpu)
    r = torch.empty(n, dtype=torch.int32, device=gpu)
    eng.acquire_batch_device(ids, torch.from_numpy(np.asarray(permits, dtype=np.int32)).to(gpu),
                             torch.from_numpy(np.asarray(ts, dtype=np.int64)).to(gpu), g, r,
                             stream=torch.cuda.current_stream(gpu).cuda_stream)
    return g.cpu().numpy(), r.cpu().numpy()


@pytest.mark.parametrize("mode", ["full", "warm", "auto"])
@pytest.mark.parametrize("hash_bits", [None, 14])
def test_churn_against_redis_truth(engine_lib, gpu, mode, hash_bits):
    """12 cycles of a sliding key window: far more distinct strings than ids, slots or arena
    bytes pass through, under 6,000 are ever alive.  Ids follow the mirror, replies follow
    one bucket per string with natural expiry, and each reclaim removes exactly the keys
    whose bucket is gone.  With hashes cut to 14 bits half of every window is assigned
    again after its probe-round neighbours were removed."""
    from distributedratelimiting.redis_amd import TokenBucketEngine, fill_rate
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory, StringDirectory, to_device
    cap, arena = 8_192, 128 << 10
    rng = np.random.default_rng(23)
    with _side_stream(gpu):
        d = StringDirectory(cap, arena, prefix="edge:", device=0, hash_bits=hash_bits, mode=mode)
        h = HostStringDirectory(cap)
        eng = TokenBucketEngine(cap, 5, 2, 10_000_000, device=0)
        ref = cref.CTokenBucket(2_000 * 11 + 4_000, 5, fill_rate(2, 10_000_000))
        new_keys = text = peak = 0
        for c in range(12):
            num = rng.integers(2_000 * c, 2_000 * c + 4_000, 3_000)
            s = [b"user-%d" % k for k in num.tolist()]
            fresh = [k for k in set(s) if k not in h.ids]
            new_keys += len(fresh)
            text += sum((len(k) + 7) // 8 * 8 for k in fresh)
            want_ids = h.assign(s)
            peak = max(peak, h.size())
            buf, offs, nb = to_device(s, gpu)
            ids = d.assign(buf, offs, nb)
            assert np.array_equal(_u64(ids), want_ids), c
            ts = np.full(3_000, T0 + 2_000_000 * c, dtype=np.int64)
            p = rng.integers(0, 4, 3_000).astype(np.int32)
            g, r = _decide(eng, ids, p, ts, gpu)
            g_ref, r_ref = ref.acquire_batch(num.astype(np.uint64), p, ts)
            assert np.array_equal(g, g_ref) and np.array_equal(r, r_ref), c
            # Redis truth: a key is gone when its bucket's last grant is a TTL behind
            _, t_ref = ref.export_state()
            gone = (t_ref == ABSENT) | (t_ref < 1000 * (int(ts[0]) // 1000 - TTL_MS))
            dead = [i for k, i in h.ids.items() if gone[int(k[5:])]]
            n_dead = h.reclaim(dead)
            assert d.reclaim(eng, int(ts[0])) == n_dead, c
            assert d.size() == h.size(), c
        print("new keys", new_keys, "text bytes", text, "peak live", peak, "live at end", h.size())
        assert peak < 6_000
        assert new_keys > 2 * cap and text > 2 * arena        # far past every limit without a reclaim
        s = [b"user-%d" % k for k in range(18_000, 26_000, 3)]
        buf, offs, nb = to_device(s, gpu)
        assert np.array_equal(_u64(d.lookup(buf, offs, nb)), h.lookup(s))
        eng.close()


def test_reclaim_survives_clock_step_back(engine_lib, gpu):
    """A's bucket is spent; A lapses and is reclaimed; B takes A's id and is decided at a
    timestamp before A's lapse.  Redis has no bucket named B: it starts full."""
    from distributedratelimiting.redis_amd import TokenBucketEngine
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory, StringDirectory, to_device
    with _side_stream(gpu):
        d = StringDirectory(16, 1 << 12, device=0)
        h = HostStringDirectory(16)
        eng = TokenBucketEngine(16, 5, 2, 10_000_000, device=0)
        buf, offs, nb = to_device([b"A"], gpu)
        ida = d.assign(buf, offs, nb)
        assert np.array_equal(_u64(ida), h.assign([b"A"]))
        g, r = _decide(eng, ida, [5], [T0], gpu)
        assert g.tolist() == [1] and r.tolist() == [0]
        assert d.reclaim(eng, T0 + 10_000_000) == h.reclaim(h.lookup([b"A"]).tolist()) == 1
        buf, offs, nb = to_device([b"B"], gpu)
        idb = d.assign(buf, offs, nb)
        assert np.array_equal(_u64(idb), h.assign([b"B"])) and _u64(idb)[0] == _u64(ida)[0]
        g, r = _decide(eng, idb, [5], [T0 + 1_000_000], gpu)     # 1 s after A's grant: A would hold 2 tokens
        assert g.tolist() == [1] and r.tolist() == [0]
        eng.close()


def test_keep_list(engine_lib, gpu):
    """Ids of an assign whose engine batch is not submitted yet have no row: they are dead
    unless the caller names them, and go with the next reclaim that does not."""
    from distributedratelimiting.redis_amd import _capi
    from distributedratelimiting.redis_amd import TokenBucketEngine
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory, StringDirectory, to_device
    s = [b"a", b"b", b"pending-c", b"pending-d"]
    with _side_stream(gpu):
        d = StringDirectory(64, 1 << 12, prefix="k:", device=0)
        h = HostStringDirectory(64)
        eng = TokenBucketEngine(64, 5, 2, 10_000_000, device=0)
        buf, offs, nb = to_device(s, gpu)
        ids = d.assign(buf, offs, nb)
        hid = h.assign(s)
        assert np.array_equal(_u64(ids), hid)
        _decide(eng, ids[:2], [1, 1], [T0, T0], gpu)
        # a and b are alive, c and d have no row but are kept
        assert d.reclaim(eng, T0 + 1_000_000, keep_ids=hid[2:]) == h.reclaim(hid[2:], keep_ids=hid[2:]) == 0
        assert np.array_equal(_u64(d.lookup(buf, offs, nb)), hid) and d.size() == 4
        assert d.key_of(int(hid[2])) == b"pending-c" and d.key_of(int(hid[3])) == b"pending-d"
        # everything is dead by now; c alone is kept
        assert d.reclaim(eng, T0 + 10_000_000, keep_ids=hid[2:3]) == h.reclaim(hid, keep_ids=hid[2:3]) == 3
        assert np.array_equal(_u64(d.lookup(buf, offs, nb)), h.lookup(s))
        assert _u64(d.lookup(buf, offs, nb)).tolist() == [int(NONE), int(NONE), int(hid[2]), int(NONE)]
        assert d.key_of(int(hid[2])) == b"pending-c" and d.size() == 1
        with pytest.raises(_capi.TbeError):
            d.key_of(int(hid[3]))
        assert d.reclaim(eng, T0 + 10_000_000) == h.reclaim(hid) == 1
        assert d.size() == h.size() == 0
        # the freed ids come back in the mirror's order
        buf, offs, nb = to_device(s[::-1] + [b"e"], gpu)
        assert np.array_equal(_u64(d.assign(buf, offs, nb)), h.assign(s[::-1] + [b"e"]))
        eng.close()


def test_removed_keys_and_reuse(engine_lib, gpu):
    """reclaim_device on crafted flags: the removed strings are unknown and their ids have
    no text until they are assigned again; the empty string and 65,536-byte strings are
    among the victims and among the survivors."""
    import torch
    from distributedratelimiting.redis_amd import _capi
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory, StringDirectory, to_device
    rng = np.random.default_rng(4)
    big1 = bytes(rng.integers(0, 256, 65_536, dtype=np.uint8))
    big2 = bytes(rng.integers(0, 256, 65_536, dtype=np.uint8))
    big3 = big1[:-1] + bytes([big1[-1] ^ 1])                  # differs from big1 in the last byte only
    cap = 100

    def reclaim(d, h, victims, keep=None):
        flags = np.zeros(cap, dtype=np.uint8)
        flags[[int(i) for i in h.lookup(victims)]] = 1
        flags[sorted(set(range(cap)) - set(h.ids.values()))[:3]] = 1   # ids that hold no key: ignored
        keep_t = None if keep is None else torch.from_numpy(h.lookup(keep).view(np.int64)).to(gpu)
        count = d.reclaim_device(torch.from_numpy(flags).to(gpu), keep_t)
        want = h.reclaim(np.flatnonzero(flags).tolist(), keep_ids=[] if keep is None else h.lookup(keep).tolist())
        assert int(count.item()) == want
        return want

    def check(d, h, known, removed_ids):
        s = list(known) + [b"never-assigned"]
        buf, offs, nb = to_device(s, gpu)
        assert np.array_equal(_u64(d.lookup(buf, offs, nb)), h.lookup(s))
        for k in known:
            i = int(h.lookup([k])[0])
            if i != int(NONE):
                assert d.key_of(i) == k
        live = set(h.ids.values())
        for i in removed_ids:
            if i not in live:
                with pytest.raises(_capi.TbeError) as ei:
                    d.key_of(i)
                assert ei.value.status == _capi.TBE_EINVAL
        assert d.size() == h.size()

    with _side_stream(gpu):
        d = StringDirectory(cap, 1 << 20, prefix="p", device=0)
        h = HostStringDirectory(cap)
        first = [b"", big1, big2, b"a", b"bb", big3, b"12345678", b"123456789"]
        buf, offs, nb = to_device(first, gpu)
        assert np.array_equal(_u64(d.assign(buf, offs, nb)), h.assign(first))
        # victims: the empty string, one 65,536-byte string, a short one; kept: one flagged key
        old = [int(i) for i in h.lookup([b"", big1, b"a"])]
        assert reclaim(d, h, [b"", big1, b"a", b"bb"], keep=[b"bb"]) == 3
        check(d, h, first, old)
        # the ids come back, top of the stack first, with the new text
        second = [b"fresh-1", b"bb", b"", b"fresh-2" * 9, b"fresh-3"]
        buf, offs, nb = to_device(second, gpu)
        got = _u64(d.assign(buf, offs, nb))
        assert np.array_equal(got, h.assign(second))
        assert sorted(got[[0, 2, 3]].tolist()) == sorted(old)
        check(d, h, first + second, old)
        # now the empty string and big3 survive while big2 and a reused id go
        old2 = [int(i) for i in h.lookup([big2, b"fresh-1", b"12345678"])]
        assert reclaim(d, h, [big2, b"fresh-1", b"12345678"]) == 3
        check(d, h, first + second, old + old2)
        third = [big1, b"a", big2, b"zz"]
        buf, offs, nb = to_device(third, gpu)
        assert np.array_equal(_u64(d.assign(buf, offs, nb)), h.assign(third))
        check(d, h, first + second + third, [])


@pytest.mark.parametrize("mode", ["full", "warm"])
def test_stack_then_counter_across_tiles_and_overflow(engine_lib, gpu, mode):
    """The string twin of the u64 directory's test of the same name: one batch takes 700 ids
    from the stack and 1,300 from the counter, its new strings spread over three
    1,024-request blocks; a batch past the room overflows, and a reclaim afterwards works
    but leaves the error in place.  The arena (64 bytes per id) is never the limit."""
    import torch
    from distributedratelimiting.redis_amd import _capi
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory, StringDirectory, to_device
    cap = 4_096
    rng = np.random.default_rng(5)

    def text(nums):
        return [b"user-%d" % k for k in np.asarray(nums).tolist()]

    def assign(d, h, s):
        want = h.assign(s)
        got = _u64(d.assign(*to_device(s, gpu)))
        assert np.array_equal(got, want)
        return want

    def flags(ids):
        f = np.zeros(cap, dtype=np.uint8)
        f[np.asarray(ids, dtype=np.int64)] = 1
        return torch.from_numpy(f).to(gpu)

    def erange(d):
        with pytest.raises(_capi.TbeError) as ei:
            d.size()
        return ei.value.status == _capi.TBE_ERANGE

    with _side_stream(gpu):
        d = StringDirectory(cap, 64 * cap, prefix="t:", device=0, mode=mode)
        h = HostStringDirectory(cap)
        ids = assign(d, h, text(np.arange(1_500)))
        vid = rng.permutation(ids.astype(np.int64))[:700]
        assert int(d.reclaim_device(flags(vid)).item()) == h.reclaim(vid.tolist()) == 700
        assert len(h.free) == 700 and h.fresh == 1_500
        # 2,000 new strings, 600 of them twice, and 400 requests of surviving strings, shuffled
        new = np.arange(10_000, 12_000)
        surv = np.array([k for k in range(1_500) if b"user-%d" % k in h.ids])
        batch = rng.permutation(np.concatenate([new, new[:600], surv[:400]]))
        assert batch.shape[0] == 3_000
        firsts = np.sort(np.unique(batch, return_index=True)[1][np.isin(np.unique(batch), new)])
        assert firsts[0] < 1_024 and (firsts >= 2_048).any() and ((firsts >= 1_024) & (firsts < 2_048)).any()
        assign(d, h, text(batch))
        assert h.free == [] and h.fresh == 1_500 + 1_300 and d.size() == h.size() == 2_800
        # room is 4,096 - 2,800 = 1,296: one string more overflows
        over = text(np.arange(20_000, 21_297))
        want = assign(d, h, over)
        assert h.overflow and (want[:1_296] != NONE).all() and want[1_296] == NONE
        assert erange(d)
        # a reclaim stays in bounds, frees ids, drops the string that has no id; the error stays
        vid = h.lookup(over[:50]).astype(np.int64)
        assert int(d.reclaim_device(flags(vid)).item()) == h.reclaim(vid.tolist()) == 50
        assert erange(d)
        probe = over + text(batch[:200])
        assert np.array_equal(_u64(d.lookup(*to_device(probe, gpu))), h.lookup(probe))
        assign(d, h, over[-3:][::-1])                      # the string without an id among them
        assert erange(d)
        d.close()


def test_noop_reclaims(engine_lib, gpu):
    import torch
    from distributedratelimiting.redis_amd import TokenBucketEngine
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory, StringDirectory, to_device
    rng = np.random.default_rng(9)
    with _side_stream(gpu):
        eng = TokenBucketEngine(3_000, 5, 2, 10_000_000, device=0)
        unused = StringDirectory(3_000, 1 << 16, device=0)
        assert unused.reclaim(eng, T0) == 0 and unused.size() == 0
        d = StringDirectory(3_000, 1 << 16, device=0, hash_bits=12)
        h = HostStringDirectory(3_000)
        s = [b"item-%d" % k for k in rng.integers(0, 1_500, 2_500)]
        buf, offs, nb = to_device(s, gpu)
        ids = _u64(d.assign(buf, offs, nb))
        assert np.array_equal(ids, h.assign(s))
        count = d.reclaim_device(torch.zeros(3_000, dtype=torch.uint8, device=gpu))
        assert int(count.item()) == 0 and d.size() == h.size()
        assert np.array_equal(_u64(d.lookup(buf, offs, nb)), ids)
        for mode in ("full", "warm"):
            d.set_mode(mode)
            assert np.array_equal(_u64(d.assign(buf, offs, nb)), ids), mode
        assert d.size() == h.size()
        more = s[:100] + [b"item-%d" % k for k in range(1_500, 1_600)]
        buf, offs, nb = to_device(more, gpu)
        assert np.array_equal(_u64(d.assign(buf, offs, nb)), h.assign(more))
        eng.close()


@pytest.mark.parametrize("hash_bits", [None, 12])
def test_survivors_stay_reachable_and_single(engine_lib, gpu, hash_bits):
    """A third of the keys is removed.  Every survivor is still found by a lookup (also
    those that sat in a later probe round because of a removed key), and assigning the
    survivors again, on the full path and on the warm one, gives no one a second id; with
    hashes cut to 12 bits about a quarter of the keys share a round-0 tag."""
    import torch
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory, StringDirectory, to_device
    cap = 2_000
    s = [b"sess/%05d" % k for k in range(1_200)]
    with _side_stream(gpu):
        d = StringDirectory(cap, 1 << 15, prefix="t:", device=0, hash_bits=hash_bits, mode="full")
        h = HostStringDirectory(cap)
        buf, offs, nb = to_device(s, gpu)
        ids = _u64(d.assign(buf, offs, nb))
        assert np.array_equal(ids, h.assign(s))
        for turn in range(3):                                  # a different third each time
            flags = np.zeros(cap, dtype=np.uint8)
            flags[h.lookup(s[turn::3]).astype(np.int64)] = 1
            count = d.reclaim_device(torch.from_numpy(flags).to(gpu))
            assert int(count.item()) == h.reclaim(np.flatnonzero(flags).tolist()) == 400
            assert np.array_equal(_u64(d.lookup(buf, offs, nb)), h.lookup(s)), turn
            rest = [k for k in s if k in h.ids]
            rbuf, roffs, rnb = to_device(rest, gpu)
            for mode in ("full", "warm"):
                d.set_mode(mode)
                assert np.array_equal(_u64(d.assign(rbuf, roffs, rnb)), h.lookup(rest)), (turn, mode)
            assert d.size() == h.size() == 800
            assert np.array_equal(_u64(d.assign(buf, offs, nb)), h.assign(s)), turn   # the third comes back
            assert d.size() == 1_200
