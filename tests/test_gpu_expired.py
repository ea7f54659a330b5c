"""tbe_expired_device (include/tbe.h): which keys' Redis hash no longer exists at a
timestamp (the EXPIRE of TB:232-235), against the numpy statement of the rule on
export_state and against tbe_query on the boundary."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ABSENT = np.iinfo(np.int64).min
TS = 1_760_000_100_000_123          # the scan's timestamp (us)
TTL_MS = 3_000                      # limit 5 at 2 tokens per second: ceil(2.5) s


def _dead_rule(t_us, ts_us, ttl_ms=TTL_MS):
    return (t_us == ABSENT) | (t_us < 1000 * (ts_us // 1000 - ttl_ms))


def _stream(gpu):
    import torch
    return torch.cuda.stream(torch.cuda.Stream(gpu))


def test_token_bucket_flags_and_clear(engine_lib, gpu):
    import torch
    from distributedratelimiting.redis_amd import TokenBucketEngine
    n = 5_000                        # no multiple of the 2,048-row bucket or of 256
    rng = np.random.default_rng(17)
    ms = TS // 1000
    v = rng.uniform(0.0, 5.0, n)
    t = TS - rng.integers(0, 6_000_000, n)            # around the TTL either way
    t[rng.random(n) < 0.2] = ABSENT
    # crafted rows inside the scanned range
    absent, on_edge, past_edge, future = 10, 11, 12, 13
    t[absent] = ABSENT
    t[on_edge] = (ms - TTL_MS) * 1000 + 7             # ts // 1000 == t // 1000 + 3000: present
    t[past_edge] = (ms - TTL_MS - 1) * 1000 + 999     # one millisecond earlier: dead
    t[future] = TS + 5_000_000                        # t_us > ts_us: present
    crafted = [absent, on_edge, past_edge, future]
    with _stream(gpu):
        cur = torch.cuda.current_stream(gpu).cuda_stream
        eng = TokenBucketEngine(n, 5, 2, 10_000_000, device=0)
        eng.import_state(v, t)
        # a random batch, enqueued and not waited for: the scan is ordered after it
        m = 3_000
        k = rng.integers(0, n, m).astype(np.uint64)
        k[np.isin(k, crafted)] = 100
        p = rng.integers(0, 4, m).astype(np.int32)
        bt = np.sort(TS - 500_000 + rng.integers(0, 400_000, m)).astype(np.int64)
        g = torch.empty(m, dtype=torch.uint8, device=gpu)
        r = torch.empty(m, dtype=torch.int32, device=gpu)
        eng.acquire_batch_device(torch.from_numpy(k.view(np.int64)).to(gpu), torch.from_numpy(p).to(gpu),
                                 torch.from_numpy(bt).to(gpu), g, r, stream=cur)
        first, count = 3, 4_001
        buf = torch.full((count + 64,), 0xAA, dtype=torch.uint8, device=gpu)
        eng.expired_device(TS, buf[:count], first=first, stream=cur)
        got = buf.cpu().numpy()
        v1, t1 = eng.export_state()
        want = _dead_rule(t1[first:first + count], TS)
        print("dead", int(want.sum()), "of", count, "mismatches", int((got[:count] != want).sum()))
        assert np.array_equal(got[:count], want.astype(np.uint8))
        assert (got[count:] == 0xAA).all()            # nothing past the range
        assert 0 < want.sum() < count
        for key in crafted:                           # untouched by the batch
            assert t1[key] == t[key]
            assert bool(got[key - first]) == (eng.query(key, TS) is None), key
        assert [int(got[key - first]) for key in crafted] == [1, 0, 1, 0]
        # clear: the lapsed rows of the range become absent, every other row keeps its bits
        buf2 = torch.full((count,), 0xAA, dtype=torch.uint8, device=gpu)
        eng.expired_device(TS, buf2, first=first, clear=True, stream=cur)
        assert np.array_equal(buf2.cpu().numpy(), got[:count])
        v2, t2 = eng.export_state()
        dead = np.zeros(n, dtype=bool)
        dead[first:first + count] = want
        assert (t2[dead] == ABSENT).all() and (v2[dead] == 5.0).all()
        assert np.array_equal(t2[~dead], t1[~dead])
        assert np.array_equal(v2[~dead].view(np.uint64), v1[~dead].view(np.uint64))
        assert _dead_rule(t1[:first], TS).any() or _dead_rule(t1[first + count:], TS).any()   # lapsed rows outside stay
        # after the clear a scan at an earlier time still finds them dead
        buf3 = torch.empty(count, dtype=torch.uint8, device=gpu)
        eng.expired_device(TS - 10_000_000, buf3, first=first, stream=cur)
        assert (buf3.cpu().numpy()[want] == 1).all()
        eng.close()


@pytest.mark.parametrize("queue_limit", [8, 2_000])
def test_queueing_kind_spares_keys_with_queued_requests(engine_lib, gpu, queue_limit):
    import torch
    from distributedratelimiting.redis_amd import QueueingTokenBucketEngine
    n = 300
    t0 = TS - 100_000_000
    with _stream(gpu):
        cur = torch.cuda.current_stream(gpu).cuda_stream
        eng = QueueingTokenBucketEngine(n, 5, 2, 10_000_000, queue_limit, device=0)
        assert eng.layout()["queue_header_32"] == (queue_limit <= 1024)
        a, b, fresh = 41, 42, 43
        # a and b spend their bucket; a's second request does not fit and waits in its queue
        status, _, _ = eng.wait_batch([a, b, a, fresh], [5, 5, 3, 1], [t0, t0, t0 + 1, TS - 1_000_000], 0)
        assert status.tolist() == [1, 1, 2, 1]
        assert len(eng.queue_of(a)) == 1 and eng.queue_of(b) == []
        d = torch.full((n,), 0xAA, dtype=torch.uint8, device=gpu)
        eng.expired_device(TS, d, stream=cur)
        got = d.cpu().numpy()
        _, t = eng.export_state()
        lapsed = _dead_rule(t, TS)
        assert lapsed[a] and lapsed[b] and not lapsed[fresh]
        want = lapsed.copy()
        want[a] = False                               # lapsed, but a request waits on it
        assert np.array_equal(got, want.astype(np.uint8))
        assert got[b] == 1 and got[a] == 0 and got[fresh] == 0 and got[0] == 1
        eng.close()


def test_approximate_kind_is_rejected(engine_lib, gpu):
    import torch
    from distributedratelimiting.redis_amd import ApproximateEngine, _capi
    with _stream(gpu):
        eng = ApproximateEngine(64, 5, 2, 10_000_000, 4, device=0)
        d = torch.full((64,), 0xAA, dtype=torch.uint8, device=gpu)
        with pytest.raises(_capi.TbeError) as ei:
            eng.expired_device(TS, d, stream=torch.cuda.current_stream(gpu).cuda_stream)
        assert ei.value.status == _capi.TBE_EINVAL
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == 0xAA).all()
        eng.close()


def test_bad_arguments_write_nothing(engine_lib, gpu):
    import torch
    from distributedratelimiting.redis_amd import TokenBucketEngine, _capi
    with _stream(gpu):
        cur = torch.cuda.current_stream(gpu).cuda_stream
        eng = TokenBucketEngine(1_000, 5, 2, 10_000_000, device=0)
        d = torch.full((600,), 0xAA, dtype=torch.uint8, device=gpu)
        for ts, first in [(-1, 0), (TS, 401), (TS, 1_001)]:
            with pytest.raises(_capi.TbeError) as ei:
                eng.expired_device(ts, d, first=first, clear=True, stream=cur)
            assert ei.value.status == _capi.TBE_EINVAL, (ts, first)
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == 0xAA).all()
        eng.expired_device(TS, d, first=400, stream=cur)      # the last range that fits
        assert (d.cpu().numpy() == 1).all()                   # every key absent
        eng.close()
