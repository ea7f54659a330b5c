"""tbe_sdir_route_keys_device and tbe_sdir_usage (include/tbe_strdir.h): the routing key of
every held id, hashed out of the arena in place, against cluster.text_route_keys of the text
the host mirror holds for the id; UINT64_MAX for the ids no key holds.

One directory of capacity 5000 over about 3000 names whose lengths sit on and around the
8-byte words the kernel reads (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65) and one name of 65536
bytes, the longest a key may be; a third of them reclaimed (the arena is compacted and the
survivors move), then new names assigned into the reused ids.  The same with string hashes
cut to 6 bits, where tags collide in every probe round: with 64 tags per round and four
rounds such a directory holds at most 256 names, so that run uses the first 72."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO = np.uint64(0xFFFFFFFFFFFFFFFF)
CAP, ARENA = 5_000, 1 << 18
LENS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65]
SEEDS = [0, 0xDEADBEEFCAFEF00D]


def _name(i: int) -> bytes:
    """Name number i, of length LENS[i % 11]; names of 7 bytes and more are distinct by their
    first seven bytes, the names of length 0 and 1 repeat and are deduplicated."""
    n = LENS[i % len(LENS)]
    if n <= 1:
        return bytes([(i // len(LENS)) % 256])[:n]
    return ((b"%07d" % i) * (n // 7 + 1))[:n]


def _names(lo: int, hi: int, shortest: int = 0):
    out = [_name(i) for i in range(lo, hi)]
    if lo == 0:
        out[5] = bytes(range(256)) * 256          # 65536 bytes
    return [s for s in dict.fromkeys(out) if len(s) >= shortest]


_KEYS = {}


def _route_key(text: bytes, seed: int) -> int:
    return _KEYS[seed][text]


def _learn(names):
    """cluster.text_route_keys of every name, once per seed."""
    from distributedratelimiting.redis_amd import cluster
    from distributedratelimiting.redis_amd.strdir import pack_strings
    for seed in SEEDS:
        have = _KEYS.setdefault(seed, {})
        new = [s for s in names if s not in have]
        if new:
            buf, offs = pack_strings(new)
            have.update(zip(new, cluster.text_route_keys(buf, offs, seed, int(offs[-1])).tolist()))


def _check(d, h, gpu):
    """route_keys over the whole capacity and over a sub-range, the held count, usage()."""
    import torch
    from distributedratelimiting.redis_amd import _capi
    room = sum((len(s) + 7) & ~7 for s in h.ids)
    assert d.usage() == (h.size(), room, ARENA) and d.size() == h.size()
    for seed in SEEDS:
        want = np.full(CAP, NO, dtype=np.uint64)
        for s, i in h.ids.items():
            want[i] = _route_key(s, seed)
        keys, held = d.route_keys(seed, return_held=True)
        assert np.array_equal(keys.cpu().numpy().view(np.uint64), want), seed
        assert int(held.item()) == h.size()
        first, count = 1_237, 2_500
        keys, held = d.route_keys(seed, first=first, count=count, return_held=True)
        assert np.array_equal(keys.cpu().numpy().view(np.uint64), want[first:first + count]), seed
        assert int(held.item()) == int((want[first:first + count] != NO).sum())
        keys = d.route_keys(seed, first=CAP - 1, count=1)
        assert np.array_equal(keys.cpu().numpy().view(np.uint64), want[CAP - 1:])
    # a range past capacity, or no output: TBE_EINVAL, nothing enqueued
    lib = _capi.load()
    out = torch.full((8,), 5, dtype=torch.int64, device=gpu)
    st = torch.cuda.current_stream(gpu).cuda_stream
    for first, count, ptr in ((CAP - 1, 2, out.data_ptr()), (CAP + 1, 0, out.data_ptr()), (0, 1 << 63, out.data_ptr()),
                              (0, 4, None)):
        assert lib.tbe_sdir_route_keys_device(d._h, 0, first, count, ptr, None, st) == _capi.TBE_EINVAL
    assert lib.tbe_sdir_usage(d._h, None) == _capi.TBE_EINVAL
    assert lib.tbe_sdir_route_keys_device(d._h, 0, CAP, 0, out.data_ptr(), None, st) == _capi.TBE_OK   # empty range
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == 5)


@pytest.mark.parametrize("hash_bits,n_names", [(None, 3_000), (6, 72)], ids=["hash62", "hash6"])
def test_route_keys_of_held_ids(engine_lib, gpu, hash_bits, n_names):
    import torch
    from distributedratelimiting.redis_amd.strdir import HostStringDirectory, StringDirectory, to_device
    names = _names(0, n_names)
    later = _names(10_000, 10_000 + n_names // 3, shortest=7)
    assert {len(s) for s in names} == set(LENS) | {65_536} and not set(names) & set(later)
    _learn(names + later)
    with torch.cuda.stream(torch.cuda.Stream(gpu)):
        d = StringDirectory(CAP, ARENA, prefix="limiter:", device=0, hash_bits=hash_bits)
        h = HostStringDirectory(CAP)
        ids = d.assign(*to_device(names, gpu))
        assert np.array_equal(ids.cpu().numpy().view(np.uint64), h.assign(names))
        _check(d, h, gpu)
        # a third of the held ids leave: the arena is compacted, every survivor's text moves
        dead = sorted(h.ids.values())[1::3]
        flags = np.zeros(CAP, dtype=np.uint8)
        flags[dead] = 1
        n = d.reclaim_device(torch.from_numpy(flags).to(gpu))
        assert h.reclaim(dead) == len(dead) == int(n.item())
        _check(d, h, gpu)
        # new names into the reused ids
        ids = d.assign(*to_device(later, gpu))
        want = h.assign(later)
        assert np.array_equal(ids.cpu().numpy().view(np.uint64), want) and set(want.tolist()) <= set(dead)
        _check(d, h, gpu)
        d.close()
