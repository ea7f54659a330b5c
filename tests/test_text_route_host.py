"""The routing key of a key's text on the host (include/tbe_cluster.h "routing text"): pinned
values, cluster.text_route_keys against a plain Python loop, tbe_text_route_key of the loaded
library against both, and snapshot.merge(owner=) for text-keyed files.  No GPU."""
import numpy as np
import pytest

from distributedratelimiting.redis_amd import _capi, cluster, snapshot
from distributedratelimiting.redis_amd.strdir import pack_strings

M64 = (1 << 64) - 1


def _mix(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def py_key(text: bytes, seed: int = 0) -> int:
    h = _mix(seed ^ (len(text) * 0x9E3779B97F4A7C15 & M64))
    for k in range(0, len(text), 8):
        h = _mix(h ^ int.from_bytes(text[k:k + 8], "little"))
    return h


def _strings():
    rng = np.random.default_rng(11)
    out = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in (0, 1, 7, 8, 9, 15, 16, 17, 65536)]
    out += [b"ab", b"ab\0", b"", "naïve-ключ-鍵-🔑".encode("utf-8"), "résumé".encode("utf-8"), b"resource-0"]
    return out


def test_pinned_values():
    assert py_key(b"") == 0x0
    assert py_key(b"a") == 0x343E69370AD4A4EE
    assert py_key(b"resource-0") == 0xCDFEEC7B9A8E85D2
    assert py_key(b"resource-0", 1) == 0xF710EA44F7E306AB
    buf, offs = pack_strings([b"", b"a", b"resource-0"])
    assert cluster.text_route_keys(buf, offs, 0, int(offs[-1])).tolist() == [0x0, 0x343E69370AD4A4EE,
                                                                              0xCDFEEC7B9A8E85D2]
    assert cluster.text_route_keys(buf, offs, 1, int(offs[-1]))[2] == 0xF710EA44F7E306AB


@pytest.mark.parametrize("seed", [0, 1, 0xDEADBEEFCAFEF00D])
def test_numpy_mirror_equals_python_loop(seed):
    strings = _strings()
    buf, offs = pack_strings(strings)
    got = cluster.text_route_keys(buf, offs, seed, int(offs[-1]))
    assert got.dtype == np.uint64 and got.tolist() == [py_key(s, seed) for s in strings]
    assert py_key(b"ab", seed) != py_key(b"ab\0", seed)          # the length is part of the key
    # int64 offsets (the device layout) and bytes without padding give the same keys
    blob = b"".join(strings)
    assert np.array_equal(cluster.text_route_keys(blob, offs.view(np.int64), seed), got)
    # a malformed string hashes as the empty one; the others are unaffected
    bad = offs.copy()
    bad[2] = bad[3] + np.uint64(1)              # string 1 passes its successor's start; string 2 ends before it starts
    keys = cluster.text_route_keys(buf, bad, seed, int(offs[-1]))
    assert keys[2] == py_key(b"", seed) and np.array_equal(keys[3:], got[3:])
    assert cluster._text_spans(bad, int(offs[-1]))[2].tolist() == [False, False, True] + [False] * (len(strings) - 3)
    past = offs.copy()
    past[-1] += np.uint64(1)                    # the last string ends past n_bytes
    assert cluster._text_spans(past, int(offs[-1]))[2].tolist() == [False] * (len(strings) - 1) + [True]
    long = np.array([0, 65537], dtype=np.uint64)
    assert cluster._text_spans(long, 1 << 20)[2].tolist() == [True]


def test_library_equals_mirror(engine_lib):
    lib = _capi.load()
    for seed in (0, 1, 0xDEADBEEFCAFEF00D):
        for s in _strings():
            assert lib.tbe_text_route_key(s, len(s), seed) == py_key(s, seed), (len(s), seed)
    assert lib.tbe_text_route_key(None, 0, 7) == py_key(b"", 7)


def test_bad_arguments_are_einval(engine_lib):
    """NULL pointers, misaligned byte buffers, n >= 2^32 and n_owners outside 1..256 are refused
    before anything is enqueued (so this needs no device)."""
    lib = _capi.load()
    bad = _capi.TBE_EINVAL
    p = 0x1000          # never dereferenced: the argument checks return first
    assert lib.tbe_route_text_keys_device(p, 8, p, 4, 0, p, None, None) == bad
    assert lib.tbe_route_text_keys_device(p, 8, None, 4, 0, p, p, None) == bad
    assert lib.tbe_route_text_keys_device(p, 8, p, 4, 0, None, p, None) == bad
    assert lib.tbe_route_text_keys_device(None, 8, p, 4, 0, p, p, None) == bad
    assert lib.tbe_route_text_keys_device(p + 1, 8, p, 4, 0, p, p, None) == bad
    assert lib.tbe_route_text_keys_device(p, 8, p, 1 << 32, 0, p, p, None) == bad
    for n_owners in (0, 257):
        assert lib.tbe_route_text_offsets_device(p, 8, 4, p, p, n_owners, p, p, p, None) == bad
    for args in ((None, 8, 4, p, p, 2, p, p, p), (p, 8, 4, None, p, 2, p, p, p), (p, 8, 4, p, None, 2, p, p, p),
                 (p, 8, 4, p, p, 2, None, p, p), (p, 8, 4, p, p, 2, p, None, p), (p, 8, 4, p, p, 2, p, p, None),
                 (p, 8, 4, p, p, 2, p + 4, p, p), (p, 8, 1 << 32, p, p, 2, p, p, p)):
        assert lib.tbe_route_text_offsets_device(*args, None) == bad
    good = [p, 8, p, 4, p, p, p, p, p, 64, p]
    for i in (0, 2, 4, 5, 6, 7, 8, 10):
        args = list(good)
        args[i] = None
        assert lib.tbe_route_text_pack_device(*args, None) == bad, i
    assert lib.tbe_route_text_pack_device(*(good[:8] + [p + 2] + good[9:]), None) == bad
    assert lib.tbe_route_text_recv_offsets_device(p, 4, p, None, None) == bad
    assert lib.tbe_route_text_recv_offsets_device(None, 4, p, p, None) == bad
    assert lib.tbe_route_text_recv_offsets_device(p, 4, None, p, None) == bad
    assert lib.tbe_route_text_pack_device(None, 0, None, 0, None, None, None, None, None, 0, None,
                                          None) == _capi.TBE_OK                       # n == 0: nothing to do
    assert lib.tbe_route_text_workspace_bytes(0) == 0 and lib.tbe_route_text_workspace_bytes(1025) == 2 * 12 + 4 * 1025


def test_plan_text_route_groups_by_owner():
    """The numpy statement of the sender's steps: a stable grouping, tightly packed text."""
    rng = np.random.default_rng(5)
    names = [b"resource-%d" % i for i in rng.integers(0, 300, 1000).tolist()]
    buf, offs = pack_strings(names)
    for world in (1, 3, 8):
        p = cluster.plan_text_route(buf, offs, world, None, 0, int(offs[-1]))
        owner = cluster.key_owner(p["keys"], world)
        assert p["n_bad"] == 0 and np.array_equal(p["counts"], np.bincount(owner, minlength=world))
        grouped = [names[i] for i in p["order"]]
        assert [owner[i] for i in p["order"]] == sorted(owner.tolist())
        assert p["out_bytes"].tobytes() == b"".join(grouped)
        assert np.array_equal(np.diff(p["send_offs"]), [len(g) for g in grouped])
        assert np.array_equal(p["order"][p["pos"]], np.arange(len(names)))
        assert p["byte_counts"].tolist() == [sum(len(n) for n, o in zip(names, owner) if o == r) for r in range(world)]


def _engine():
    import types
    return types.SimpleNamespace(config=_capi.make_config(1 << 20, 5, 2, 10_000_000, device=0))


def test_merge_owner_for_text_files(tmp_path):
    rng = np.random.default_rng(9)
    names = [b"resource-%d" % i for i in range(300)] + [b"", "ключ".encode("utf-8"), b"x" * 100]
    half = len(names) // 2
    meta = snapshot.option_meta(_engine().config, 1_760_000_100_000_123)
    v, t = rng.uniform(0.0, 5.0, len(names)), rng.integers(1, 1 << 50, len(names))
    paths = []
    for name, sl in (("a.npz", slice(0, half)), ("b.npz", slice(half, None))):
        snapshot.write(tmp_path / name, meta, v[sl], t[sl], text=pack_strings(names[sl]))
        paths.append(tmp_path / name)
    buf, offs = pack_strings(names)
    omap = cluster.balanced_owner_map(rng.integers(0, 50, 4096), 3)
    for world, owner_map, seed in ((2, None, None), (3, None, None), (8, None, None), (3, omap, None), (8, None, 5),
                                   (3, omap, 0xFFFFFFFFFFFFFFFF)):
        keys = cluster.text_route_keys(buf, offs, seed or 0, int(offs[-1]))
        own = cluster.key_owner(keys, world, owner_map)
        seen = []
        for rank in range(world):
            owner = (rank, world, owner_map) if seed is None else (rank, world, owner_map, seed)
            rows = snapshot.merge(paths, _engine().config, "text", owner=owner)
            blob, o = rows["text"]
            got = [blob.tobytes()[int(o[i]):int(o[i + 1])] for i in range(len(o) - 1)]
            keep = own == rank
            assert got == [n for n, k in zip(names, keep) if k]            # file order kept
            assert np.array_equal(rows["v"].view(np.uint64), v[keep].view(np.uint64))
            assert np.array_equal(rows["t_us"], t[keep])
            assert len(got) > 0
            seen += got
        assert sorted(seen) == sorted(names)                               # a partition: the union is the file
    # a seed moves names between owners; three-entry tuples still select u64 keys as before
    k0, k5 = (cluster.key_owner(cluster.text_route_keys(buf, offs, s, int(offs[-1])), 8) for s in (0, 5))
    assert (k0 != k5).any()
    snapshot.write(tmp_path / "k.npz", meta, v[:3], t[:3], keys=np.array([1, 2, 3], dtype=np.uint64))
    for owner in ((0, 2, None), (0, 2, None, 9)):
        rows = snapshot.merge([tmp_path / "k.npz"], _engine().config, "keys", owner=owner)
        assert rows["keys"].tolist() == [k for k in (1, 2, 3) if cluster.key_owner(np.array([k], np.uint64), 2)[0] == 0]
