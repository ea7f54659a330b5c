"""The text-routing kernels (include/tbe_cluster.h "routing text": tbe_route_text_keys_device,
tbe_route_plan_map_device over the keys, tbe_route_text_offsets_device,
tbe_route_text_pack_device, tbe_route_text_recv_offsets_device) against their numpy statement
(cluster.plan_text_route) in one process: every output word for word, guard bytes behind the
packed text and the rows untouched, malformed offsets counted and never followed."""
import numpy as np
import pytest

from distributedratelimiting.redis_amd import _capi, cluster
from distributedratelimiting.redis_amd.strdir import pack_strings

TILE = 4096                      # requests per routing tile (kRtTile)
GUARD = 64
T0 = 1_760_000_000_000_000


def _run(gpu, buf, offs, nb, n_owners, omap=None, seed=0):
    """The sender's four steps and the receiver's offsets of the send rows on the device;
    every output as a numpy array, with the guards."""
    import torch
    lib = _capi.load()
    n = len(offs) - 1
    ref = cluster.plan_text_route(buf, offs, n_owners, omap, seed, nb)
    total = int(ref["send_offs"][-1])
    rng = np.random.default_rng(n + 7 * n_owners)
    permits = rng.integers(0, 4, n, dtype=np.int32)
    ts = T0 + np.sort(rng.integers(0, 1_000_000, n)).astype(np.int64)
    with torch.cuda.stream(torch.cuda.Stream(gpu)):
        st = cluster.device_stream(gpu)
        d_buf = torch.from_numpy(np.ascontiguousarray(buf[:nb])).to(gpu) if nb else torch.zeros(8, dtype=torch.uint8,
                                                                                                 device=gpu)
        d_offs = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).to(gpu)
        d_p, d_t = torch.from_numpy(permits).to(gpu), torch.from_numpy(ts).to(gpu)
        keys = torch.full((n + 8,), -7, dtype=torch.int64, device=gpu)
        n_bad = torch.full((1,), 99, dtype=torch.int64, device=gpu)
        pos = torch.full((n + 8,), -7, dtype=torch.int32, device=gpu)
        counts = torch.full((n_owners,), 99, dtype=torch.int64, device=gpu)
        byte_counts = torch.full((n_owners,), 99, dtype=torch.int64, device=gpu)
        send_offs = torch.full((n + 1 + 8,), -7, dtype=torch.int64, device=gpu)
        cap = (total + 7) // 8 * 8 + GUARD
        out_bytes = torch.full((cap,), 0xA5, dtype=torch.uint8, device=gpu)
        rows = torch.full((n + 4, 3), -7, dtype=torch.int64, device=gpu)
        roffs = torch.full((n + 1 + 8,), -7, dtype=torch.int64, device=gpu)
        work = torch.empty(max(8, lib.tbe_route_workspace_bytes(n, n_owners), lib.tbe_route_text_workspace_bytes(n)),
                           dtype=torch.uint8, device=gpu)
        dmap = cluster._device_map(omap, gpu, n_owners)
        ok = _capi.TBE_OK
        assert lib.tbe_route_text_keys_device(d_buf.data_ptr(), nb, d_offs.data_ptr(), n, seed, keys.data_ptr(),
                                              n_bad.data_ptr(), st) == ok
        assert lib.tbe_route_plan_map_device(keys.data_ptr(), n, n_owners, dmap.data_ptr() if dmap is not None else None,
                                             work.data_ptr(), pos.data_ptr(), counts.data_ptr(), st) == ok
        assert lib.tbe_route_text_offsets_device(d_offs.data_ptr(), nb, n, pos.data_ptr(), counts.data_ptr(), n_owners,
                                                 work.data_ptr(), send_offs.data_ptr(), byte_counts.data_ptr(), st) == ok
        assert lib.tbe_route_text_pack_device(d_buf.data_ptr(), nb, d_offs.data_ptr(), n, pos.data_ptr(),
                                              send_offs.data_ptr(), d_p.data_ptr(), d_t.data_ptr(), out_bytes.data_ptr(),
                                              cap, rows.data_ptr(), st) == ok
        assert lib.tbe_route_text_recv_offsets_device(rows.data_ptr(), n, work.data_ptr(), roffs.data_ptr(), st) == ok
        torch.cuda.current_stream(gpu).synchronize()
    got = {k: v.cpu().numpy() for k, v in dict(keys=keys, n_bad=n_bad, pos=pos, counts=counts, byte_counts=byte_counts,
                                               send_offs=send_offs, out_bytes=out_bytes, rows=rows, roffs=roffs).items()}
    order = ref["order"]
    ref["rows"] = np.stack([ref["lens"][order], ts[order], permits[order].astype(np.int64)], axis=1).reshape(-1, 3)
    return got, ref, n, total


def _check(got, ref, n, total):
    assert int(got["n_bad"][0]) == ref["n_bad"]
    assert np.array_equal(got["keys"][:n].view(np.uint64), ref["keys"])
    assert np.array_equal(got["pos"][:n], ref["pos"])
    assert np.array_equal(got["counts"], ref["counts"])
    assert np.array_equal(got["byte_counts"], ref["byte_counts"])
    assert np.array_equal(got["send_offs"][:n + 1], ref["send_offs"])
    assert np.array_equal(got["out_bytes"][:total], ref["out_bytes"])          # every byte
    assert np.array_equal(got["rows"][:n], ref["rows"])
    assert np.array_equal(got["roffs"][:n + 1], ref["send_offs"])              # the receiver's scan of the row lengths
    # guards: nothing behind the text, the rows or the other arrays was touched
    assert (got["out_bytes"][total:] == 0xA5).all()
    assert (got["rows"][n:] == -7).all()
    assert (got["keys"][n:] == -7).all() and (got["pos"][n:] == -7).all()
    assert (got["send_offs"][n + 1:] == -7).all() and (got["roffs"][n + 1:] == -7).all()


def _names(n: int, seed: int):
    """n strings of 0..40 bytes drawn from a pool (so that strings recur)."""
    rng = np.random.default_rng(seed)
    pool = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in rng.integers(0, 41, 300)]
    return [pool[i] for i in rng.integers(0, len(pool), n)]


def _maps(n_owners: int):
    rng = np.random.default_rng(n_owners)
    return [None, rng.integers(0, n_owners, cluster.OWNER_MAP_SIZE).astype(np.uint8)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_kernels_equal_numpy(gpu, engine_lib, n):
    strings = _names(n, n)
    buf, offs = pack_strings(strings)
    nb = int(offs[-1])
    for n_owners in (1, 2, 3, 8, 256):
        for omap in _maps(n_owners):
            got, ref, _, total = _run(gpu, buf, offs, nb, n_owners, omap, seed=n_owners)
            _check(got, ref, n, total)
            assert ref["n_bad"] == 0 and total == nb
            if n_owners == 1:      # a loopback: the receiver's offsets reproduce the text in input order
                o = got["roffs"]
                blob = got["out_bytes"].tobytes()
                assert [blob[o[j]:o[j + 1]] for j in range(n)] == strings
    # a map that sends everything to one owner
    omap = np.full(cluster.OWNER_MAP_SIZE, 5, dtype=np.uint8)
    got, ref, _, total = _run(gpu, buf, offs, nb, 8, omap)
    _check(got, ref, n, total)
    assert got["counts"].tolist() == [0] * 5 + [n, 0, 0] and got["byte_counts"][5] == nb
    assert np.array_equal(got["pos"][:n], np.arange(n))


@pytest.mark.gpu
def test_edges_of_neighbouring_strings(gpu, engine_lib):
    """Adjacent strings of every length 0..17 in every order of neighbours, one of 65536 bytes,
    only empty strings, text that ends at an odd n_bytes, duplicates."""
    rng = np.random.default_rng(3)
    short = [rng.integers(1, 256, ln, dtype=np.uint8).tobytes() for ln in range(18)]
    strings = [short[x] for a in range(18) for b in range(18) for x in (a, b)]   # every ordered pair of lengths
    strings += strings[:30]                                           # duplicates
    long = strings[:40] + [rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()] + strings[40:80]
    odd = strings + [b"z" * (1 + sum(len(s) for s in strings) % 2)]
    few = ((1, None), (3, _maps(3)[1]))
    for batch, owners in ((strings, few + ((2, None), (8, None))), (long, few), ([b""] * 200, few), (odd, few)):
        buf, offs = pack_strings(batch)
        nb = int(offs[-1])
        if batch is odd:
            assert nb % 2 == 1                                        # the text ends past `safe`: its tail is read by bytes
        for n_owners, omap in owners:
            got, ref, n, total = _run(gpu, buf, offs, nb, n_owners, omap)
            _check(got, ref, n, total)
            assert ref["n_bad"] == 0 and total == nb


@pytest.mark.gpu
def test_malformed_offsets_are_counted_and_never_followed(gpu, engine_lib):
    strings = _names(500, 77)
    buf, offs = pack_strings(strings)
    nb = int(offs[-1])
    cases = []
    dec = offs.copy()
    dec[100] = dec[101] + np.uint64(3)                                # string 100 ends in front of its start
    dec[300] = np.uint64(0)                                           # string 299 too
    cases.append((buf, dec, nb, 2))
    past = offs.copy()
    past[-1] = np.uint64(nb + 5)                                      # the last string ends past n_bytes
    past[200] = np.uint64(1 << 40)                                    # string 199 far past it, string 200 backwards
    cases.append((buf, past, nb, 3))
    big = np.zeros(70_000, dtype=np.uint8)
    big[:] = np.random.default_rng(1).integers(0, 256, big.shape[0])
    cases.append((big, np.array([0, 65537, 65537 + 100, 69_000, 69_000], dtype=np.uint64), 70_000, 1))
    cases.append((big, np.array([0, 65536, 70_000, 4_000, 70_000], dtype=np.uint64), 70_000, 2))
    for b, o, n_bytes, n_bad in cases:
        for n_owners in (1, 3):
            got, ref, n, total = _run(gpu, b, o, n_bytes, n_owners)
            assert ref["n_bad"] == n_bad
            _check(got, ref, n, total)                                # the guards are part of it


@pytest.mark.gpu
def test_text_vnode_loads_of_a_misaligned_slice(gpu, engine_lib):
    """A byte buffer that starts off an 8-byte boundary (a slice of a larger tensor) is copied to
    an aligned one, not refused; the loads equal the numpy count of the routing keys' nodes."""
    import torch
    strings = _names(1000, 5)
    buf, offs = pack_strings(strings)
    nb = int(offs[-1])
    with torch.cuda.stream(torch.cuda.Stream(gpu)):
        big = torch.zeros(buf.shape[0] + 16, dtype=torch.uint8, device=gpu)
        big[3:3 + buf.shape[0]] = torch.from_numpy(buf).to(gpu)
        view = big[3:3 + buf.shape[0]]
        assert view.data_ptr() % 8 == 3
        loads = cluster.text_vnode_loads(view, torch.from_numpy(offs.view(np.int64)).to(gpu), seed=9, n_bytes=nb)
        torch.cuda.current_stream(gpu).synchronize()
    want = np.bincount(cluster.key_vnode(cluster.text_route_keys(buf, offs, 9, nb)), minlength=cluster.OWNER_MAP_SIZE)
    assert np.array_equal(loads.cpu().numpy(), want)
