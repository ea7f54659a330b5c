"""Save, restart, restore (distributedratelimiting.redis_amd/snapshot.py): an engine that
is saved after three batches and restored into a fresh engine behind a fresh directory
(other ids), or into another number of owners, decides the rest of the stream exactly as
the engine that kept running, and as oracle.semantics.TokenBucketTable run uninterrupted.

The stream: 20,000 distinct keys, six batches of 30,000 requests, non-decreasing
timestamps; limit 5 at 2 tokens/s (TTL 3 s).  Batch 1 draws from the first 12,000 keys,
batch 2 from keys 3,000 to 12,000, batch 3 from keys 6,000 to 16,000 and ends 3.9 s after
the start, so the buckets last granted in batch 1 (keys below 3,000 among them) have lapsed
at the save and are not in the file; more lapse between the later batches.  Final states are
compared as the store holds them at the last timestamp (the live rows): a row that had
lapsed at the save is still in the running engine's table and absent in the restored
one, which decides the same from the save's timestamp on."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T0 = 1_760_000_000_000_000
N_KEYS, N_REQ, TABLE = 20_000, 30_000, 32_768
LIMIT, TOKENS, TICKS = 5, 2, 10_000_000
STARTS_S = [0.0, 1.5, 3.5, 5.0, 6.5, 8.5]            # batch starts; each batch spans 0.4 s
RANGES = [(0, 12_000), (3_000, 12_000), (6_000, 16_000), (4_000, 20_000), (4_000, 20_000), (0, 20_000)]
PREFIX = "resource-"


def _stream(gpu):
    import torch
    return torch.cuda.stream(torch.cuda.Stream(gpu))


@pytest.fixture(scope="module")
def trace():
    """The six batches by key index, the keys' global u64 names, and the uninterrupted
    oracle's replies and final live state; computed once, read-only."""
    from oracle.semantics import TokenBucketConfig, TokenBucketTable
    rng = np.random.default_rng(41)
    gkeys = np.unique(rng.integers(0, (1 << 64) - 1, N_KEYS + 64, dtype=np.uint64))
    gkeys = rng.permutation(gkeys)[:N_KEYS]
    assert gkeys.shape[0] == N_KEYS
    batches = []
    for start, (lo, hi) in zip(STARTS_S, RANGES):
        idx = rng.integers(lo, hi, N_REQ).astype(np.int64)
        p = rng.integers(0, 4, N_REQ).astype(np.int32)
        ts = np.sort(T0 + int(start * 1e6) + rng.integers(0, 400_000, N_REQ)).astype(np.int64)
        batches.append((idx, p, ts))
    table = TokenBucketTable(TokenBucketConfig.from_options(LIMIT, TOKENS, TICKS))
    replies = []
    for idx, p, ts in batches:
        g, r = table.acquire_batch(idx.tolist(), p.tolist(), ts.tolist())
        replies.append((np.array(g, dtype=np.uint8), np.array(r, dtype=np.int32)))
    ts_end = int(batches[-1][2][-1])
    final = {k: (np.float64(st.v).view(np.uint64), st.t_us) for k, st in list(table.state.items())
             if table.load(k, ts_end) is not None}
    return {"gkeys": gkeys, "batches": batches, "replies": replies, "final": final,
            "ts_save": int(batches[2][2][-1]), "ts_end": ts_end}


class Node:
    """One engine and the directory its keys go through ('keys', 'text' or 'ids')."""

    def __init__(self, form, gpu, gkeys, warm_up=0):
        from distributedratelimiting.redis_amd import TokenBucketEngine
        from distributedratelimiting.redis_amd.cluster import DeviceDirectory
        from distributedratelimiting.redis_amd.strdir import StringDirectory
        self.form, self.gpu, self.gkeys = form, gpu, gkeys
        self.eng = TokenBucketEngine(TABLE, LIMIT, TOKENS, TICKS, device=0)
        self.dir = {"keys": lambda: DeviceDirectory(TABLE, device=0),
                    "text": lambda: StringDirectory(TABLE, 1 << 20, prefix="limiter:", device=0),
                    "ids": lambda: None}[form]()
        if warm_up:                                   # unrelated keys first, so that its ids differ
            self.ids_of(np.arange(1_000_000, 1_000_000 + warm_up), gkeys=np.arange(1, 2_000_000, dtype=np.uint64))

    def ids_of(self, idx, gkeys=None):
        import torch
        from distributedratelimiting.redis_amd.strdir import synthetic_key_text
        d_idx = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(self.gpu)
        if self.form == "ids":
            return d_idx
        if self.form == "text":
            return self.dir.assign(*synthetic_key_text(d_idx, PREFIX))
        g = self.gkeys if gkeys is None else gkeys
        return self.dir.assign(torch.from_numpy(g[idx].view(np.int64)).to(self.gpu))

    def decide(self, idx, p, ts):
        import torch
        cur = torch.cuda.current_stream(self.gpu).cuda_stream
        d_ids = self.ids_of(idx)
        g = torch.empty(idx.shape[0], dtype=torch.uint8, device=self.gpu)
        r = torch.empty(idx.shape[0], dtype=torch.int32, device=self.gpu)
        self.eng.acquire_batch_device(d_ids, torch.from_numpy(p).to(self.gpu), torch.from_numpy(ts).to(self.gpu),
                                      g, r, stream=cur)
        return g, r

    def live(self, ts_us):
        """{key index: (v bits, t_us)} of the buckets alive at ts_us, through the directory."""
        import torch
        cur = torch.cuda.current_stream(self.gpu).cuda_stream
        d_ids, d_v, d_t = self.eng.export_live(ts_us, stream=cur)
        v, t = d_v.cpu().numpy().view(np.uint64), d_t.cpu().numpy()
        if self.form == "ids":
            names = d_ids.cpu().numpy().tolist()
        elif self.form == "keys":
            k = self.dir.keys_of(d_ids).cpu().numpy().view(np.uint64)
            order = np.argsort(self.gkeys)
            pos = np.searchsorted(self.gkeys[order], k)
            assert np.array_equal(self.gkeys[order][pos], k)          # every live bucket has a known key
            names = order[pos].tolist()
        else:
            buf, offs, missing = self.dir.text_of(d_ids, return_missing=True)
            assert missing == 0
            blob, o = buf.cpu().numpy().tobytes(), offs.cpu().numpy()
            names = [int(blob[o[i] + len(PREFIX):o[i + 1]]) for i in range(o.shape[0] - 1)]
            assert all(blob[o[i]:o[i] + len(PREFIX)] == PREFIX.encode() for i in range(0, o.shape[0] - 1, 97))
        assert len(set(names)) == len(names)
        return dict(zip(names, zip(v.tolist(), t.tolist())))

    def close(self):
        self.eng.close()
        if self.dir is not None:
            self.dir.close()


def _same(replies, want, what):
    import torch
    torch.cuda.synchronize()
    g, r = replies[0].cpu().numpy(), replies[1].cpu().numpy()
    print(what, "granted", int(g.sum()), "of", g.shape[0], "mismatches", int((g != want[0]).sum()),
          int((r != want[1]).sum()))
    assert np.array_equal(g, want[0]), what
    assert np.array_equal(r, want[1]), what


@pytest.mark.parametrize("form", ["keys", "text", "ids"])
def test_restart_behind_a_fresh_directory(engine_lib, gpu, trace, tmp_path, form):
    from distributedratelimiting.redis_amd import snapshot
    path = tmp_path / "engine.npz"
    with _stream(gpu):
        a = Node(form, gpu, trace["gkeys"])
        for b in range(3):
            _same(a.decide(*trace["batches"][b]), trace["replies"][b], f"A batch {b + 1}")
        reclaimed = 0
        if form == "text":                            # freed ids exist in A's directory at the save
            reclaimed = a.dir.reclaim(a.eng, trace["ts_save"])
            assert reclaimed > 0
        present = int((a.eng.export_state()[1] != np.iinfo(np.int64).min).sum())
        saved = snapshot.save(path, a.eng, trace["ts_save"], a.dir)
        assert 0 < saved < present + reclaimed       # the buckets that lapsed are not in the file
        assert saved == len(a.live(trace["ts_save"]))
        # B: a fresh engine; its directory has met 1,000 other keys, so ids differ from A's
        b_node = Node(form, gpu, trace["gkeys"], warm_up=0 if form == "ids" else 1_000)
        assert snapshot.load([path], b_node.eng, b_node.dir) == saved
        if form != "ids":
            probe = trace["batches"][2][0][:2_000]
            ia, ib = a.ids_of(probe).cpu().numpy(), b_node.ids_of(probe).cpu().numpy()
            assert (ia != ib).mean() > 0.9
        for b in range(3, 6):
            ra = a.decide(*trace["batches"][b])
            rb = b_node.decide(*trace["batches"][b])
            _same(ra, trace["replies"][b], f"A batch {b + 1}")
            _same(rb, trace["replies"][b], f"B batch {b + 1}")
        a.eng.synchronize()
        b_node.eng.synchronize()
        fa, fb = a.live(trace["ts_end"]), b_node.live(trace["ts_end"])
        assert fa == fb
        assert fa == {k: (int(v), t) for k, (v, t) in trace["final"].items()}
        a.close()
        b_node.close()


def test_reshard_two_owners_into_one_and_three(engine_lib, gpu, trace, tmp_path):
    from distributedratelimiting.redis_amd import snapshot
    from distributedratelimiting.redis_amd.cluster import key_owner
    gkeys = trace["gkeys"]

    def run(nodes, b):
        """Batch b split by owner, every owner's share in arrival order; replies back in place."""
        import torch
        idx, p, ts = trace["batches"][b]
        own = key_owner(gkeys[idx], len(nodes))
        parts = [(np.flatnonzero(own == r), nodes[r]) for r in range(len(nodes))]
        out = [(sel, node.decide(idx[sel], p[sel], ts[sel])) for sel, node in parts if sel.shape[0]]
        torch.cuda.synchronize()
        g, r = np.empty(N_REQ, dtype=np.uint8), np.empty(N_REQ, dtype=np.int32)
        for sel, (dg, dr) in out:
            g[sel], r[sel] = dg.cpu().numpy(), dr.cpu().numpy()
        return g, r

    with _stream(gpu):
        two = [Node("keys", gpu, gkeys) for _ in range(2)]
        for b in range(3):
            g, r = run(two, b)
            assert np.array_equal(g, trace["replies"][b][0]) and np.array_equal(r, trace["replies"][b][1])
        shards = [tmp_path / f"owner{r}.npz" for r in range(2)]
        saved = [snapshot.save(shards[r], two[r].eng, trace["ts_save"], two[r].dir) for r in range(2)]
        assert min(saved) > 0
        for world in (1, 3):
            nodes = [Node("keys", gpu, gkeys, warm_up=100 * (r + 1)) for r in range(world)]
            loaded = [snapshot.load(shards, nodes[r].eng, nodes[r].dir, owner=(r, world, None))
                      for r in range(world)]
            print("world", world, "saved", saved, "loaded", loaded)
            assert sum(loaded) == sum(saved) and min(loaded) > 0
            for b in range(3, 6):
                g, r = run(nodes, b)
                assert np.array_equal(g, trace["replies"][b][0]), (world, b)
                assert np.array_equal(r, trace["replies"][b][1]), (world, b)
            final = {}
            for node in nodes:
                node.eng.synchronize()
                part = node.live(trace["ts_end"])
                assert not set(part) & set(final)
                final.update(part)
            assert final == {k: (int(v), t) for k, (v, t) in trace["final"].items()}
            for node in nodes:
                node.close()
        for node in two:
            node.close()
