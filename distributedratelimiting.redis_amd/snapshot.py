"""Portable snapshots: the live buckets of an engine, saved by key and restored
(DESIGN.md §8 "Portable snapshots").

The reference keeps its buckets in Redis, where they outlive every client and are reached
by key whatever the number of clients.  Here a bucket lives in one engine's table under a
dense id, and an id is only a function of the order in which a directory met its keys.  A
snapshot therefore lists the live buckets as ``(key, v, t_us)``, ``key`` being what the
caller knows the bucket by:

- the global u64 key of a ``DeviceDirectory`` (arrays ``keys``);
- the resourceID text of a ``StringDirectory`` (arrays ``text_bytes`` + ``text_offs``);
- the dense id when there is no directory (array ``ids``).

``save`` writes one ``.npz`` (plain arrays: ``numpy.load(..., allow_pickle=False)`` reads it);
``load`` restores one or several of them into a fresh engine and directory, whose ids may
differ, and, with ``owner=``, into another number of owners.  Token-bucket and queueing
kinds: only bucket rows are saved (what ``tbe_import_state`` covers), queues are not.
Approximate kind: the replica of the global tier, rows ``(key, v, p, t_us)``; the tier is
replicated, so every rank loads every row and ``owner=`` is refused.

The export and the import run on the device (``tbe_export_live_device``,
``tbe_dir_keys_of_device`` / ``tbe_sdir_text_*_device``, ``tbe_import_rows_device`` and
their ``tbe_approx_*`` counterparts); this module moves the lists between the device and the
file.  ``live_rows``, ``approx_live_rows``, ``approx_idle_rows``, ``write``, ``read`` and
``merge`` need neither a GPU nor the engine library.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence, Tuple

import numpy as np

from .cluster import key_owner, text_route_keys

FORMAT_VERSION = 1
ABSENT = np.iinfo(np.int64).min
META_FIELDS = ("version", "kind", "token_limit", "fill_rate_bits", "ttl_ms", "ts_us")
KEY_FORMS = ("keys", "text", "ids")
KIND_APPROXIMATE = 2                   # tbe_kind TBE_KIND_APPROXIMATE
APPROX_TTL_MS = 86_400_000             # EXPIRE 86400 of the sync script (A:268)


def live_rows(v, t_us, ts_us: int, ttl_ms: int) -> np.ndarray:
    """Ascending ids (int64) of the rows that are live at ts_us: present (t_us != INT64_MIN)
    and not lapsed, t_us < 1000 * (ts_us // 1000 - ttl_ms) being a lapsed row -- the
    complement of tbe_expired_device's row rule.  ts_us < 0 skips the lapse test.  `v` is
    not read (a row's liveness is a matter of its timestamp alone)."""
    t_us = np.asarray(t_us, dtype=np.int64)
    live = t_us != ABSENT
    if ts_us >= 0:
        live &= ~(t_us < 1000 * (int(ts_us) // 1000 - int(ttl_ms)))
    return np.flatnonzero(live).astype(np.int64)


def _new_t(ts_us) -> np.ndarray:
    """TB:202-203 / A:241-242: now[1] + now[2] / 1000000 of injected microseconds, as f64."""
    ts_us = np.asarray(ts_us, dtype=np.int64)
    return (ts_us // 1_000_000).astype(np.float64) + (ts_us % 1_000_000).astype(np.float64) / np.float64(1e6)


def _approx_present(t_us: np.ndarray, ts_us: int) -> np.ndarray:
    live = t_us != ABSENT
    if ts_us >= 0:
        live &= ~(t_us < 1000 * (int(ts_us) // 1000 - APPROX_TTL_MS))
    return live


def approx_live_rows(t_us, ts_us: int, skip=None) -> np.ndarray:
    """Ascending ids (int64) of the approximate kind's tier rows that
    tbe_approx_export_live_device exports: present, not lapsed at ts_us by the sync script's
    one-day EXPIRE (A:268; ts_us < 0 skips the test), and with a zero byte in `skip` where a
    mask is given."""
    live = _approx_present(np.asarray(t_us, dtype=np.int64), ts_us)
    if skip is not None:
        live &= np.asarray(skip) == 0
    return np.flatnonzero(live).astype(np.int64)


def approx_idle_rows(local, global_score, queued, v, t_us, ts_us: int, decay_rate: float) -> np.ndarray:
    """tbe_approx_idle_device's rule per row, as a bool array.  `local`,
    `global_score` and `queued` are ``local_state``'s _localThrottleScore,
    _globalThrottleScore and queue length; `v`, `t_us` the tier row (``export_global``);
    decay_rate the fill rate.  A row is idle when nothing is queued, ConsumedTokens (A:36:
    global + local in C# unchecked int32) is 0, and the row gives a client syncing at ts_us
    nothing: absent, lapsed, or max(0, v - max(0, new_t(ts_us) - new_t(t_us)) * decay_rate)
    == 0 with Lua's max and the script's operation order (A:255-258)."""
    local = np.asarray(local).astype(np.int64)
    global_score = np.asarray(global_score).astype(np.int64)
    v = np.asarray(v, dtype=np.float64)
    t_us = np.asarray(t_us, dtype=np.int64)
    if ts_us < 0:
        raise ValueError("ts_us < 0")
    present = _approx_present(t_us, ts_us)
    x = _new_t(ts_us) - _new_t(np.where(present, t_us, 0))
    dt = np.where(x > 0.0, x, 0.0)                       # lua_max(0, x)
    y = v - dt * np.float64(decay_rate)                  # two roundings, no contraction
    worthless = ~present | (np.where(y > 0.0, y, 0.0) == 0.0)
    consumed = ((global_score + local) & 0xFFFFFFFF) != 0
    return (np.asarray(queued) == 0) & ~consumed & worthless


def option_meta(config, ts_us: int) -> np.ndarray:
    """The `meta` array of a snapshot for an engine's ``config`` (a ``_capi.TbeConfig`` or
    anything with its kind / token_limit / tokens_per_period / replenishment_period_ticks):
    META_FIELDS as int64.  The fill rate is FillRatePerSecond (TBO:82-85) as raw f64 bits
    and ttl_ms the script's EXPIRE (TB:234), both computed as the engine computes them; the
    approximate kind's rate is its decay rate (the same quotient, A:224) and its ttl_ms the
    sync script's one day (A:268)."""
    rate = np.float64(config.tokens_per_period) / (np.float64(config.replenishment_period_ticks) / np.float64(1e7))
    q = min(max(np.float64(config.token_limit) / rate, 1.0), 31536000.0)
    ttl_ms = APPROX_TTL_MS if int(config.kind) == KIND_APPROXIMATE else int(np.ceil(q)) * 1000
    bits = int(np.array([rate], dtype=np.float64).view(np.int64)[0])
    return np.array([FORMAT_VERSION, int(config.kind), int(config.token_limit), bits, ttl_ms, int(ts_us)],
                    dtype=np.int64)


def write(path, meta, v, t_us, keys=None, text=None, ids=None, p=None) -> None:
    """One snapshot file: `meta` (option_meta), `v` as its f64 bit pattern (u64), `t_us`
    (i64) and exactly one key form -- keys (u64), text = (bytes u8, offsets u64 [n + 1])
    or ids (u64).  `p` (the approximate kind's period estimates, one per row) adds an array
    ``p`` of f64 bit patterns; without it the file is a token-bucket file as before."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    t_us = np.ascontiguousarray(t_us, dtype=np.int64)
    n = v.shape[0]
    if sum(x is not None for x in (keys, text, ids)) != 1:
        raise ValueError("exactly one of keys, text and ids")
    arrays = {"meta": np.asarray(meta, dtype=np.int64), "v": v.view(np.uint64), "t_us": t_us}
    if p is not None:
        p = np.ascontiguousarray(p, dtype=np.float64)
        if p.shape[0] != n:
            raise ValueError("p must have one entry per row")
        arrays["p"] = p.view(np.uint64)
    if keys is not None:
        arrays["keys"] = np.ascontiguousarray(keys).astype(np.uint64, copy=False)
    elif ids is not None:
        arrays["ids"] = np.ascontiguousarray(ids).astype(np.uint64, copy=False)
    else:
        offs = np.ascontiguousarray(text[1]).astype(np.uint64, copy=False)
        if offs.shape[0] != n + 1:
            raise ValueError("text offsets must have n + 1 entries")
        arrays["text_offs"] = offs
        arrays["text_bytes"] = np.ascontiguousarray(text[0], dtype=np.uint8)[: int(offs[-1])]
    for name in ("keys", "ids"):
        if name in arrays and arrays[name].shape[0] != n:
            raise ValueError(f"{name} must have one entry per row")
    if t_us.shape[0] != n or arrays["meta"].shape != (len(META_FIELDS),):
        raise ValueError("malformed snapshot arrays")
    with open(path, "wb") as f:          # (np.savez would append ".npz" to a bare name)
        np.savez(f, **arrays)


def read(path) -> dict:
    """A snapshot file as a dict: meta (name -> int), form (one of KEY_FORMS), v (f64),
    t_us (i64), p (f64, approximate-kind files only) and keys / ids (u64) or text = (bytes
    u8, offsets u64)."""
    with np.load(path, allow_pickle=False) as z:
        meta = dict(zip(META_FIELDS, (int(x) for x in z["meta"])))
        if meta["version"] != FORMAT_VERSION:
            raise ValueError(f"{path}: snapshot format {meta['version']}, this build reads {FORMAT_VERSION}")
        out = {"meta": meta, "v": z["v"].view(np.float64), "t_us": z["t_us"].astype(np.int64, copy=False)}
        if "p" in z.files:
            out["p"] = z["p"].view(np.float64)
        if "keys" in z.files:
            out["form"], out["keys"] = "keys", z["keys"]
        elif "ids" in z.files:
            out["form"], out["ids"] = "ids", z["ids"]
        else:
            out["form"], out["text"] = "text", (z["text_bytes"], z["text_offs"])
    return out


def _form_of(directory) -> str:
    if directory is None:
        return "ids"
    return "text" if hasattr(directory, "text_of") else "keys"


def merge(paths: Sequence, config, form: str, owner: Optional[Tuple] = None) -> dict:
    """The host half of ``load``: read the shard files in the order given, check each
    against the engine's options and the directory's key form, keep the rows of `owner`
    (u64 keys by ``key_owner``; text by ``key_owner`` of ``text_route_keys(text, seed)``, seed
    being the optional fourth entry of `owner`, default 0) and refuse a key that occurs twice.
    Returns {form, v, t_us, keys | ids | text}, rows in file order, plus p for an approximate
    engine.  Raises ValueError as ``load`` documents."""
    if isinstance(paths, (str, bytes, os.PathLike)):
        paths = [paths]
    want = option_meta(config, 0)
    approx = int(config.kind) == KIND_APPROXIMATE
    if approx and owner is not None:
        raise ValueError("owner= splits buckets between owners; the approximate kind's tier is replicated: "
                         "every rank loads every row")
    shards = []
    for p in paths:
        s = read(p)
        m = s["meta"]
        if m["token_limit"] != int(want[2]) or m["fill_rate_bits"] != int(want[3]):
            raise ValueError(f"{p}: saved with token_limit {m['token_limit']} and fill-rate bits "
                             f"{m['fill_rate_bits']:#x}, the engine has {int(want[2])} and {int(want[3]):#x}")
        if (m["kind"] == KIND_APPROXIMATE) != approx or ("p" in s) != approx:
            raise ValueError(f"{p}: saved from an engine of kind {m['kind']}, the engine is of kind {int(config.kind)}")
        if s["form"] != form:
            raise ValueError(f"{p}: buckets saved by {s['form']}, the directory takes {form}")
        shards.append(s)
    v = np.concatenate([s["v"] for s in shards]) if shards else np.zeros(0, dtype=np.float64)
    t_us = np.concatenate([s["t_us"] for s in shards]) if shards else np.zeros(0, dtype=np.int64)
    out = {"form": form}
    if approx:
        out["p"] = np.concatenate([s["p"] for s in shards]) if shards else np.zeros(0, dtype=np.float64)
    if form == "text":
        lens = [np.diff(s["text"][1].astype(np.int64)) for s in shards]
        lens = np.concatenate(lens) if lens else np.zeros(0, dtype=np.int64)
        blob = b"".join(s["text"][0].tobytes() for s in shards)
        offs = np.zeros(lens.shape[0] + 1, dtype=np.int64)
        np.cumsum(lens, out=offs[1:])
        texts = [blob[offs[i]:offs[i + 1]] for i in range(lens.shape[0])]
        if len(set(texts)) != len(texts):
            raise ValueError("a key occurs twice across the shards")
        if owner is not None:            # by the routing key of the text (cluster.text_route_keys)
            rank, world, owner_map = owner[:3]
            seed = int(owner[3]) if len(owner) > 3 else 0
            keep = key_owner(text_route_keys(blob, offs, seed), int(world), owner_map) == int(rank)
            v, t_us, lens = v[keep], t_us[keep], lens[keep]
            blob = b"".join(t for t, k in zip(texts, keep.tolist()) if k)
            offs = np.zeros(lens.shape[0] + 1, dtype=np.int64)
            np.cumsum(lens, out=offs[1:])
        out["text"] = (np.frombuffer(blob, dtype=np.uint8), offs.astype(np.uint64))
    else:
        k = np.concatenate([s[form] for s in shards]) if shards else np.zeros(0, dtype=np.uint64)
        if np.unique(k).shape[0] != k.shape[0]:
            raise ValueError("a key occurs twice across the shards")
        if owner is not None:
            if form != "keys":
                raise ValueError("owner= selects by u64 key; id-keyed snapshots have none")
            rank, world, owner_map = owner[:3]
            keep = key_owner(k, int(world), owner_map) == int(rank)
            k, v, t_us = k[keep], v[keep], t_us[keep]
        out[form] = k
    out["v"], out["t_us"] = v, t_us
    return out


def _device_of(engine):
    import torch
    return torch.device("cuda", engine.config.device if engine.config.device >= 0 else torch.cuda.current_device())


def _unheld_mask(engine, directory):
    """uint8 device tensor over the engine's ids, 1 where `directory` holds no key for the id
    (tbe_approx_export_live_device's skip mask); None without a directory."""
    if directory is None:
        return None
    import torch
    dev = _device_of(engine)
    n = min(int(directory.capacity), int(engine.n_keys))
    skip = torch.ones(engine.n_keys, dtype=torch.uint8, device=dev)
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    if _form_of(directory) == "keys":
        skip[:n] = (directory.keys_of(ids) == -1).to(torch.uint8)
    else:
        _, offs, missing = directory.text_of(ids, return_missing=True)
        empty = (offs[1:] - offs[:-1]) == 0
        if int(empty.sum().item()) != missing:
            raise ValueError("the directory holds an empty key text: held and unheld ids cannot be told apart")
        skip[:n] = empty.to(torch.uint8)
    return skip


def save(path, engine, ts_us: int, directory=None, stream: Optional[int] = None) -> int:
    """Write the buckets of `engine` that are live at ts_us (ts_us < 0: every present one)
    to `path`, keyed through `directory` (a DeviceDirectory, a StringDirectory, or None for
    dense ids).  Ordered after every batch enqueued on the engine (`stream` as in
    ``export_live``).  Returns the number of rows written.  An ``ApproximateEngine``'s file
    holds its {v, p, t} tier rows (array ``p`` beside ``v``) for the ids the directory
    holds; local tiers and client views are in-process state and not saved."""
    if getattr(engine, "classed", False):
        raise ValueError("snapshot.save: the engine holds limit classes, and a snapshot file carries one "
                         "limiter's options and no per-key class; save a classed engine's rows with "
                         "export_live and its classes with get_class")
    approx = int(engine.config.kind) == KIND_APPROXIMATE
    if approx:
        # every synced id holds a tier row, held by a name or not: skip the ids the directory
        # does not hold (idle rows of held names stay: their p is the estimator's state)
        d_skip = _unheld_mask(engine, directory)
        if d_skip is not None and not stream:
            import torch
            torch.cuda.synchronize(d_skip.device)     # the mask is complete before the engine reads it
        d_ids, d_v, d_p, d_t = engine.export_live(ts_us, stream=stream, d_skip=d_skip)
    else:
        d_ids, d_v, d_t = engine.export_live(ts_us, stream=stream)
    if stream:
        import torch
        torch.cuda.synchronize(d_ids.device)
    meta = option_meta(engine.config, ts_us)
    v, t = d_v.cpu().numpy(), d_t.cpu().numpy()
    extra = {"p": d_p.cpu().numpy()} if approx else {}
    form = _form_of(directory)
    if form == "ids":
        write(path, meta, v, t, ids=d_ids.cpu().numpy().view(np.uint64), **extra)
    elif form == "keys":
        keys = directory.keys_of(d_ids).cpu().numpy().view(np.uint64)
        if (keys == np.uint64(0xFFFFFFFFFFFFFFFF)).any():
            raise ValueError("a live bucket's id is not held by the directory")
        write(path, meta, v, t, keys=keys, **extra)
    else:
        buf, offs, missing = directory.text_of(d_ids, return_missing=True)
        if missing:
            raise ValueError(f"{missing} live buckets' ids are not held by the directory")
        write(path, meta, v, t, text=(buf.cpu().numpy(), offs.cpu().numpy().view(np.uint64)), **extra)
    return int(v.shape[0])


def load(paths, engine, directory=None, owner: Optional[Tuple] = None, stream: Optional[int] = None) -> int:
    """Restore snapshot files into `engine` behind `directory`; returns the rows loaded.

    `paths`: one file or several shard files, processed in the order given, rows in file
    order (which is the order the directory first sees the keys in, hence their ids).
    Raises ValueError when a file's token_limit or fill-rate bits differ from the engine's,
    when its key form does not match the directory, or when a key occurs twice across the
    shards; nothing is imported then.  owner=(rank, world, owner_map_or_None[, seed]) keeps only
    the rows with ``cluster.key_owner(keys, world, owner_map) == rank``, for a text-keyed file
    with keys = ``cluster.text_route_keys(text, seed)`` (the key ``route_text_batch`` routes
    by; seed defaults to 0), so text-keyed state re-shards as u64-keyed state does.  The
    kept keys are assigned through the directory and the rows imported under the resulting
    ids (``import_rows``), ordered before every batch enqueued afterwards.  An
    ``ApproximateEngine`` takes approximate-kind files only (and the other kinds none of
    those), and refuses ``owner=``: its tier is replicated, every rank loads every row."""
    import torch
    rows = merge(paths, engine.config, _form_of(directory), owner)
    n = int(rows["v"].shape[0])
    if n == 0:
        return 0
    dev = _device_of(engine)
    if rows["form"] == "ids":
        d_ids = torch.from_numpy(rows["ids"].view(np.int64).copy()).to(dev)
    elif rows["form"] == "keys":
        d_ids = directory.assign(torch.from_numpy(rows["keys"].view(np.int64).copy()).to(dev))
        directory.check()
    else:
        blob, offs = rows["text"]
        buf = np.zeros((blob.shape[0] + 7) // 8 * 8 + 8, dtype=np.uint8)
        buf[: blob.shape[0]] = blob
        d_ids = directory.assign(torch.from_numpy(buf).to(dev), torch.from_numpy(offs.view(np.int64).copy()).to(dev),
                                 int(offs[-1]))
        directory.size()                 # raises once the directory is over capacity
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream or None
    if not stream:
        torch.cuda.synchronize(dev)      # the ids and rows are complete before the engine reads them
    extra = {"d_p": torch.from_numpy(rows["p"].copy()).to(dev)} if "p" in rows else {}
    engine.import_rows(d_ids, torch.from_numpy(rows["v"].copy()).to(dev),
                       torch.from_numpy(rows["t_us"].copy()).to(dev), stream=stream, **extra)
    return n


__all__ = ["FORMAT_VERSION", "live_rows", "approx_live_rows", "approx_idle_rows", "option_meta", "write", "read", "merge", "save", "load"]
