"""Python host mirror of the engine (tests, bench).  Every decision runs in the HIP
engine through the C ABI (``_capi``); this module only moves buffers.

``TokenBucketEngine`` corresponds to one ``RedisTokenBucketRateLimiterOptions`` /
``PartitionedRedisTokenBucketRateLimiter`` instance of the reference
(TokenBucket/PartitionedRedisTokenBucketRateLimiter.cs:7-55), with the per-request
``ScriptEvaluateAsync`` (PTB:42) replaced by ``acquire_batch``.
"""
from __future__ import annotations

import ctypes
from ctypes import byref, c_double, c_int32, c_uint32, c_void_p
from typing import Optional, Tuple

import numpy as np

from . import _capi
from ._capi import TbeError


def fill_rate(tokens_per_period: int, period_ticks: int) -> float:
    return _capi.load().tbe_fill_rate(tokens_per_period, period_ticks)


class PinnedArray:
    """A numpy array over page-locked host memory from ``tbe_alloc_host`` (the host-buffer
    calls copy it by DMA).  ``.array`` is valid until ``free()`` or collection of this
    object; keep the object alive while the array (or a view of it) is in use."""

    def __init__(self, n: int, dtype):
        self._lib = _capi.load()
        dt = np.dtype(dtype)
        nbytes = max(1, int(n) * dt.itemsize)
        p = c_void_p()
        st = self._lib.tbe_alloc_host(nbytes, byref(p))
        if st != 0 or not p.value:
            raise TbeError(st, f"tbe_alloc_host({nbytes}) failed")
        self._ptr = p.value
        buf = (ctypes.c_uint8 * nbytes).from_address(self._ptr)
        self.array = np.frombuffer(buf, dtype=np.uint8)[: int(n) * dt.itemsize].view(dt)

    def free(self) -> None:
        if self._ptr:
            self.array = None
            self._lib.tbe_free_host(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class TokenBucketEngine:
    KIND = _capi.TBE_KIND_TOKEN_BUCKET

    def __init__(self, n_keys: int, token_limit: int, tokens_per_period: int, period_ticks: int,
                 device: int = -1, stage_timing: bool = False, max_batch: int = 0,
                 queue_limit: int = 0, queue_order: int = 0, pack: bool = True, hot: bool = True,
                 pipeline: bool = True, narrow: bool = True, zero_wait_slots: int = 0,
                 fold_records: bool = True, digit_stream: bool = True, rerank: bool = False,
                 classes=None, stats: bool = False, approx_classes=None):
        """classes: extra limit classes 1.. as (token_limit, tokens_per_period, period_ticks)
        (tbe_create_classes; class 0 is this engine's own three options).
        approx_classes: the approximate kind's extra classes (``ApproximateEngine``).
        stats: keep lease statistics (TBE_FLAG_STATS; ``statistics``, ``stats_totals``)."""
        self._lib = _capi.load()
        # stage_timing: True (every stage), "fold" (the fold alone) or False
        flags = (_capi.TBE_FLAG_FOLD_TIMING if stage_timing == "fold"
                 else _capi.TBE_FLAG_STAGE_TIMING if stage_timing else 0)
        if not pack:
            flags |= _capi.TBE_FLAG_NO_PACK
        if not hot:
            flags |= _capi.TBE_FLAG_NO_HOT
        if not pipeline:
            flags |= _capi.TBE_FLAG_NO_PIPELINE
        if not narrow:
            flags |= _capi.TBE_FLAG_NO_NARROW
        if not fold_records:
            flags |= _capi.TBE_FLAG_UNSCATTER_ALL
        if not digit_stream:
            flags |= _capi.TBE_FLAG_HIST_RECORDS
        if rerank:
            flags |= _capi.TBE_FLAG_RERANK
        if stats:
            flags |= _capi.TBE_FLAG_STATS
        self.stats = bool(stats)
        self.config = _capi.make_config(n_keys, token_limit, tokens_per_period, period_ticks,
                                        kind=self.KIND, queue_limit=queue_limit,
                                        queue_order=queue_order, device=device, flags=flags,
                                        max_batch=max_batch, zero_wait_slots=zero_wait_slots)
        h = c_void_p()
        if classes and self.KIND == _capi.TBE_KIND_APPROXIMATE:
            raise ValueError("limit classes: token-bucket and queueing kinds only "
                             "(the approximate kind takes approx_classes=)")
        if approx_classes and self.KIND != _capi.TBE_KIND_APPROXIMATE:
            raise ValueError("approx_classes: approximate kind only")
        if approx_classes:
            # five options per class: (token_limit, tokens_per_period, period_ticks, queue_limit, order)
            extra = (_capi.TbeQueueClass * len(approx_classes))(
                *[_capi.TbeQueueClass(*(int(x) for x in c)) for c in approx_classes])
            st = self._lib.tbe_create_approx_classes(byref(self.config), extra, len(approx_classes), byref(h))
        elif classes and self.KIND == _capi.TBE_KIND_QUEUEING:
            # five options per class: (token_limit, tokens_per_period, period_ticks, queue_limit, order)
            extra = (_capi.TbeQueueClass * len(classes))(*[_capi.TbeQueueClass(*(int(x) for x in c)) for c in classes])
            st = self._lib.tbe_create_queue_classes(byref(self.config), extra, len(classes), byref(h))
        elif classes:
            extra = (_capi.TbeClass * len(classes))(*[_capi.TbeClass(int(a), int(b), int(c)) for a, b, c in classes])
            st = self._lib.tbe_create_classes(byref(self.config), extra, len(classes), byref(h))
        else:
            st = self._lib.tbe_create(byref(self.config), byref(h))
        if st != _capi.TBE_OK:
            raise TbeError(st, "tbe_create failed: " + self._lib.tbe_last_error(None).decode())
        self._h = h
        self.n_keys = n_keys
        self.classed = bool(classes) or bool(approx_classes)

    # ------------------------------------------------------------------ lifetime
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.tbe_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int) -> None:
        if st != _capi.TBE_OK:
            msg = self._lib.tbe_last_error(self._h).decode() if self._h else "disposed"
            raise TbeError(st, msg)

    @property
    def handle(self) -> c_void_p:
        if not self._h:
            raise TbeError(_capi.TBE_EDISPOSED, "engine disposed")
        return self._h

    # ------------------------------------------------------------------ decisions
    def acquire_batch(self, keys, permits, ts_us, granted=None, remaining=None) -> Tuple[np.ndarray, np.ndarray]:
        """Host arrays in, host arrays out (granted u8, remaining i32), arrival order.
        granted/remaining: optional output arrays (e.g. PinnedArray.array: with every
        buffer page-locked, large batches take the chunked path whose copies overlap the
        decisions)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        permits = np.ascontiguousarray(permits, dtype=np.int32)
        ts_us = np.ascontiguousarray(ts_us, dtype=np.int64)
        n = keys.shape[0]
        if permits.shape[0] != n or ts_us.shape[0] != n:
            raise ValueError("keys, permits and ts_us must have the same length")
        granted = np.empty(n, dtype=np.uint8) if granted is None else granted
        remaining = np.empty(n, dtype=np.int32) if remaining is None else remaining
        if granted.shape != (n,) or remaining.shape != (n,) or granted.dtype != np.uint8 or \
                remaining.dtype != np.int32 or not (granted.flags.c_contiguous and remaining.flags.c_contiguous):
            raise ValueError("granted must be u8[n] and remaining i32[n], contiguous")
        self._check(self._lib.tbe_acquire_batch(
            self.handle, keys.ctypes.data, permits.ctypes.data, ts_us.ctypes.data, n,
            granted.ctypes.data, remaining.ctypes.data))
        return granted, remaining

    def acquire_batch_device(self, d_keys, d_permits, d_ts, d_granted, d_remaining,
                             stream: Optional[int] = None) -> None:
        """Device tensors (torch, on this engine's GPU); enqueued, not synchronised.
        stream=None: the inputs must be complete now and the replies are complete at
        ``synchronize()``; a stream handle orders both on that stream (tbe.h)."""
        n = d_keys.numel()
        self._check(self._lib.tbe_acquire_batch_device(
            self.handle, d_keys.data_ptr(), d_permits.data_ptr(), d_ts.data_ptr(), n,
            d_granted.data_ptr(), d_remaining.data_ptr(), stream))

    def synchronize(self) -> None:
        self._check(self._lib.tbe_synchronize(self.handle))

    # ------------------------------------------------------------------ state
    def query(self, key: int, ts_us: int = -1) -> Optional[Tuple[float, float]]:
        v, t, present = c_double(), c_double(), c_int32()
        self._check(self._lib.tbe_query(self.handle, key, ts_us, byref(v), byref(t), byref(present)))
        return (v.value, t.value) if present.value else None

    def export_state(self, first: int = 0, count: Optional[int] = None):
        if count is None:
            count = self.n_keys - first
        v = np.empty(count, dtype=np.float64)
        t = np.empty(count, dtype=np.int64)
        self._check(self._lib.tbe_export_state(self.handle, first, count, v.ctypes.data,
                                               t.ctypes.data))
        return v, t

    def import_state(self, v, t_us, first: int = 0) -> None:
        """Restore rows [first, first + len) from an export_state snapshot (tbe_import_state)."""
        v = np.ascontiguousarray(v, dtype=np.float64)
        t_us = np.ascontiguousarray(t_us, dtype=np.int64)
        if v.shape != t_us.shape:
            raise ValueError("v and t_us must have the same length")
        self._check(self._lib.tbe_import_state(self.handle, first, v.shape[0], v.ctypes.data,
                                               t_us.ctypes.data))

    def expired_device(self, ts_us: int, d_dead, first: int = 0, clear: bool = False,
                       stream: Optional[int] = None) -> None:
        """d_dead (uint8 device tensor): d_dead[k - first] = 1 for every key of [first, first +
        len) whose Redis hash would not exist at ts_us (tbe_expired_device); clear=True also
        rewrites the lapsed rows absent.  Enqueued, not synchronised; stream as in
        ``acquire_batch_device``."""
        self._check(self._lib.tbe_expired_device(self.handle, ts_us, first, d_dead.numel(), d_dead.data_ptr(),
                                                 1 if clear else 0, stream))

    def export_live_device(self, ts_us: int, d_ids, d_v, d_t_us, d_n_live, first: int = 0,
                           count: Optional[int] = None, capacity: Optional[int] = None,
                           stream: Optional[int] = None) -> None:
        """One tbe_export_live_device call into caller tensors (int64 ids, float64 v, int64
        t_us, one-element int64 count); capacity defaults to d_ids.numel(), and capacity 0
        with d_ids = d_v = d_t_us = None only counts.  Enqueued, not synchronised."""
        if count is None:
            count = self.n_keys - first
        if capacity is None:
            capacity = 0 if d_ids is None else d_ids.numel()
        if capacity and min(d_ids.numel(), d_v.numel(), d_t_us.numel()) < capacity:
            raise ValueError("capacity exceeds the output tensors")
        ptr = (lambda t: None if t is None else t.data_ptr())
        self._check(self._lib.tbe_export_live_device(self.handle, ts_us, first, count, ptr(d_ids), ptr(d_v),
                                                     ptr(d_t_us), capacity, d_n_live.data_ptr(), stream))

    def export_live(self, ts_us: int, first: int = 0, count: Optional[int] = None, stream: Optional[int] = None):
        """The live rows of [first, first + count) at ts_us as int64 ids, float64 v and int64
        t_us device tensors, ascending ids (tbe_export_live_device; ts_us < 0: every present
        row).  A counting call, one read-back of the count (the device is synchronised for
        it), then the filling call: ordered on `stream` when one is given, complete on return
        otherwise."""
        import torch
        if count is None:
            count = self.n_keys - first
        dev = torch.device("cuda", self.config.device if self.config.device >= 0 else torch.cuda.current_device())
        d_n = torch.zeros(1, dtype=torch.int64, device=dev)
        self._check(self._lib.tbe_export_live_device(self.handle, ts_us, first, count, None, None, None, 0,
                                                     d_n.data_ptr(), stream))
        torch.cuda.synchronize(dev)
        n = int(d_n.item())
        d_ids = torch.empty(n, dtype=torch.int64, device=dev)
        d_v = torch.empty(n, dtype=torch.float64, device=dev)
        d_t = torch.empty(n, dtype=torch.int64, device=dev)
        if n:
            self._check(self._lib.tbe_export_live_device(self.handle, ts_us, first, count, d_ids.data_ptr(),
                                                         d_v.data_ptr(), d_t.data_ptr(), n, d_n.data_ptr(), stream))
            if not stream:
                torch.cuda.synchronize(dev)
        return d_ids, d_v, d_t

    def import_rows(self, d_ids, d_v, d_t_us, stream: Optional[int] = None) -> None:
        """table[d_ids[i]] = {d_v[i], d_t_us[i]} from device tensors (tbe_import_rows_device);
        enqueued, an invalid row voids the call and raises at ``synchronize()``."""
        n = d_ids.numel()
        if d_v.numel() != n or d_t_us.numel() != n:
            raise ValueError("d_ids, d_v and d_t_us must have the same length")
        d_ids, d_v, d_t_us = d_ids.contiguous(), d_v.contiguous(), d_t_us.contiguous()
        self._check(self._lib.tbe_import_rows_device(self.handle, d_ids.data_ptr(), d_v.data_ptr(),
                                                     d_t_us.data_ptr(), n, stream))
        self._rows_in_flight = (d_ids, d_v, d_t_us)   # read by the enqueued kernels

    # ------------------------------------------------------------------ live owner-map change
    def migrate_out_device(self, ts_us: int, d_key_of_id, d_owner_map, n_owners: int, self_rank: int, d_rows,
                           d_counts, d_leaving=None, commit: bool = False, first: int = 0,
                           capacity: Optional[int] = None, stream: Optional[int] = None, row_ids=None) -> None:
        """One tbe_migrate_out_device call over ids [first, first + d_key_of_id.numel()): the
        live rows of the ids whose key (int64 device tensor, -1 = unheld) `d_owner_map` (uint8
        device tensor of 4096 owners, or None for the hash partition) gives to another owner
        than self_rank, packed as int64 {key, bits of v, t_us, class} into d_rows grouped by
        destination; d_counts (int64, n_owners + 2): rows per owner, leaving ids, orphans;
        d_leaving (uint8, one per id, optional): 1 where the id's key leaves.  capacity (rows)
        defaults to what d_rows holds; 0 with d_rows=None only counts.  commit=True also
        rewrites the leaving rows absent.  row_ids (int64 device tensor of at least capacity
        entries, optional): row_ids[j] = the id whose row is d_rows[j] (tbe_migrate_out_ids_device).
        Enqueued; a refused call raises at ``synchronize()``."""
        self._migrate_out_device(self._lib.tbe_migrate_out_ids_device, ts_us, d_key_of_id, d_owner_map, n_owners,
                                 self_rank, d_rows, d_counts, d_leaving, commit, first, capacity, stream, row_ids)

    def _migrate_out_device(self, fn, ts_us, d_key_of_id, d_owner_map, n_owners, self_rank, d_rows, d_counts,
                            d_leaving, commit, first, capacity, stream, row_ids) -> None:
        # fn: tbe_migrate_out_ids_device, or the queueing kind's entry point of the same signature
        count = d_key_of_id.numel()
        if capacity is None:
            capacity = 0 if d_rows is None else d_rows.numel() // 4
        if capacity and (d_rows is None or d_rows.numel() < 4 * capacity or not d_rows.is_contiguous()):
            raise ValueError("capacity exceeds d_rows")
        if d_counts.numel() < n_owners + 2 or d_counts.element_size() != 8:
            raise ValueError("d_counts must hold n_owners + 2 64-bit counters")
        if d_leaving is not None and (d_leaving.numel() != count or d_leaving.element_size() != 1):
            raise ValueError("d_leaving must hold one byte per id")
        if d_owner_map is not None and (d_owner_map.numel() != 4096 or d_owner_map.element_size() != 1):
            raise ValueError("the owner map must be 4096 uint8 entries")
        if not d_key_of_id.is_contiguous() or d_key_of_id.element_size() != 8:
            raise ValueError("d_key_of_id must be a contiguous 64-bit tensor")
        if row_ids is not None and (row_ids.numel() < capacity or row_ids.element_size() != 8
                                    or not row_ids.is_contiguous()):
            raise ValueError("row_ids must be a contiguous 64-bit tensor of at least capacity entries")
        ptr = (lambda t: None if t is None else t.data_ptr())
        self._check(fn(
            self.handle, ts_us, first, count, d_key_of_id.data_ptr(), ptr(d_owner_map), n_owners, self_rank,
            ptr(d_rows) if capacity else None, capacity, d_counts.data_ptr(), ptr(d_leaving), 1 if commit else 0,
            ptr(row_ids) if capacity else None, stream))
        self._migrate_in_flight = (d_key_of_id, d_owner_map)   # read by the enqueued kernels

    def migrate_out(self, ts_us: int, key_of_id, owner_map, n_owners: int, self_rank: int, commit: bool = False,
                    first: int = 0, capacity: Optional[int] = None, row_ids: bool = False):
        """The same with host arrays (tbe_migrate_out; synchronous): returns (rows int64
        [capacity, 4] of which the first min(total, capacity) are written, counts uint64
        [n_owners + 2], leaving uint8 [count]).  capacity defaults to the number of ids.
        row_ids=True (tbe_migrate_out_ids) appends the rows' ids, uint64 [capacity], written as
        far as the rows are."""
        return self._migrate_out(self._lib.tbe_migrate_out_ids, ts_us, key_of_id, owner_map, n_owners, self_rank,
                                 commit, first, capacity, row_ids)

    def _migrate_out(self, fn, ts_us, key_of_id, owner_map, n_owners, self_rank, commit, first, capacity, row_ids):
        key_of_id = np.ascontiguousarray(key_of_id, dtype=np.uint64)
        count = key_of_id.shape[0]
        if owner_map is not None:
            owner_map = np.ascontiguousarray(owner_map, dtype=np.uint8)
            if owner_map.shape != (4096,):
                raise ValueError("the owner map must be 4096 uint8 entries")
        if capacity is None:
            capacity = count
        rows = np.zeros((capacity, 4), dtype=np.int64)
        counts = np.zeros(n_owners + 2, dtype=np.uint64)
        leaving = np.zeros(count, dtype=np.uint8)
        ids = np.zeros(capacity, dtype=np.uint64) if row_ids else None
        self._check(fn(
            self.handle, ts_us, first, count, key_of_id.ctypes.data,
            None if owner_map is None else owner_map.ctypes.data, n_owners, self_rank,
            rows.ctypes.data if capacity else None, capacity, counts.ctypes.data, leaving.ctypes.data,
            1 if commit else 0, ids.ctypes.data if row_ids and capacity else None))
        return (rows, counts, leaving, ids) if row_ids else (rows, counts, leaving)

    # ------------------------------------------------------------------ limit classes
    def classes(self):
        """Every class's (token_limit, tokens_per_period, period_ticks), class 0 first (tbe_classes)."""
        n = c_uint32()
        self._check(self._lib.tbe_classes(self.handle, None, 0, byref(n)))
        out = (_capi.TbeClass * n.value)()
        self._check(self._lib.tbe_classes(self.handle, out, n.value, byref(n)))
        return [(c.token_limit, c.tokens_per_period, c.replenishment_period_ticks) for c in out]

    def set_class(self, ids, cls) -> None:
        """cls[ids[i]] = cls[i] from host arrays; synchronous, an invalid pair raises and writes
        nothing (tbe_set_class)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        cls = np.ascontiguousarray(cls, dtype=np.uint8)
        if ids.shape != cls.shape:
            raise ValueError("ids and cls must have the same length")
        self._check(self._lib.tbe_set_class(self.handle, ids.ctypes.data, cls.ctypes.data, ids.shape[0]))

    def set_class_device(self, d_ids, d_cls, stream: Optional[int] = None) -> None:
        """The same from device tensors (int64 or uint64 ids, uint8 classes); enqueued, an invalid
        pair voids the call and raises at ``synchronize()`` (tbe_set_class_device)."""
        n = d_ids.numel()
        if d_cls.numel() != n:
            raise ValueError("d_ids and d_cls must have the same length")
        d_ids, d_cls = d_ids.contiguous(), d_cls.contiguous()
        self._check(self._lib.tbe_set_class_device(self.handle, d_ids.data_ptr(), d_cls.data_ptr(), n, stream))
        self._cls_in_flight = (d_ids, d_cls)   # read by the enqueued kernels

    def get_class(self, ids) -> np.ndarray:
        """The classes of ids (host arrays; synchronous; tbe_get_class)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        out = np.empty(ids.shape[0], dtype=np.uint8)
        self._check(self._lib.tbe_get_class(self.handle, ids.ctypes.data, ids.shape[0], out.ctypes.data))
        return out

    def get_class_device(self, d_ids, d_cls, stream: Optional[int] = None) -> None:
        """d_cls[i] = class of d_ids[i], device tensors; enqueued (tbe_get_class_device)."""
        n = d_ids.numel()
        if d_cls.numel() != n or not d_ids.is_contiguous() or not d_cls.is_contiguous():
            raise ValueError("d_ids and d_cls must be contiguous and of the same length")
        self._check(self._lib.tbe_get_class_device(self.handle, d_ids.data_ptr(), n, d_cls.data_ptr(), stream))

    # ------------------------------------------------------------------ lease statistics
    def statistics(self, keys, ts_us: int = 0):
        """(ok u64, failed u64, available i32, queued u32) of `keys` (host array; keys may
        repeat): the GA ``GetStatistics()`` fields per key (tbe_stats_batch; synchronous).
        Without ``stats=True`` ok and failed are None; available and queued work on every
        engine.  ts_us: when `available` is evaluated (ignored by the approximate kind)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        n = keys.shape[0]
        ok = np.empty(n, dtype=np.uint64) if self.stats else None
        failed = np.empty(n, dtype=np.uint64) if self.stats else None
        avail = np.empty(n, dtype=np.int32)
        queued = np.empty(n, dtype=np.uint32)
        ptr = (lambda a: None if a is None else a.ctypes.data)
        self._check(self._lib.tbe_stats_batch(self.handle, keys.ctypes.data, n, ts_us, ptr(ok), ptr(failed),
                                              avail.ctypes.data, queued.ctypes.data))
        return ok, failed, avail, queued

    def statistics_device(self, d_keys, ts_us: int = 0, d_ok=None, d_failed=None, d_available=None,
                          d_queued=None, stream: Optional[int] = None) -> None:
        """The same into device tensors (int64 ok / failed, int32 available and queued), any of
        which may be None; enqueued, a key >= n_keys voids the call and raises at
        ``synchronize()`` (tbe_stats_batch_device)."""
        ptr = (lambda t: None if t is None else t.data_ptr())
        self._check(self._lib.tbe_stats_batch_device(self.handle, d_keys.data_ptr(), d_keys.numel(), ts_us,
                                                     ptr(d_ok), ptr(d_failed), ptr(d_available), ptr(d_queued),
                                                     stream))

    def stats_totals(self) -> Tuple[int, int]:
        """(TotalSuccessfulLeases, TotalFailedLeases) of the whole engine (tbe_stats_totals)."""
        ok, failed = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.tbe_stats_totals(self.handle, byref(ok), byref(failed)))
        return ok.value, failed.value

    def stats_export(self, first: int = 0, count: Optional[int] = None):
        """(ok u64, failed u64) of keys [first, first + count) (tbe_stats_export)."""
        if count is None:
            count = self.n_keys - first
        ok = np.empty(count, dtype=np.uint64)
        failed = np.empty(count, dtype=np.uint64)
        self._check(self._lib.tbe_stats_export(self.handle, first, count, ok.ctypes.data, failed.ctypes.data))
        return ok, failed

    def stats_import(self, ok, failed, first: int = 0) -> None:
        """Counters of keys [first, first + len) from host arrays; the totals move by the
        difference (tbe_stats_import)."""
        ok = np.ascontiguousarray(ok, dtype=np.uint64)
        failed = np.ascontiguousarray(failed, dtype=np.uint64)
        if ok.shape != failed.shape:
            raise ValueError("ok and failed must have the same length")
        self._check(self._lib.tbe_stats_import(self.handle, first, ok.shape[0], ok.ctypes.data, failed.ctypes.data))

    def layout(self) -> dict:
        """{passes, r_bits, packed, hot, pipeline, narrow, medium, fold_records, digit_stream, rerank,
        narrow_pass0, queue_header_32} of this engine's
        batch pipeline (tbe_layout)."""
        a, b, c = c_uint32(), c_uint32(), c_uint32()
        self._check(self._lib.tbe_layout(self.handle, byref(a), byref(b), byref(c)))
        return {"passes": a.value, "r_bits": b.value, "packed": bool(c.value & 1),
                "hot": bool(c.value & 2), "pipeline": bool(c.value & 4), "narrow": bool(c.value & 8),
                "medium": bool(c.value & 16), "fold_records": bool(c.value & 32),
                "digit_stream": bool(c.value & 64), "rerank": bool(c.value & 128),
                "narrow_pass0": bool(c.value & 256), "queue_header_32": bool(c.value & 512)}

    def batch_format(self, n: int) -> dict:
        """The record layout a batch of n requests takes (tbe_batch_format)."""
        out = (c_uint32 * 9)()
        self._check(self._lib.tbe_batch_format(self.handle, n, out, 9))
        names = ("passes", "fold_records", "position_bits", "fold_time_bits", "key_bits", "permit_bits",
                 "pass0_time_bits", "r_bits", "sparse")
        return {k: (bool(out[i]) if k in ("fold_records", "sparse") else out[i]) for i, k in enumerate(names)}

    def stage_times(self) -> dict:
        out = (c_double * len(_capi.STAGES))()
        nw = c_uint32()
        self._check(self._lib.tbe_stage_times(self.handle, out, len(_capi.STAGES), byref(nw)))
        return {name: out[i] for i, name in enumerate(_capi.STAGES[: nw.value])}


class QueueingTokenBucketEngine(TokenBucketEngine):
    """TokenBucketWithQueue (TokenBucketWithQueue/RedisTokenBucketRateLimiter.cs, Q):
    WaitAsyncCore (Q:67-134) as ``wait_batch``, the timer drain (Q:237-271) as ``refresh``."""

    KIND = _capi.TBE_KIND_QUEUEING

    def __init__(self, n_keys: int, token_limit: int, tokens_per_period: int, period_ticks: int,
                 queue_limit: int, queue_order: int = 0, **kw):
        super().__init__(n_keys, token_limit, tokens_per_period, period_ticks,
                         queue_limit=queue_limit, queue_order=queue_order, **kw)
        self.queue_limit = queue_limit
        # queue_of's buffer size: the longest ring of any class (the engine validated them)
        self._ring_len = max([max(1, queue_limit)] +
                             [max(1, q[3]) for q in (self._five_option_classes() if self.classed else [])])

    def _five_option_classes(self):
        return self.queue_classes()

    def queue_classes(self):
        """Every class's (token_limit, tokens_per_period, period_ticks, queue_limit, order),
        class 0 first (tbe_queue_classes)."""
        n = c_uint32()
        self._check(self._lib.tbe_queue_classes(self.handle, None, 0, byref(n)))
        out = (_capi.TbeQueueClass * n.value)()
        self._check(self._lib.tbe_queue_classes(self.handle, out, n.value, byref(n)))
        return [(c.token_limit, c.tokens_per_period, c.replenishment_period_ticks, c.queue_limit, c.queue_order)
                for c in out]

    def wait_batch(self, keys, permits, ts_us, id_base: int, status=None, remaining=None):
        """Returns (status u8, remaining i32, evicted (cause index u64, request id i64)).
        `status` / `remaining` may be caller arrays (e.g. PinnedArray: with page-locked
        inputs too, batches of >= 2 chunks take the overlapped chunked path)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        permits = np.ascontiguousarray(permits, dtype=np.int32)
        ts_us = np.ascontiguousarray(ts_us, dtype=np.int64)
        n = keys.shape[0]
        status = np.empty(n, dtype=np.uint8) if status is None else status
        remaining = np.empty(n, dtype=np.int32) if remaining is None else remaining
        n_ev = ctypes.c_uint64()
        self._check(self._lib.tbe_wait_batch(self.handle, keys.ctypes.data, permits.ctypes.data,
                                             ts_us.ctypes.data, n, id_base, status.ctypes.data,
                                             remaining.ctypes.data, byref(n_ev)))
        m = n_ev.value
        cause = np.empty(m, dtype=np.uint64)
        ids = np.empty(m, dtype=np.int64)
        nw = ctypes.c_uint64()
        if m:
            self._check(self._lib.tbe_evicted(self.handle, cause.ctypes.data, ids.ctypes.data, m, byref(nw)))
        return status, remaining, (cause, ids)

    def attempt_batch(self, keys, permits, ts_us):
        """AttemptAcquire (lease or fail, never queue); returns (status u8, remaining i32)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        permits = np.ascontiguousarray(permits, dtype=np.int32)
        ts_us = np.ascontiguousarray(ts_us, dtype=np.int64)
        n = keys.shape[0]
        status = np.empty(n, dtype=np.uint8)
        remaining = np.empty(n, dtype=np.int32)
        self._check(self._lib.tbe_queue_attempt_batch(self.handle, keys.ctypes.data, permits.ctypes.data,
                                                      ts_us.ctypes.data, n, status.ctypes.data,
                                                      remaining.ctypes.data))
        return status, remaining

    def wait_batch_device(self, d_keys, d_permits, d_ts, d_status, d_remaining, id_base: int,
                          wait: bool = True, stream: Optional[int] = None) -> None:
        """Device tensors in and out; enqueued, not synchronised (tbe_wait_batch_device).
        NewestFirst evictions: ``evicted()`` after the call."""
        n = d_keys.numel()
        self._check(self._lib.tbe_wait_batch_device(
            self.handle, d_keys.data_ptr(), d_permits.data_ptr(), d_ts.data_ptr(), n, id_base,
            1 if wait else 0, d_status.data_ptr(), d_remaining.data_ptr(), stream))

    def evicted(self):
        """(cause index u64, request id i64) of the last wait batch, sorted (tbe_evicted)."""
        nw = ctypes.c_uint64()
        self._check(self._lib.tbe_evicted(self.handle, None, None, 0, byref(nw)))
        # capacity 0 fetched the log; a second call copies it out
        cap = 1 << 20
        while True:
            cause = np.empty(cap, dtype=np.uint64)
            ids = np.empty(cap, dtype=np.int64)
            self._check(self._lib.tbe_evicted(self.handle, cause.ctypes.data, ids.ctypes.data, cap,
                                              byref(nw)))
            if nw.value < cap:
                return cause[: nw.value], ids[: nw.value]
            cap *= 4

    def refresh_bound(self) -> int:
        b = ctypes.c_uint64()
        self._check(self._lib.tbe_refresh_bound(self.handle, byref(b)))
        return b.value

    def refresh_device(self, ts_us: int, d_keyseq, d_ids, d_rem, d_count,
                       stream: Optional[int] = None, classes=None) -> None:
        """Enqueue one replenish tick; the drain log lands in the device tensors
        (capacity = d_keyseq.numel(), which must be >= refresh_bound()).  ``classes``: an
        iterable of class numbers; the tick drains those classes' keys alone and leaves every
        other key untouched (tbe_refresh_classes_device)."""
        if classes is not None:
            self._check(self._lib.tbe_refresh_classes_device(
                self.handle, ts_us, _capi.class_mask(classes), d_keyseq.data_ptr(), d_ids.data_ptr(),
                d_rem.data_ptr(), d_keyseq.numel(), d_count.data_ptr(), stream))
            return
        self._check(self._lib.tbe_refresh_device(self.handle, ts_us, d_keyseq.data_ptr(), d_ids.data_ptr(),
                                                 d_rem.data_ptr(), d_keyseq.numel(), d_count.data_ptr(),
                                                 stream))

    def wait_batch_tick_device(self, d_keys, d_permits, d_ts, d_status, d_remaining, id_base: int,
                               tick_ts_us: int, d_keyseq, d_ids, d_rem, d_count, wait: bool = True,
                               stream: Optional[int] = None, classes=None) -> None:
        """``wait_batch_device`` then ``refresh_device(tick_ts_us)`` as one fused call
        (tbe_wait_batch_tick_device); the log capacity must cover ``refresh_bound()`` after
        the batch.  ``classes``: the batch is decided for every class and the fused tick drains
        the named classes alone (tbe_wait_batch_tick_classes_device)."""
        n = d_keys.numel()
        if classes is not None:
            self._check(self._lib.tbe_wait_batch_tick_classes_device(
                self.handle, d_keys.data_ptr(), d_permits.data_ptr(), d_ts.data_ptr(), n, id_base,
                1 if wait else 0, d_status.data_ptr(), d_remaining.data_ptr(), tick_ts_us,
                _capi.class_mask(classes), d_keyseq.data_ptr(), d_ids.data_ptr(), d_rem.data_ptr(),
                d_keyseq.numel(), d_count.data_ptr(), stream))
            return
        self._check(self._lib.tbe_wait_batch_tick_device(
            self.handle, d_keys.data_ptr(), d_permits.data_ptr(), d_ts.data_ptr(), n, id_base,
            1 if wait else 0, d_status.data_ptr(), d_remaining.data_ptr(), tick_ts_us, d_keyseq.data_ptr(),
            d_ids.data_ptr(), d_rem.data_ptr(), d_keyseq.numel(), d_count.data_ptr(), stream))

    def refresh(self, ts_us: int, classes=None):
        """One replenish tick; returns (keys u64, request ids i64, remaining i32) in (key, drain) order.
        ``classes``: an iterable of class numbers whose keys the tick drains (tbe_refresh_classes:
        each limiter's own timer in the reference); every other key is left untouched."""
        n = ctypes.c_uint64()
        if classes is None:
            self._check(self._lib.tbe_refresh(self.handle, ts_us, byref(n)))
        else:
            self._check(self._lib.tbe_refresh_classes(self.handle, ts_us, _capi.class_mask(classes), byref(n)))
        m = n.value
        keys = np.empty(m, dtype=np.uint64)
        ids = np.empty(m, dtype=np.int64)
        rem = np.empty(m, dtype=np.int32)
        nw = ctypes.c_uint64()
        if m:
            self._check(self._lib.tbe_refresh_log(self.handle, keys.ctypes.data, ids.ctypes.data,
                                                  rem.ctypes.data, m, byref(nw)))
        return keys, ids, rem

    def queue_of(self, key: int):
        cap = self._ring_len + getattr(self, "zero_wait_slots", 0)
        ids = np.empty(cap, dtype=np.int64)
        ps = np.empty(cap, dtype=np.int32)
        cnt = c_uint32()
        self._check(self._lib.tbe_queue_of(self.handle, key, ids.ctypes.data, ps.ctypes.data, cap,
                                           byref(cnt)))
        c = min(cnt.value, cap)
        return list(zip(ids[:c].tolist(), ps[:c].tolist()))

    def cancel(self, keys, request_ids):
        """Cancel queued requests (CancelQueueState.TrySetCanceled, Q:480-506 / A:531-557;
        tbe_queue_cancel); returns u8[n], 1 where the request was queued and is removed."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        request_ids = np.ascontiguousarray(request_ids, dtype=np.int64)
        n = keys.shape[0]
        if request_ids.shape[0] != n:
            raise ValueError("keys and request_ids differ in length")
        out = np.empty(n, dtype=np.uint8)
        m = ctypes.c_uint64()
        self._check(self._lib.tbe_queue_cancel(self.handle, keys.ctypes.data, request_ids.ctypes.data,
                                               n, out.ctypes.data, byref(m)))
        return out

    # ------------------------------------------------------------------ bulk queue export / import
    def queue_export_ids_device(self, d_ids, d_qcount, d_entry_start, d_entries, d_n_entries, clear: bool = False,
                                capacity: Optional[int] = None, stream: Optional[int] = None) -> None:
        """One tbe_queue_export_ids_device call: the queues of the listed ids (64-bit device
        tensor) into d_qcount (int32/uint32, one per id), d_entry_start (64-bit, one per id and
        one more, or None), d_entries (64-bit ``request_id << 16 | permits`` words, oldest
        first, or None with capacity 0: only count) and d_n_entries (one 64-bit word).
        capacity (entries) defaults to what d_entries holds.  clear=True also empties the listed
        queues; a clearing call whose entries do not fit changes nothing.  Enqueued; a refused
        call raises at ``synchronize()``."""
        n = d_ids.numel()
        if capacity is None:
            capacity = 0 if d_entries is None else d_entries.numel()
        if capacity and (d_entries is None or d_entries.numel() < capacity or d_entries.element_size() != 8
                         or not d_entries.is_contiguous()):
            raise ValueError("capacity exceeds d_entries")
        if not d_ids.is_contiguous() or d_ids.element_size() != 8:
            raise ValueError("d_ids must be a contiguous 64-bit tensor")
        if d_qcount.numel() < n or d_qcount.element_size() != 4 or not d_qcount.is_contiguous():
            raise ValueError("d_qcount must hold one 32-bit count per id")
        if d_entry_start is not None and (d_entry_start.numel() < n + 1 or d_entry_start.element_size() != 8
                                          or not d_entry_start.is_contiguous()):
            raise ValueError("d_entry_start must hold n + 1 64-bit entries")
        if d_n_entries.numel() < 1 or d_n_entries.element_size() != 8:
            raise ValueError("d_n_entries must hold one 64-bit word")
        ptr = (lambda t: None if t is None else t.data_ptr())
        self._check(self._lib.tbe_queue_export_ids_device(
            self.handle, d_ids.data_ptr(), n, d_qcount.data_ptr(), ptr(d_entry_start),
            ptr(d_entries) if capacity else None, capacity, d_n_entries.data_ptr(), 1 if clear else 0, stream))
        self._queue_in_flight = (d_ids,)   # read by the enqueued kernels

    def queue_export_ids(self, ids, clear: bool = False, capacity: Optional[int] = None):
        """The same with host arrays (tbe_queue_export_ids; synchronous): returns (qcount uint32
        [n], entry_start uint64 [n + 1], entries uint64 [min(total, capacity)], total).  capacity
        defaults to every entry (a counting call sizes the buffer)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        n = ids.shape[0]
        qcount = np.zeros(n, dtype=np.uint32)
        start = np.zeros(n + 1, dtype=np.uint64)
        total = ctypes.c_uint64()
        if capacity is None:
            self._check(self._lib.tbe_queue_export_ids(self.handle, ids.ctypes.data, n, qcount.ctypes.data,
                                                       start.ctypes.data, None, 0, byref(total), 0))
            capacity = total.value
        entries = np.zeros(capacity, dtype=np.uint64)
        self._check(self._lib.tbe_queue_export_ids(self.handle, ids.ctypes.data, n, qcount.ctypes.data,
                                                   start.ctypes.data, entries.ctypes.data if capacity else None,
                                                   capacity, byref(total), 1 if clear else 0))
        return qcount, start, entries[: min(total.value, capacity)], total.value

    def queue_import_ids_device(self, d_ids, d_qcount, d_entries, n_entries: Optional[int] = None,
                                stream: Optional[int] = None) -> None:
        """One tbe_queue_import_ids_device call: id i takes the next d_qcount[i] of d_entries
        (64-bit ``request_id << 16 | permits`` words; n_entries defaults to d_entries.numel()).
        Every id and entry is judged first; a void call writes nothing and raises at
        ``synchronize()``.  Set a moved key's class and row before its queue."""
        n = d_ids.numel()
        if n_entries is None:
            n_entries = 0 if d_entries is None else d_entries.numel()
        if not d_ids.is_contiguous() or d_ids.element_size() != 8:
            raise ValueError("d_ids must be a contiguous 64-bit tensor")
        if d_qcount.numel() != n or d_qcount.element_size() != 4 or not d_qcount.is_contiguous():
            raise ValueError("d_qcount must hold one 32-bit count per id")
        if n_entries and (d_entries is None or d_entries.numel() < n_entries or d_entries.element_size() != 8
                          or not d_entries.is_contiguous()):
            raise ValueError("n_entries exceeds d_entries")
        self._check(self._lib.tbe_queue_import_ids_device(
            self.handle, d_ids.data_ptr(), d_qcount.data_ptr(), n,
            d_entries.data_ptr() if n_entries else None, n_entries, stream))
        self._queue_in_flight = (d_ids, d_qcount, d_entries)   # read by the enqueued kernels

    def queue_import_ids(self, ids, qcount, entries) -> None:
        """The same from host arrays (tbe_queue_import_ids; synchronous): a void call raises and
        changes nothing."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        qcount = np.ascontiguousarray(qcount, dtype=np.uint32)
        entries = np.ascontiguousarray(entries, dtype=np.uint64)
        if ids.shape != qcount.shape:
            raise ValueError("ids and qcount must have the same length")
        self._check(self._lib.tbe_queue_import_ids(self.handle, ids.ctypes.data, qcount.ctypes.data, ids.shape[0],
                                                   entries.ctypes.data if entries.shape[0] else None,
                                                   entries.shape[0]))

    def queue_migrate_out_device(self, ts_us: int, d_key_of_id, d_owner_map, n_owners: int, self_rank: int, d_rows,
                                 d_counts, d_leaving=None, commit: bool = False, first: int = 0,
                                 capacity: Optional[int] = None, stream: Optional[int] = None, row_ids=None) -> None:
        """``migrate_out_device`` for a queueing engine (tbe_queue_migrate_out_ids_device): a
        leaving id sends a row when its bucket row is live or its queue is not empty, word 3 of
        a row is ``class | queue entries << 8``, and commit=True leaves the queue headers alone:
        ``queue_export_ids_device(row_ids, ..., clear=True)`` takes the queues, next and with
        nothing in between."""
        self._migrate_out_device(self._lib.tbe_queue_migrate_out_ids_device, ts_us, d_key_of_id, d_owner_map,
                                 n_owners, self_rank, d_rows, d_counts, d_leaving, commit, first, capacity, stream,
                                 row_ids)

    def queue_migrate_out(self, ts_us: int, key_of_id, owner_map, n_owners: int, self_rank: int,
                          commit: bool = False, first: int = 0, capacity: Optional[int] = None):
        """The same with host arrays (tbe_queue_migrate_out_ids; synchronous): returns (rows,
        counts, leaving, row_ids) as ``migrate_out(row_ids=True)`` does."""
        return self._migrate_out(self._lib.tbe_queue_migrate_out_ids, ts_us, key_of_id, owner_map, n_owners,
                                 self_rank, commit, first, capacity, True)


class ApproximateEngine(QueueingTokenBucketEngine):
    """ApproximateTokenBucket (ApproximateTokenBucket/RedisApproximateTokenBucketRateLimiter.cs, A):
    one client's local tier for every key plus a replica of the shared global tier.
    ``acquire_batch`` = AcquireCore / WaitAsyncCore (A:84-183); a refresh epoch =
    ``collect`` (A:430-435) -> exchange the counts between clients (RCCL all-gather, or
    all-reduce for one node-wide client) -> ``sync`` (A:439-508)."""

    KIND = _capi.TBE_KIND_APPROXIMATE

    def __init__(self, n_keys: int, token_limit: int, tokens_per_period: int, period_ticks: int,
                 queue_limit: int, queue_order: int = 0, zero_wait_slots: int = 4, approx_classes=None, **kw):
        """zero_wait_slots: queue entries per key for zero-permit waits (tbe.h).
        approx_classes: extra limit classes 1.. as (token_limit, tokens_per_period,
        period_ticks, queue_limit, order) (tbe_create_approx_classes; class 0 is this
        engine's own five options, zero_wait_slots is shared).  Keys move between classes
        with ``set_class``; ``collect``, ``sync`` and ``refresh`` take ``classes=`` to sync
        each class at its own ReplenishmentPeriod (A:443)."""
        super().__init__(n_keys, token_limit, tokens_per_period, period_ticks, queue_limit,
                         queue_order, zero_wait_slots=zero_wait_slots, approx_classes=approx_classes, **kw)
        self.zero_wait_slots = zero_wait_slots

    def approx_classes(self):
        """Every class's (token_limit, tokens_per_period, period_ticks, queue_limit, order),
        class 0 first (tbe_approx_classes)."""
        n = c_uint32()
        self._check(self._lib.tbe_approx_classes(self.handle, None, 0, byref(n)))
        out = (_capi.TbeQueueClass * n.value)()
        self._check(self._lib.tbe_approx_classes(self.handle, out, n.value, byref(n)))
        return [(c.token_limit, c.tokens_per_period, c.replenishment_period_ticks, c.queue_limit, c.queue_order)
                for c in out]

    def _five_option_classes(self):   # (the base class sizes queue_of's buffer from the longest ring)
        return self.approx_classes()

    def acquire_batch(self, keys, permits, wait: bool = True, id_base: int = 0, status=None, available=None,
                      retry_after=False):
        """Returns (status u8, available i32, evicted (cause index, request id)).

        retry_after: True, or an int64 array to fill: the failed leases' RetryAfter in .NET
        ticks (tbe_approx_acquire_batch_retry; TBE_RETRY_NONE where the status is not
        FAILED), returned as a fourth element."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        permits = np.ascontiguousarray(permits, dtype=np.int32)
        n = keys.shape[0]
        status = np.empty(n, dtype=np.uint8) if status is None else status
        avail = np.empty(n, dtype=np.int32) if available is None else available
        n_ev = ctypes.c_uint64()
        want_retry = retry_after is not False and retry_after is not None
        if want_retry:
            ticks = np.empty(n, dtype=np.int64) if retry_after is True else retry_after
            self._check(self._lib.tbe_approx_acquire_batch_retry(
                self.handle, keys.ctypes.data, permits.ctypes.data, n, 1 if wait else 0, id_base,
                status.ctypes.data, avail.ctypes.data, ticks.ctypes.data, byref(n_ev)))
        else:
            self._check(self._lib.tbe_approx_acquire_batch(self.handle, keys.ctypes.data, permits.ctypes.data,
                                                           n, 1 if wait else 0, id_base, status.ctypes.data,
                                                           avail.ctypes.data, byref(n_ev)))
        m = n_ev.value
        cause = np.empty(m, dtype=np.uint64)
        ids = np.empty(m, dtype=np.int64)
        nw = ctypes.c_uint64()
        if m:
            self._check(self._lib.tbe_evicted(self.handle, cause.ctypes.data, ids.ctypes.data, m, byref(nw)))
        if want_retry:
            return status, avail, (cause, ids), ticks
        return status, avail, (cause, ids)

    def acquire_batch_device(self, d_keys, d_permits, d_status, d_available, wait: bool = False,
                             id_base: int = 0, stream: Optional[int] = None, d_retry_after=None) -> None:
        """Device tensors in and out; enqueued (tbe_approx_acquire_batch_device, or
        tbe_approx_acquire_batch_retry_device with the int64 tensor `d_retry_after`)."""
        n = d_keys.numel()
        if d_retry_after is not None:
            self._check(self._lib.tbe_approx_acquire_batch_retry_device(
                self.handle, d_keys.data_ptr(), d_permits.data_ptr(), n, 1 if wait else 0, id_base,
                d_status.data_ptr(), d_available.data_ptr(), d_retry_after.data_ptr(), stream))
            return
        self._check(self._lib.tbe_approx_acquire_batch_device(
            self.handle, d_keys.data_ptr(), d_permits.data_ptr(), n, 1 if wait else 0, id_base,
            d_status.data_ptr(), d_available.data_ptr(), stream))

    def collect(self, d_counts, classes=None) -> None:
        """Local scores of every key into the int32 device tensor `d_counts` [n_keys].
        classes: an iterable of class numbers; keys of other classes give 0 and keep their
        count (tbe_approx_collect_classes)."""
        if classes is not None:
            self._check(self._lib.tbe_approx_collect_classes(self.handle, d_counts.data_ptr(),
                                                             _capi.class_mask(classes), None))
            return
        self._check(self._lib.tbe_approx_collect(self.handle, d_counts.data_ptr(), None))

    def sync(self, d_all_counts, n_clients: int, my_client: int, ts_us: int, stagger_us: int,
             stream: Optional[int] = None, classes=None):
        """Replay the epoch's sync calls; returns the drain log (keys, request ids, available).
        stream=None: d_all_counts must be complete at the call (tbe_approx_sync); a stream
        handle: the replay is ordered after the work enqueued on that stream so far
        (tbe_approx_sync_stream), e.g. the collective or copy that produced the counts.
        classes: an iterable of class numbers; keys of other classes are left untouched
        (tbe_approx_sync_classes(_stream))."""
        n = ctypes.c_uint64()
        if classes is not None:
            mask = _capi.class_mask(classes)
            if stream is None:
                self._check(self._lib.tbe_approx_sync_classes(self.handle, d_all_counts.data_ptr(), n_clients,
                                                              my_client, ts_us, stagger_us, mask, byref(n)))
            else:
                self._check(self._lib.tbe_approx_sync_classes_stream(self.handle, d_all_counts.data_ptr(), n_clients,
                                                                     my_client, ts_us, stagger_us, mask, stream,
                                                                     byref(n)))
            return self._drain_log(n.value)
        if stream is None:
            self._check(self._lib.tbe_approx_sync(self.handle, d_all_counts.data_ptr(), n_clients, my_client,
                                                  ts_us, stagger_us, byref(n)))
        else:
            self._check(self._lib.tbe_approx_sync_stream(self.handle, d_all_counts.data_ptr(), n_clients,
                                                         my_client, ts_us, stagger_us, stream, byref(n)))
        return self._drain_log(n.value)

    def refresh(self, ts_us: int, classes=None):
        """RefreshAsync as the only client of the global tier (A:412-508); classes: an
        iterable of class numbers to refresh alone (tbe_approx_refresh_classes)."""
        n = ctypes.c_uint64()
        if classes is not None:
            self._check(self._lib.tbe_approx_refresh_classes(self.handle, ts_us, _capi.class_mask(classes), byref(n)))
            return self._drain_log(n.value)
        self._check(self._lib.tbe_approx_refresh(self.handle, ts_us, byref(n)))
        return self._drain_log(n.value)

    def _drain_log(self, m: int):
        keys = np.empty(m, dtype=np.uint64)
        ids = np.empty(m, dtype=np.int64)
        rem = np.empty(m, dtype=np.int32)
        nw = ctypes.c_uint64()
        if m:
            self._check(self._lib.tbe_refresh_log(self.handle, keys.ctypes.data, ids.ctypes.data,
                                                  rem.ctypes.data, m, byref(nw)))
        return keys, ids, rem

    def export_global(self, first: int = 0, count: Optional[int] = None):
        """Replica of the global tier (tbe_approx_export_state): (v, p, t_us), t_us =
        INT64_MIN for absent keys."""
        if count is None:
            count = self.n_keys - first
        v = np.empty(count, dtype=np.float64)
        p = np.empty(count, dtype=np.float64)
        t = np.empty(count, dtype=np.int64)
        self._check(self._lib.tbe_approx_export_state(self.handle, first, count, v.ctypes.data,
                                                      p.ctypes.data, t.ctypes.data))
        return v, p, t

    def import_global(self, v, p, t_us, first: int = 0) -> None:
        """Restore rows of the global-tier replica (tbe_approx_import_state)."""
        v = np.ascontiguousarray(v, dtype=np.float64)
        p = np.ascontiguousarray(p, dtype=np.float64)
        t_us = np.ascontiguousarray(t_us, dtype=np.int64)
        if not (v.shape == p.shape == t_us.shape):
            raise ValueError("v, p and t_us must have the same length")
        self._check(self._lib.tbe_approx_import_state(self.handle, first, v.shape[0], v.ctypes.data,
                                                      p.ctypes.data, t_us.ctypes.data))

    # ------------------------------------------------------------------ idle keys, snapshots
    def idle_device(self, ts_us: int, d_idle, first: int = 0, stream: Optional[int] = None) -> None:
        """d_idle (uint8 device tensor): d_idle[k - first] = 1 for every key of [first, first +
        len) that is idle at ts_us -- nothing queued, ConsumedTokens == 0 and a tier row worth
        no tokens (tbe_approx_idle_device; ``snapshot.approx_idle_rows`` states the rule).
        Enqueued, not synchronised; stream as in ``acquire_batch_device``."""
        self._check(self._lib.tbe_approx_idle_device(self.handle, ts_us, first, d_idle.numel(), d_idle.data_ptr(),
                                                     stream))

    def reset_device(self, d_flags, first: int = 0, stream: Optional[int] = None) -> None:
        """Every key k of [first, first + len) with d_flags[k - first] != 0 (uint8 device
        tensor) gets the state of a new engine (tbe_approx_reset_device).  Enqueued."""
        self._check(self._lib.tbe_approx_reset_device(self.handle, first, d_flags.numel(), d_flags.data_ptr(),
                                                      stream))

    def export_live_device(self, ts_us: int, d_ids, d_v, d_t_us, d_n_live, first: int = 0,
                           count: Optional[int] = None, capacity: Optional[int] = None,
                           stream: Optional[int] = None, d_p=None, d_skip=None, tier: bool = False) -> None:
        """One tbe_approx_export_live_device call: the {v, p, t} tier rows that are present and
        not lapsed at ts_us, minus those with a non-zero byte in d_skip (uint8, one per key of
        the range), into int64 ids, float64 v and p, int64 t_us and a one-element int64 count.
        Selected by d_p (or, for a counting call without buffers, tier=True); without either
        this is the token-bucket entry point, which refuses an approximate engine (tbe.h)."""
        if d_p is None and d_skip is None and not tier:
            return super().export_live_device(ts_us, d_ids, d_v, d_t_us, d_n_live, first, count, capacity, stream)
        if count is None:
            count = self.n_keys - first
        if capacity is None:
            capacity = 0 if d_ids is None else d_ids.numel()
        if capacity and min(d_ids.numel(), d_v.numel(), d_p.numel(), d_t_us.numel()) < capacity:
            raise ValueError("capacity exceeds the output tensors")
        if d_skip is not None and (d_skip.numel() != count or d_skip.element_size() != 1):
            raise ValueError("d_skip must hold one byte per key of the range")
        ptr = (lambda t: None if t is None else t.data_ptr())
        self._check(self._lib.tbe_approx_export_live_device(self.handle, ts_us, first, count, ptr(d_skip), ptr(d_ids),
                                                            ptr(d_v), ptr(d_p), ptr(d_t_us), capacity,
                                                            d_n_live.data_ptr(), stream))

    def export_live(self, ts_us: int, first: int = 0, count: Optional[int] = None, stream: Optional[int] = None,
                    d_skip=None):
        """The exported tier rows of [first, first + count) as (ids int64, v, p float64, t_us
        int64) device tensors, ascending ids: a counting call, one read-back of the count,
        then the filling call (as ``TokenBucketEngine.export_live``)."""
        import torch
        if count is None:
            count = self.n_keys - first
        dev = torch.device("cuda", self.config.device if self.config.device >= 0 else torch.cuda.current_device())
        d_n = torch.zeros(1, dtype=torch.int64, device=dev)
        self.export_live_device(ts_us, None, None, None, d_n, first, count, 0, stream, d_skip=d_skip, tier=True)
        torch.cuda.synchronize(dev)
        n = int(d_n.item())
        d_ids = torch.empty(n, dtype=torch.int64, device=dev)
        d_v = torch.empty(n, dtype=torch.float64, device=dev)
        d_p = torch.empty(n, dtype=torch.float64, device=dev)
        d_t = torch.empty(n, dtype=torch.int64, device=dev)
        if n:
            self.export_live_device(ts_us, d_ids, d_v, d_t, d_n, first, count, n, stream, d_p=d_p, d_skip=d_skip)
            if not stream:
                torch.cuda.synchronize(dev)
        return d_ids, d_v, d_p, d_t

    def import_rows(self, d_ids, d_v, d_t_us, stream: Optional[int] = None, d_p=None) -> None:
        """tier[d_ids[i]] = {d_v[i], d_p[i], d_t_us[i]} from device tensors
        (tbe_approx_import_rows_device); enqueued, an invalid row voids the call and raises at
        ``synchronize()``.  Without d_p this is the token-bucket entry point, which refuses an
        approximate engine (tbe.h)."""
        if d_p is None:
            return super().import_rows(d_ids, d_v, d_t_us, stream)
        n = d_ids.numel()
        if d_v.numel() != n or d_p.numel() != n or d_t_us.numel() != n:
            raise ValueError("d_ids, d_v, d_p and d_t_us must have the same length")
        d_ids, d_v, d_p, d_t_us = d_ids.contiguous(), d_v.contiguous(), d_p.contiguous(), d_t_us.contiguous()
        self._check(self._lib.tbe_approx_import_rows_device(self.handle, d_ids.data_ptr(), d_v.data_ptr(),
                                                            d_p.data_ptr(), d_t_us.data_ptr(), n, stream))
        self._rows_in_flight = (d_ids, d_v, d_p, d_t_us)   # read by the enqueued kernels

    def local_state(self, key: int):
        """(local, global, est, available, queued) of one key."""
        lo, gl, av = c_int32(), c_int32(), c_int32()
        est = c_double()
        q = c_uint32()
        self._check(self._lib.tbe_approx_query(self.handle, key, byref(lo), byref(gl), byref(est),
                                               byref(av), byref(q)))
        return lo.value, gl.value, est.value, av.value, q.value
