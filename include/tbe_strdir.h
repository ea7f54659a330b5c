/*
 * tbe_strdir.h -- device-resident string-key directory, C ABI.
 *
 * The reference's bucket key is the exact string InstanceName + resourceID
 * (PartitionedRedisTokenBucketRateLimiter.cs:42, `BucketId = InstanceName + resourceID`);
 * Redis keys are compared byte for byte, so two resource ids never share a bucket.  This
 * directory maps such strings to the engine's dense key ids in HBM, batch at a time:
 *
 *   - a directory belongs to one limiter and holds its InstanceName as `prefix`; the
 *     strings passed per request are the resourceIDs (the key is prefix + resourceID);
 *   - strings are compared byte for byte (a 64-bit hash only chooses the slot: at 1e8
 *     keys two of them share a hash with probability ~2.7e-4), so the
 *     mapping is collision-free;
 *   - ids are assigned exactly like tbe_dir_* (tbe_cluster.h): strings new to the
 *     directory get consecutive counters in order of first occurrence (batches in call
 *     order, arrival order inside a batch) and id = a fixed bijection of [0, capacity)
 *     applied to the counter.  An id depends only on that order, never on hashes.
 *   - keys whose bucket no longer exists in the store are removed by a reclaim (below),
 *     the counterpart of Redis dropping a key at its EXPIRE (TB:232-235).  The directory
 *     holds a stack of freed ids and a `fresh` counter: a reclaim pushes the ids it
 *     removes in ascending order; a batch's new strings, in order of first occurrence,
 *     each pop the stack, and once it is empty take bijection(fresh++).  Ids stay a pure
 *     function of the call sequence (assigns and reclaims).  A directory that is never
 *     reclaimed assigns the ids described above.
 *
 * Batch layout (Arrow-style string array): string i is bytes [offs[i], offs[i+1]) of
 * `bytes`; offs has n + 1 u64 entries, non-decreasing, offs[n] <= n_bytes; a string is
 * at most 65536 bytes; `bytes` is 8-byte aligned.  A request whose offsets break these
 * rules gets id UINT64_MAX and the directory's error state (tbe_sdir_size: TBE_EINVAL).
 *
 * Limits: `capacity` keys and `arena_bytes` bytes of key text held at one time (each key
 * takes its length rounded up to 8).  Both bound the keys the directory holds, not the
 * keys it has ever seen: a caller whose key space churns (client addresses, sessions,
 * API tokens) calls tbe_sdir_reclaim from a timer, well before either limit is reached,
 * and the ids and text bytes of the buckets that have expired are used again.  Room for
 * new keys is (freed ids) + capacity - fresh.  A batch that brings more new keys than
 * either limit leaves the directory in the sticky TBE_ERANGE state: keys that got an id
 * keep it, unique; the others get UINT64_MAX (an engine batch containing them is
 * rejected).  That state is not undone by a reclaim: the directory must be recreated.
 *
 * All device calls enqueue on `stream` (hipStream_t; NULL = the default stream).
 */
#ifndef TBE_STRDIR_H_
#define TBE_STRDIR_H_

#include <stdint.h>

#include "tbe.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tbe_string_directory tbe_string_directory;

/* prefix: InstanceName (prefix_len bytes, may be 0). */
tbe_status tbe_sdir_create(uint64_t capacity, uint64_t arena_bytes, const char *prefix, uint32_t prefix_len,
                           int32_t device, tbe_string_directory **out);
void tbe_sdir_destroy(tbe_string_directory *dir);

/* d_ids[i] = id of string i (assigning new ones).  n < 2^32. */
tbe_status tbe_sdir_assign_device(tbe_string_directory *dir, const uint8_t *d_bytes, uint64_t n_bytes,
                                  const uint64_t *d_offs, uint64_t n, uint64_t *d_ids, void *stream);
/* d_ids[i] = id of string i, UINT64_MAX for a string never assigned (nothing changes). */
tbe_status tbe_sdir_lookup_device(tbe_string_directory *dir, const uint8_t *d_bytes, uint64_t n_bytes,
                                  const uint64_t *d_offs, uint64_t n, uint64_t *d_ids, void *stream);
/* Host buffers (staged through the directory's device; synchronises before returning). */
tbe_status tbe_sdir_assign(tbe_string_directory *dir, const uint8_t *bytes, uint64_t n_bytes,
                           const uint64_t *offs, uint64_t n, uint64_t *ids);

/* Keys held: ids assigned and not reclaimed since (synchronises).  TBE_ERANGE after a
 * capacity or arena overflow (or a string whose hashes collided in all four probe
 * rounds: never observed with 64-bit hashes), TBE_EINVAL after a malformed batch. */
tbe_status tbe_sdir_size(tbe_string_directory *dir, uint64_t *n_ids);

/* Key text of an id (resourceID part, without the prefix): *len = its length; copies
 * min(len, cap) bytes to buf.  TBE_EINVAL for an id never assigned.  Synchronises. */
tbe_status tbe_sdir_key_of(tbe_string_directory *dir, uint64_t id, uint8_t *buf, uint64_t cap, uint64_t *len);

/* Key text of many ids, on the device (bulk tbe_sdir_key_of; mirrors tbe_key_text_lengths_device
 * / tbe_key_text_device of tbe_tools.h).  First call: d_lens[i] = length of the resourceID
 * (without the prefix) held by id d_ids[i]; an id that is not held (never assigned,
 * reclaimed, or >= capacity) gets 0 and is counted in *d_n_missing (device u64, may be
 * NULL).  The caller scans the lengths into n + 1 offsets; the second call copies the text
 * of id d_ids[i] to d_bytes[d_offs[i], d_offs[i+1]), which must hold d_offs[n] bytes.  The
 * result is the batch layout tbe_sdir_assign_device takes.  Contract as for a lookup: no
 * assign or reclaim may be in flight on another stream, nor run between the two calls. */
tbe_status tbe_sdir_text_lengths_device(tbe_string_directory *dir, const uint64_t *d_ids, uint64_t n,
                                        uint64_t *d_lens, uint64_t *d_n_missing, void *stream);
tbe_status tbe_sdir_text_device(tbe_string_directory *dir, const uint64_t *d_ids, uint64_t n,
                                const uint64_t *d_offs, uint8_t *d_bytes, void *stream);

/* Routing keys of the held ids, on the device: what a live owner-map change of text-keyed
 * buckets hands to tbe_migrate_out_device as its key-of-id table (tbe_cluster.h "Migrating
 * text-keyed buckets").  d_keys[i] = tbe_text_route_key(text, len, seed) of the resourceID
 * (without the prefix) that id first + i holds -- the key tbe_route_text_keys_device computes
 * for the same text on the sending side, bit for bit --, and UINT64_MAX for an id that is not
 * held (never assigned, or reclaimed).  *d_n_held (device u64, may be NULL) = held ids of the
 * range.  The text is read out of the arena in place.  A range past capacity or a NULL
 * d_keys: TBE_EINVAL, nothing enqueued.  Contract as for a lookup: no assign or reclaim in
 * flight on another stream.
 * A held string whose routing key is itself UINT64_MAX (probability 2^-64 per key) reads as
 * unheld.  The value is not remapped, because the senders route that string by the same
 * unmapped key; if the id's row is live, the migration's pre-flight counts it as an orphan
 * and refuses the change, so nothing is lost. */
tbe_status tbe_sdir_route_keys_device(tbe_string_directory *dir, uint64_t seed, uint64_t first, uint64_t count,
                                      uint64_t *d_keys, uint64_t *d_n_held, void *stream);

/* out = {keys held (what tbe_sdir_size reports), arena bytes in use (every held key's length
 * rounded up to 8), arena_bytes}.  Synchronises; statuses as tbe_sdir_size (out is filled for
 * TBE_ERANGE and TBE_EINVAL too).  The room check of a migration reads it, so that no
 * incoming key can push the arena into the sticky TBE_ERANGE state. */
tbe_status tbe_sdir_usage(tbe_string_directory *dir, uint64_t out[3]);

/* Remove the keys flagged dead and reuse what they held.  d_dead: `capacity` bytes of
 * device memory indexed by id (tbe_expired_device over [0, capacity) writes them);
 * d_keep_ids: n_keep ids (device memory) that are never removed.  For every id that is
 * assigned, flagged and not kept: its string leaves the directory (lookup: UINT64_MAX;
 * tbe_sdir_key_of: TBE_EINVAL until the id is assigned again), the id goes onto the free
 * stack (ascending id order within one reclaim) and its text bytes are given back.
 * Every other key keeps its id and text.  *d_n_reclaimed (device memory, may be NULL)
 * gets the number of keys removed.  Enqueued on `stream`, nothing is synchronised.
 *
 * Contract: the reclaim rebuilds the slot table and compacts the arena, so
 *   - no assign or lookup may be in flight on another stream (work enqueued on `stream`
 *     before and after the call is ordered as usual);
 *   - d_dead must describe the engine after every batch that used this directory's ids;
 *     an id handed out by an assign whose engine batch has not been submitted yet has
 *     an absent row and would be flagged: such ids go in d_keep_ids.
 * Cost: one pass over the ids and the slots plus a copy of the live keys' text, O(live
 * keys + live text): a maintenance call made every few seconds to minutes.  The first
 * reclaim allocates its working memory, kept until tbe_sdir_destroy: a second arena
 * (arena_bytes) and 29 bytes per id of capacity (flags, free stack, survivor records). */
tbe_status tbe_sdir_reclaim_device(tbe_string_directory *dir, const uint8_t *d_dead,
                                   const uint64_t *d_keep_ids, uint64_t n_keep,
                                   uint64_t *d_n_reclaimed, void *stream);

/* The periodic call of a host: tbe_expired_device(engine, ts_us, 0, capacity, clear = 1)
 * followed by tbe_sdir_reclaim_device, ordered after everything enqueued before it on
 * any stream; synchronous.  The engine (token-bucket or queueing kind, on the
 * directory's device) must have n_keys >= capacity.  The lapsed rows are written back
 * absent, so a reused id starts from a full bucket whatever timestamp comes next.
 * keep_ids is a host array (may be NULL when n_keep is 0); *n_reclaimed = keys removed.
 * One more byte per id of capacity is held for the flags.
 * On an engine with limit classes (tbe_create_classes) each key lapses by its own class's
 * TTL, and a reclaimed id keeps the class byte of the key that held it: the caller sets the
 * class of the new key (tbe_set_class) before that key's first batch. */
tbe_status tbe_sdir_reclaim(tbe_string_directory *dir, tbe_engine *engine, int64_t ts_us,
                            const uint64_t *keep_ids, uint64_t n_keep, uint64_t *n_reclaimed);

/* Assign path: 0 = automatic (default), 1 = full pass, 2 = warm path.  The warm path first
 * resolves every string of the batch that is already known (one lookup pass: hash,
 * probe, byte compare with the stored text) and runs the assign passes over the misses
 * only, listed in arrival order; automatic takes it while the last batch whose id count
 * has come back brought new keys (fresh or reused ids alike) for less than half of its
 * requests.  Ids, errors and the directory's state are the same on either path. */
tbe_status tbe_sdir_set_mode(tbe_string_directory *dir, int32_t mode);

/* Test hook: keep only the low `bits` (1..62) bits of every string hash, so that distinct
 * strings share hashes often and the byte comparison and re-probe rounds run.  Ids do not
 * change (they depend only on first occurrence).  Only before the first assign. */
tbe_status tbe_sdir_set_hash_bits(tbe_string_directory *dir, uint32_t bits);

#ifdef __cplusplus
}
#endif

#endif /* TBE_STRDIR_H_ */
