/*
 * tbe_cluster.h -- multi-GPU data path of the engine, C ABI.
 *
 * The reference distributes by letting every client process share ONE Redis key space
 * (README:1-9; the bucket key is InstanceName + resourceID, PTB:42).  Here each GPU
 * owns a hash partition of the keys and holds their buckets in its own HBM:
 *
 *   owner(key) = ((mix64(key) >> 32) * n_owners) >> 32
 *              = mix64(key) >> (64 - log2 n_owners)      for a power-of-two n_owners
 *
 * Requests that arrive at the wrong GPU are routed with one all-to-all (RCCL over xGMI,
 * driven by the host through torch.distributed): tbe_route_plan_device groups a batch by
 * owner, stably (arrival order kept inside each owner's group), tbe_route_pack_device
 * lays the groups out as the all-to-all's send buffer, and after the owners decide,
 * tbe_route_gather_device puts the replies back in arrival order.  On the owner, a
 * device-resident key directory (tbe_dir_*) turns the owned global keys into dense local
 * bucket ids, collision-free (it compares whole keys).  Everything stays in HBM; only the
 * n_owners group sizes cross to the host (the all-to-all's split sizes).  A batch keyed by
 * text instead of u64 keys is routed by a hash of the text and carries its bytes to the owner,
 * whose string directory (tbe_strdir.h) resolves them ("routing text" below).
 *
 * All calls enqueue on `stream` (hipStream_t, NULL = the default stream) and return
 * TBE_OK, or TBE_EINVAL for bad arguments (nothing enqueued).
 */
#ifndef TBE_CLUSTER_H_
#define TBE_CLUSTER_H_

#include <stdint.h>

#include "tbe.h"

#ifdef __cplusplus
extern "C" {
#endif

/* owner(key) as above, on the host (the device kernels use the same function). */
uint32_t tbe_key_owner(uint64_t key, uint32_t n_owners);

/* Stable partition of a batch by owner, 1 <= n_owners <= 256, n < 2^32:
 * d_counts[o] (u64) = requests of owner o; d_pos[i] = position of request i in the
 * owner-grouped order (owner-major, arrival order inside an owner).  Uses a workspace
 * of tbe_route_workspace_bytes(n, n_owners) bytes at d_work. */
uint64_t tbe_route_workspace_bytes(uint64_t n, uint32_t n_owners);
tbe_status tbe_route_plan_device(const uint64_t *d_keys, uint64_t n, uint32_t n_owners, void *d_work,
                                 uint32_t *d_pos, uint64_t *d_counts, void *stream);

/* ---------------------------------------------------------------- owner maps
 * Table-driven ownership (DESIGN.md §7 "owner maps"): owner(key) = map[vnode(key)], with
 * vnode(key) = mix64(key) >> 52, one of TBE_OWNER_MAP_SIZE virtual nodes, and `map` a u8
 * array of TBE_OWNER_MAP_SIZE owners (4-byte aligned), the same on every GPU.  The map
 * v -> (v * n_owners) >> 12 is the hash partition above for a power-of-two n_owners; a
 * balanced map gives the virtual nodes of hot keys' owners fewer others, so a Zipf
 * stream's owner loads even out (SURVEY.md §7 hard part iii).  A key still has exactly
 * one owner.  Owners hold their buckets by dense id, so a map changes between batches by
 * migrating the buckets it reassigns (DESIGN.md §7 "Migrating buckets"): every owner packs
 * the live rows of the keys the new map gives away (tbe_dir_keys_of_device over its ids,
 * then tbe_migrate_out_device with commit), drops those keys (tbe_dir_reclaim_device with
 * the leaving flags), the rows cross in one all-to-all, and each new owner installs them
 * behind its own directory (tbe_dir_assign_device, tbe_set_class_device,
 * tbe_import_rows_device); the tables stay in HBM.  Buckets keyed by text migrate the same
 * way (DESIGN.md §7 "Migrating text-keyed buckets"): the key-of-id table is
 * tbe_sdir_route_keys_device's, tbe_migrate_out_ids_device also gives the packed rows' ids,
 * whose text tbe_sdir_text_lengths_device / tbe_sdir_text_device fetch before
 * tbe_sdir_reclaim_device forgets it, and the text crosses in an all-to-all of its own to the
 * new owner's tbe_sdir_assign_device.  The number of owners still changes
 * through a snapshot: every owner saves its live buckets by key (tbe_export_live_device,
 * tbe_dir_keys_of_device) and each new owner loads the keys the new map gives it
 * (DESIGN.md §8 "Portable snapshots"). */
#define TBE_OWNER_MAP_BITS 12
#define TBE_OWNER_MAP_SIZE 4096
uint32_t tbe_key_vnode(uint64_t key);
/* tbe_route_plan_device with owner = d_owner_map[vnode(key)] (d_owner_map NULL: the hash
 * partition, exactly tbe_route_plan_device); every map entry must be < n_owners. */
tbe_status tbe_route_plan_map_device(const uint64_t *d_keys, uint64_t n, uint32_t n_owners,
                                     const uint8_t *d_owner_map, void *d_work, uint32_t *d_pos,
                                     uint64_t *d_counts, void *stream);
/* d_counts[v] (u64, TBE_OWNER_MAP_SIZE of them, zeroed first) = requests of the batch on
 * virtual node v: the load histogram a balanced map is built from. */
tbe_status tbe_vnode_count_device(const uint64_t *d_keys, uint64_t n, uint64_t *d_counts, void *stream);

/* Send buffer of the routing all-to-all: out[pos[i]] = {key, ts_us, permits} as three
 * int64 per request (d_out holds 3n). */
tbe_status tbe_route_pack_device(const uint32_t *d_pos, uint64_t n, const uint64_t *d_keys,
                                 const int32_t *d_permits, const int64_t *d_ts_us, int64_t *d_out,
                                 void *stream);

/* Replies back to arrival order: out[i*cols + c] = in[pos[i]*cols + c], 1 <= cols <= 8. */
tbe_status tbe_route_gather_device(const uint32_t *d_pos, uint64_t n, const int64_t *d_in, uint32_t cols,
                                   int64_t *d_out, void *stream);

/* ---------------------------------------------------------------- routing text
 * The reference's bucket key is a string (InstanceName + resourceID, PTB:42), and a batch
 * keyed by text is an Arrow-style string array as tbe_sdir_assign_device takes it
 * (tbe_strdir.h): d_bytes (8-byte aligned), d_offs[n + 1], n_bytes.  Its strings are routed
 * by a 64-bit routing key
 *
 *   text_route_key(text, seed) = H(text, seed):  h = mix64(seed ^ len * 0x9E3779B97F4A7C15),
 *   then h = mix64(h ^ w_k) over the little-endian 8-byte words w_k of the text, the last
 *   one zero-padded
 *
 * (the hash the string directory tags its slots with), and owner(text) is the owner of that
 * u64 exactly as above: tbe_key_owner, or d_owner_map[tbe_key_vnode(.)], so owner maps,
 * tbe_vnode_count_device and a balanced map serve text unchanged.  `seed` lets each limiter
 * (InstanceName) spread its names on its own.  Two strings with one routing key merely
 * share an owner: each string travels with its text, and the owner's string directory
 * compares bytes.  Sender, per batch: tbe_route_text_keys_device, tbe_route_plan_map_device
 * over the keys, tbe_route_text_offsets_device, tbe_route_text_pack_device; the per-owner row
 * and byte counts are the split sizes of the two all-to-alls (rows, bytes).  Receiver:
 * tbe_route_text_recv_offsets_device, then tbe_sdir_assign_device over the received bytes.
 * The replies return through tbe_route_gather_device as for u64 keys.
 *
 * A string whose offsets are malformed by tbe_strdir.h's rules (end < start, end > n_bytes,
 * longer than 65536 bytes) is counted and treated as the empty string by every step; no
 * step reads outside [0, n_bytes) whatever the offsets say.  n < 2^32; byte totals are u64;
 * n == 0 is valid. */
uint64_t tbe_text_route_key(const uint8_t *text, uint64_t len, uint64_t seed);

/* d_keys[i] = routing key of string i; *d_n_bad (u64, device memory) = malformed strings. */
tbe_status tbe_route_text_keys_device(const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *d_offs,
                                      uint64_t n, uint64_t seed, uint64_t *d_keys, uint64_t *d_n_bad,
                                      void *stream);

/* The send offsets: d_send_offs[j] (u64, n + 1 of them) = bytes in front of the string at
 * position j of the owner-grouped order (d_pos and d_counts: tbe_route_plan_map_device's),
 * d_send_offs[n] = all bytes; d_byte_counts[o] (u64) = bytes of owner o's group.  d_work:
 * tbe_route_text_workspace_bytes(n) bytes, 8-byte aligned. */
uint64_t tbe_route_text_workspace_bytes(uint64_t n);
tbe_status tbe_route_text_offsets_device(const uint64_t *d_offs, uint64_t n_bytes, uint64_t n,
                                         const uint32_t *d_pos, const uint64_t *d_counts, uint32_t n_owners,
                                         void *d_work, uint64_t *d_send_offs, uint64_t *d_byte_counts,
                                         void *stream);

/* Send buffers of the two all-to-alls: the text of string i at d_out_bytes[d_send_offs[pos[i]]
 * ..), tightly packed (an owner's segment is the concatenation of its strings in arrival
 * order), and d_out_rows[pos[i]] = {len, ts_us, permits} as three int64 (d_out_rows holds
 * 3n): tbe_route_pack_device's record with the length in the key's place.  d_out_bytes is
 * 8-byte aligned and holds out_capacity bytes; bytes outside [0, d_send_offs[n]) are left
 * alone, and a string that would pass out_capacity is left out (only a malformed batch,
 * whose spans may overlap, can need more than n_bytes). */
tbe_status tbe_route_text_pack_device(const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *d_offs,
                                      uint64_t n, const uint32_t *d_pos, const uint64_t *d_send_offs,
                                      const int32_t *d_permits, const int64_t *d_ts_us, uint8_t *d_out_bytes,
                                      uint64_t out_capacity, int64_t *d_out_rows, void *stream);

/* The receiver's offsets: d_offs[m + 1] = exclusive scan of column 0 of the m received
 * rows (a length outside 0..65536 counts as 65536).  d_work as above, for m. */
tbe_status tbe_route_text_recv_offsets_device(const int64_t *d_rows, uint64_t m, void *d_work, uint64_t *d_offs,
                                              void *stream);

/* ---------------------------------------------------------------- key directory
 * Global key (any u64 but UINT64_MAX) -> dense local id in [0, capacity), assigned when a
 * key is first seen: keys new to the directory get consecutive counters in order of
 * first occurrence (batches in call order, arrival order inside a batch), and the id is
 * a fixed bijection of [0, capacity) applied to the counter (so hot keys, which are seen
 * first, do not crowd the first buckets).  Collision-free: the table stores whole keys.
 * Keys whose bucket no longer exists in the store are removed by a reclaim (below), the
 * counterpart of Redis dropping a key at its EXPIRE (TB:232-235), by the rule of the string
 * directory (tbe_strdir.h): the directory holds a stack of freed ids and a `fresh` counter;
 * a reclaim pushes the ids it removes in ascending order; a batch's new keys, in order of
 * first occurrence, each pop the stack, and once it is empty take bijection(fresh++).  Ids
 * stay a pure function of the call sequence (assigns and reclaims), and a directory that
 * is never reclaimed assigns the ids described above.
 * Capacity: `capacity` bounds the keys the directory holds at one time, not the keys it has
 * ever seen.  A caller whose key space churns (client addresses, sessions, API tokens)
 * calls tbe_dir_reclaim from a timer, well before the limit is reached, and the ids of the
 * buckets that have expired are used again.  Room for new keys is (freed ids) + capacity -
 * fresh.  A batch that brings more new keys than that leaves the directory in the sticky
 * TBE_ERANGE state (tbe_dir_size reports it from then on): every key that gets an id keeps
 * a unique one in [0, capacity), but which of the new keys get one is unspecified (the
 * hash table, 2x capacity, may fill up first); the others get UINT64_MAX, and an engine
 * batch containing them is rejected as invalid.  That state is not undone by a reclaim. */
typedef struct tbe_directory tbe_directory;

tbe_status tbe_dir_create(uint64_t capacity, int32_t device, tbe_directory **out);
void tbe_dir_destroy(tbe_directory *dir);
/* d_ids[i] = id of d_keys[i] (assigning new ones).  n < 2^32. */
tbe_status tbe_dir_assign_device(tbe_directory *dir, const uint64_t *d_keys, uint64_t n, uint64_t *d_ids,
                                 void *stream);
/* d_ids[i] = id of d_keys[i], UINT64_MAX for a key never assigned (nothing changes). */
tbe_status tbe_dir_lookup_device(tbe_directory *dir, const uint64_t *d_keys, uint64_t n, uint64_t *d_ids,
                                 void *stream);
/* Reverse lookup: d_keys[i] = the key that holds id d_ids[i]; UINT64_MAX when no key holds
 * it (never assigned, or reclaimed and not assigned again) or the id is >= capacity.  The
 * id -> key table (capacity u64, allocated by the first call) is built from the slots by
 * one pass, again whenever ids have been assigned or reclaimed since; like a lookup it
 * must not run concurrently with an assign or a reclaim on another stream. */
tbe_status tbe_dir_keys_of_device(tbe_directory *dir, const uint64_t *d_ids, uint64_t n, uint64_t *d_keys,
                                  void *stream);
/* Keys held: ids assigned and not reclaimed since (synchronises the directory's device). */
tbe_status tbe_dir_size(tbe_directory *dir, uint64_t *n_ids);
/* The same without synchronising: enqueues on `stream` a copy of {keys held, error
 * bits} (two u64; error bits != 0 once a batch exceeded the capacity, the condition
 * tbe_dir_size reports as TBE_ERANGE) into out2, pinned host or device memory.  Lets a
 * caller notice an overflow a batch later without a device synchronisation per batch;
 * the batch that overflowed is caught by the engine anyway (its UINT64_MAX ids make the
 * engine batch invalid). */
tbe_status tbe_dir_state_async(tbe_directory *dir, uint64_t *out2, void *stream);

/* Remove the keys flagged dead and reuse their ids.  d_dead: `capacity` bytes of device
 * memory indexed by id (tbe_expired_device over [0, capacity) writes them); d_keep_ids:
 * n_keep ids (device memory) that are never removed; a keep id >= capacity is ignored and
 * an id given twice is harmless.  For every id that is assigned, flagged and not kept: its
 * key leaves the directory (tbe_dir_lookup_device: UINT64_MAX; tbe_dir_keys_of_device:
 * UINT64_MAX for the id until it is assigned again, then the new key) and the id goes onto
 * the free stack (ascending id order within one reclaim).  Every other key keeps its id.
 * *d_n_reclaimed (device memory, may be NULL) gets the number of keys removed.  Enqueued
 * on `stream`, nothing is synchronised.
 *
 * The table stays a plain linear-probe table without tombstones: the reclaim rebuilds it
 * from the survivors, so probe chains that ran through a removed key still resolve.  After
 * an overflow (TBE_ERANGE) a reclaim still works within bounds and frees ids, but the error
 * state stays; slots that hold a key without an id are dropped.
 *
 * Contract: the reclaim rebuilds the slot table, so
 *   - no assign, lookup or keys_of may be in flight on another stream (work enqueued on
 *     `stream` before and after the call is ordered as usual);
 *   - d_dead must describe the engine after every batch that used this directory's ids;
 *     an id handed out by an assign whose engine batch has not been submitted yet has
 *     an absent row and would be flagged: such ids go in d_keep_ids.
 * Cost: two passes over the ids and three over the slots plus the re-insertion of the live
 * keys: a maintenance call made every few seconds to minutes.  The first reclaim allocates
 * its working memory, kept until tbe_dir_destroy: 17 bytes per id of capacity (1 of flags,
 * 4 of free stack, 12 of survivor records) and 4 bytes per 1024 ids and per 1024 slots. */
tbe_status tbe_dir_reclaim_device(tbe_directory *dir, const uint8_t *d_dead,
                                  const uint64_t *d_keep_ids, uint64_t n_keep,
                                  uint64_t *d_n_reclaimed, void *stream);

/* The periodic call of a host: tbe_expired_device(engine, ts_us, 0, capacity, clear = 1)
 * followed by tbe_dir_reclaim_device, ordered after everything enqueued before it on any
 * stream; synchronous.  The engine must be of the token-bucket or queueing kind, on the
 * directory's device, with n_keys >= capacity; anything else (the approximate kind, which
 * tbe_expired_device refuses, included) is TBE_EINVAL and nothing changes.  The lapsed rows
 * are written back absent, so a reused id starts from a full bucket whatever timestamp
 * comes next.  keep_ids is a host array (may be NULL when n_keep is 0); *n_reclaimed =
 * keys removed.  One more byte per id of capacity is held for the flags.
 * On an engine with limit classes (tbe_create_classes) each key lapses by its own class's
 * TTL, and a reclaimed id keeps the class byte of the key that held it: the caller sets the
 * class of the new key (tbe_set_class) before that key's first batch. */
tbe_status tbe_dir_reclaim(tbe_directory *dir, tbe_engine *engine, int64_t ts_us,
                           const uint64_t *keep_ids, uint64_t n_keep, uint64_t *n_reclaimed);

#ifdef __cplusplus
}
#endif

#endif /* TBE_CLUSTER_H_ */
