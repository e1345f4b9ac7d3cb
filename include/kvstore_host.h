/*
 * kvstore_host.h — host side of the drop-in: the KVStore::open path of
 * whispem/mini-kvstore-v2 (src/store/engine.rs:24-76) rebuilt around kvr_replay.
 *
 *   kvh_discover      segment discovery + ordering        engine.rs:31-51
 *   kvh_gen_segment   synthetic segments, framing writer  engine.rs:157-198 (byte-identical to
 *                     kvr_gen_segment_device)
 *   kvh_fold          last-writer-wins index fold         engine.rs:137 (insert), :141 (remove)
 *   kvs_open / kvs_get / kvs_put_many / kvs_set / kvs_delete / kvs_list_keys / kvs_stats / kvs_compact / kvs_close
 *                     the crate-public KVStore surface the replay path feeds (lib.rs:2-3,
 *                     engine.rs:24, :200, :232-259); the index has the shape of the reference's
 *                     dead `Index` (src/store/index.rs:7): key -> (segment, offset, length).
 *
 * Status codes and kvr_error are those of kvreplay.h.
 */
#ifndef KVSTORE_HOST_H
#define KVSTORE_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "kvreplay.h"

#ifdef __cplusplus
extern "C" {
#endif

/* CPU generator: same bytes and manifest as kvr_gen_segment_device for (p, seg_no).
 * buf may be NULL to only size the segment (*len_out, *n_rec_out). */
int kvh_gen_segment(const kvr_gen_params *p, uint64_t seg_no, uint8_t *buf, uint64_t cap, uint64_t *len_out,
                    uint32_t *expected, uint64_t exp_cap, uint64_t *n_rec_out);

/* Discovery as engine.rs:31-51: entries of dir named "segment-<id>.dat" whose <id> parses as a
 * Rust u64 (optional '+', ASCII digits, no overflow), in ascending id order (ties by name).
 * Writes up to cap ids to ids[] and NUL-separated full paths into paths (path_cap bytes);
 * *n_out = number of segments found.  Returns KVR_OK, KVR_CAPACITY or KVR_EIO. */
int kvh_discover(const char *dir, uint64_t *ids, size_t cap, char *paths, size_t path_cap, size_t *n_out);

/* Rust `u64::from_str` on [s, s+n): returns 1 and *out on success. */
int kvh_parse_u64(const char *s, size_t n, uint64_t *out);

/* Fold tuples (in (segment, offset) order) by last-writer-wins.  Keys are read from
 * segs[t.seg_idx].bytes + t.rec_off + 5 (host memory).  live[i] = 1 iff tuple i is the final
 * SET of its key.  Returns the number of live keys (stats().num_keys) and *total_bytes
 * (stats().total_bytes, engine.rs:253-255). */
uint64_t kvh_fold(const kvr_segment *segs, const kvr_tuple *t, size_t n, uint8_t *live, uint64_t *total_bytes);
/* The same fold on n_threads host threads (0 = all cores): keys are split by
 * key_tag into one partition per thread (the last writer of a key is its maximal (segment,
 * offset) record, so partitions fold independently).  Same results as kvh_fold. */
uint64_t kvh_fold_parallel(const kvr_segment *segs, const kvr_tuple *t, size_t n, uint32_t n_threads,
                           uint8_t *live, uint64_t *total_bytes);

typedef struct kvs_store kvs_store;

typedef struct kvs_stats {          /* StoreStats, src/store/stats.rs:3-10 */
    uint64_t num_keys;
    uint64_t num_segments;
    uint64_t total_bytes;
    uint64_t active_segment_id;
    uint64_t oldest_segment_id;
} kvs_stats;

/* KVStore::open(dir): create the directory if missing, discover and read the segments,
 * replay them on ctx's GPU, fold the index, create the next active segment file
 * (engine.rs:59-68).  On KVR_CORRUPTED, *err and msg (the exact engine.rs message, without
 * error.rs's "Corrupted data: " prefix) describe the first error. */
int kvs_open(const char *dir, kvr_ctx *ctx, kvs_store **out, kvr_error *err, char *msg, size_t msg_cap);
/* kvs_open with options.  The default path maps every segment file read-only (mmap, populated
 * from the page cache by up to 16 threads: the store's host bytes are the page cache, no copy),
 * registers each mapping for DMA (kvr_host_register) and pushes the segment to HBM
 * (kvr_ingest_push) in store order.  KVS_OPEN_PREAD (or a failed mmap) reads the files instead:
 * 16 threads pread 8-MiB pieces into one arena on 2-MiB pages, and groups of consecutive segments
 * (>= 256 MiB) are registered and pushed as soon as their bytes are in, so reading and PCIe
 * overlap.  Then kvr_ingest_index replays, folds and builds the key table on the GPU and only the
 * live tuples and the table come back.  When the store does not fit in HBM (KVR_ENOMEM) or
 * exceeds the fold's 2^31-tuple limit (KVR_EINVAL), the host-fold path takes over:
 * kvr_replay_stream in batches, kvh_fold_parallel, kvr_index_build_host.  Both give the same index.
 * An unopenable segment k is reported (KVR_E_OPEN) only when segments 0 .. k-1 replay cleanly,
 * as engine.rs:55-57 opens the files one after the other.
 * Segment files must not be truncated by another process while the store is open: a mapped page
 * past the new end of file raises SIGBUS when it is touched (later DMA re-reads, compaction).  The
 * store itself only appends to the active file, and kvs_compact writes new files and unlinks the
 * old ones (an unlinked file's mapping keeps its pages), so its own mappings never lose bytes;
 * KVS_OPEN_PREAD copies the bytes and is immune to outside truncation. */
#define KVS_OPEN_HOST_FOLD  0x1u   /* force the host-fold path                         */
#define KVS_OPEN_NO_PIN     0x2u   /* no kvr_host_register: HIP stages the transfers    */
#define KVS_OPEN_PREAD      0x4u   /* read the files into an arena instead of mapping   */
#define KVS_PATH_DEVICE_INDEX 1u
#define KVS_PATH_HOST_FOLD    2u
#define KVS_LOAD_MMAP  1u
#define KVS_LOAD_PREAD 2u
typedef struct kvs_open_stats {
    double   ms_total;       /* the whole kvs_open_ex call                                        */
    double   ms_register;    /* kvr_host_register calls (inside ms_read)                           */
    double   ms_push;        /* kvr_ingest_push calls (inside ms_read)                             */
    double   ms_read;        /* loading: mapping or reading, registration, pushes                  */
    double   ms_index;       /* after loading -> index ready: transfer tail, replay, fold, copies  */
    uint64_t bytes;          /* segment bytes                                                      */
    uint64_t n_segments;
    uint64_t n_live;         /* stats().num_keys                                                   */
    uint32_t path;           /* KVS_PATH_DEVICE_INDEX or KVS_PATH_HOST_FOLD (last index build)      */
    uint32_t read_threads;
    uint32_t mode;           /* KVS_LOAD_MMAP or KVS_LOAD_PREAD                                     */
    uint32_t pad;
} kvs_open_stats;
/* ctx may be NULL: the store then opens on the host only, which succeeds only when its segments
 * hold no bytes (a new or emptied store); a store with records returns KVR_EINVAL. */
int kvs_open_ex(const char *dir, kvr_ctx *ctx, uint32_t flags, kvs_store **out, kvr_error *err, char *msg,
                size_t msg_cap);
int kvs_last_open_stats(const kvs_store *s, kvs_open_stats *out);
/* KVStore::get (engine.rs:200): 1 and the value bytes if live, 0 if absent. */
int kvs_get(const kvs_store *s, const uint8_t *key, size_t klen, const uint8_t **val, size_t *vlen);
/* The host multi-get over a host copy of an index (live, slots: kvr_replay_index's arrays or
 * kvr_index_build_host's) and its segments (host bytes): kvr_index_find per key, then memcpy of
 * the values, on n_threads host threads (0 or 1: the calling thread).  Arguments, outputs and
 * return codes as kvs_get_many, which runs this on one thread when the device cannot answer. */
int kvh_get_many(const kvr_tuple *live, size_t n_live, const uint32_t *slots, uint64_t n_slots, const kvr_segment *segs,
                 const uint8_t *keys, const uint64_t *key_off, size_t n, uint32_t n_threads, int64_t *live_idx,
                 uint64_t *val_off, uint8_t *vals, uint64_t vals_cap, uint64_t *val_bytes);
/* KVStore::get for n keys at once: key i is keys[key_off[i] .. key_off[i+1]); live_idx[i] = index
 * of the key's final SET in the store's live list, -1 = absent; value i is
 * vals[val_off[i] .. val_off[i+1]) (empty for a miss); *val_bytes = val_off[n].  All buffers are
 * host memory.  When ctx still holds the key table this store's last index build left on it
 * (kvr_index_epoch(ctx) is the value the store remembered), kvr_get_batch answers on the device;
 * otherwise (ctx NULL, the host-fold path, or the context used for another replay since) a host
 * loop over kvr_index_find and memcpy does.  Both give the same results.
 * Returns KVR_OK, KVR_CAPACITY when vals_cap < *val_bytes (live_idx, val_off and *val_bytes are
 * complete, nothing is written past vals + vals_cap), KVR_EINVAL (NULL where a buffer is needed,
 * key_off not non-decreasing, a key of 2^32 bytes or more) or < 0. */
int kvs_get_many(const kvs_store *s, kvr_ctx *ctx, const uint8_t *keys, const uint64_t *key_off, size_t n,
                 int64_t *live_idx, uint64_t *val_off, uint8_t *vals, uint64_t vals_cap, uint64_t *val_bytes);
/* Index entry (index.rs:7 shape): segment id, value offset inside that segment file, length. */
int kvs_locate(const kvs_store *s, const uint8_t *key, size_t klen, uint64_t *seg_id, uint64_t *val_off, uint64_t *len);
int kvs_stats_get(const kvs_store *s, kvs_stats *out);
/* KVStore::compact (engine.rs:262-266 -> compaction.rs:9-29) with the intended semantics of
 * README.md:283-287 (the reference deletes every segment without rewriting a key):
 * kvr_compact rewrites the live records into new files segment-<active+1>.dat, ... (segments
 * of about seg_target bytes, 0 = one file), written and fsync'd before every other
 * segment-*.dat is removed (compaction.rs:11-23); then a fresh empty active segment is created
 * (reset_active_segment, engine.rs:209-229) and the index is rebuilt over the new files.  A crash
 * between the writes and the removals leaves old and new files, whose replay gives the same map.
 * Returns KVR_OK, KVR_CORRUPTED (*err) or < 0 (KVR_EIO: a file could not be written/removed). */
int kvs_compact(kvs_store *s, kvr_ctx *ctx, uint64_t seg_target, kvr_error *err);
/* stats().num_keys: the number of live keys. */
size_t kvs_num_keys(const kvs_store *s);
/* KVStore::list_keys (engine.rs:204-206): the live keys as an arena, in the live list's order —
 * key i is keys[key_off[i] .. key_off[i+1]), key_off has num_keys + 1 entries, *key_bytes = the
 * total.  KVR_CAPACITY (*key_bytes set) when keys_cap or off_cap is short. */
int kvs_list_keys(const kvs_store *s, uint8_t *keys, uint64_t keys_cap, uint64_t *key_off, size_t off_cap,
                  uint64_t *key_bytes);

/* ---- writes: KVStore::set (engine.rs:157-179), KVStore::delete (engine.rs:182-198) -------------
 * kvh_encode_batch: the reference's loop on one host thread — the bytes set / delete would append
 * for n operations and the tuples kvr_replay would emit for them (rec_off from base_off, seg_idx as
 * given, crc32 = the ETag of storage.rs:27), with the arguments, the validation and the return
 * codes of kvr_put_batch's framing half: KVR_EINVAL (nothing written) for offsets that decrease, a
 * key or value of 2^32 bytes or more, an op byte other than 0 / 1, a DEL with a value, a key that
 * is not valid UTF-8, NULL where a buffer is needed; KVR_CAPACITY (*out_len set) when out_cap is
 * short.  It is kvs_put_many's fallback and the baseline of tools/put_bench.py. */
int kvh_encode_batch(const uint8_t *ops, const uint8_t *keys, const uint64_t *key_off, const uint8_t *vals,
                     const uint64_t *val_off, size_t n, uint32_t seg_idx, uint64_t base_off, uint8_t *out, uint64_t out_cap,
                     uint64_t *out_len, kvr_tuple *tuples);
/* The host index update behind a batch whose tuples are t[0 .. n) (kvh_encode_batch's; key i is
 * keys[key_off[i] .. key_off[i+1])): every key's last op of the batch supersedes the key's entry in
 * live[0 .. n_live) (found through slots / segs as kvr_index_find does), the entries that remain
 * keep their order, and the batch-last SETs follow in batch order — in place, live has room for
 * live_cap >= n_live entries; *n_live_out = the new count (KVR_CAPACITY, nothing changed, when it
 * exceeds live_cap).  The caller rebuilds the table with kvr_index_build_host.  One thread,
 * O(n_live + n). */
int kvh_index_update(kvr_tuple *live, size_t n_live, size_t live_cap, const uint32_t *slots, uint64_t n_slots,
                     const kvr_segment *segs, const kvr_tuple *t, const uint8_t *keys, const uint64_t *key_off, size_t n,
                     size_t *n_live_out);
/* n set / delete operations in order (arguments as kvr_put_batch, host memory): encoded on the
 * device (kvr_put_batch) while ctx still holds this store's key table (the epoch matches), else by
 * kvh_encode_batch; appended to segment-<active_id>.dat with one write per batch, flushed to the OS
 * as engine.rs:174 does; the active segment's bytes are kept as a host segment, so kvs_get and
 * kvs_locate read the new values; the host index follows (device path: kvr_index_fetch; host path:
 * superseded entries dropped, batch-last SETs appended, kvr_index_build_host).  Both refreshes are
 * O(live keys) per call: batches are the intended interface.  crc_out (optional): the ETag word
 * of value i (0 for a DEL).  stats().total_bytes and num_keys follow engine.rs:253-255.
 * Returns KVR_OK, KVR_EINVAL, KVR_EIO (the write failed; the store is unchanged) or < 0. */
int kvs_put_many(kvs_store *s, kvr_ctx *ctx, const uint8_t *ops, const uint8_t *keys, const uint64_t *key_off,
                 const uint8_t *vals, const uint64_t *val_off, size_t n, uint32_t *crc_out);
/* The n = 1 forms: KVStore::set (crc_out optional: BlobStorage::put's ETag word, storage.rs:26-35)
 * and KVStore::delete. */
int kvs_set(kvs_store *s, kvr_ctx *ctx, const uint8_t *key, size_t klen, const uint8_t *val, size_t vlen,
            uint32_t *crc_out);
int kvs_delete(kvs_store *s, kvr_ctx *ctx, const uint8_t *key, size_t klen);
void kvs_close(kvs_store *s);

#ifdef __cplusplus
}
#endif
#endif
