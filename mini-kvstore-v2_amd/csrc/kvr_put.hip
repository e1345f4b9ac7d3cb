/*
 * kvr_put.hip — batched writes on the device, included by kvr_api.hip.
 *
 * KVStore::set (engine.rs:157-179) / KVStore::delete (engine.rs:182-198) for n operations at once,
 * against the index kvr_replay_index / kvr_ingest_index left in HBM: the batch is framed as the
 * bytes the reference would append, the values' CRC-32s (the ETags of storage.rs:27) and the key
 * tags are computed, and the live list and the key table are rebuilt beside the old ones in
 * O(live keys + n) and swapped in when everything succeeded.  No byte of an old segment is read
 * except for key compares during the probe.
 *   k_put_key       one op per lane: validation (offsets, op byte, DEL without value, UTF-8), key
 *                   CRC, record size, and the in-batch last writer: a scratch open-addressing
 *                   table claims one representative op per distinct key (CAS; key bytes compared in
 *                   the arena, CRC-colliding keys are distinct keys), then atomicMax of the op index
 *   ExclusiveSum    record sizes -> offsets in the batch; value chunk counts -> the ETag kernels' map
 *   k_put_probe     op i is batch-last iff it holds its key's maximum; a batch-last op probes the
 *                   resident table as k_get_probe does and clears the keep flag of the live entry
 *                   it supersedes; a batch-last SET raises its own flag
 *   k_put_frame     one wave per record: header bytes, key and value copied with 16-B stores to
 *                   the 16-B aligned part of the destination, heads and tails one byte per lane
 *   etag kernels    the batch ETag path over the value arena; k_put_tuples assembles the tuples
 *   ExclusiveSum    keep flags -> positions; k_put_scatter writes the new live list (old entries
 *                   kept, in order, then the batch-last SETs in batch order); k_put_table inserts
 *                   it into a fresh table by CAS (live keys are distinct: no key compare)
 * Two host syncs: after k_put_probe (sizes, error flags, counts) and at the end.
 */

namespace {

constexpr int PUT_T = 256;   // one op per lane; the 256 threads also derive the CRC byte table
constexpr uint32_t PUT_ERR_OFF = 1u, PUT_ERR_OP = 2u, PUT_ERR_DELVAL = 4u, PUT_ERR_UTF8 = 8u;
constexpr unsigned long long PUT_EMPTY = ~0ull;
// totals (u64): [0] bytes of the batch, [1] n, [2] value chunks, [3] PUT_ERR_*, [4] SETs, [5] DELs,
// [6] live entries superseded, [7] batch-last SETs, [8] end of the value arena (val_off[n])
constexpr int PUT_NTOT = 9;

// std::str::from_utf8 acceptance, as the replay's KVR_E_UTF8 check and the oracle's oracle_utf8_check
__host__ __device__ inline bool put_utf8_ok(const uint8_t *s, uint64_t n) {
    uint64_t i = 0;
    while (i < n) {
        const uint32_t b = s[i];
        if (b < 0x80u) { ++i; continue; }
        const uint32_t w = (b >= 0xC2u && b <= 0xDFu) ? 2u : (b >= 0xE0u && b <= 0xEFu) ? 3u : (b >= 0xF0u && b <= 0xF4u) ? 4u : 0u;
        if (!w || i + w > n) return false;
        const uint32_t c1 = s[i + 1];
        uint32_t lo = 0x80u, hi = 0xBFu;
        if (b == 0xE0u) lo = 0xA0u;
        if (b == 0xEDu) hi = 0x9Fu;
        if (b == 0xF0u) lo = 0x90u;
        if (b == 0xF4u) hi = 0x8Fu;
        if (c1 < lo || c1 > hi) return false;
        for (uint32_t k = 2; k < w; ++k)
            if ((s[i + k] & 0xC0u) != 0x80u) return false;
        i += w;
    }
    return true;
}

__global__ __launch_bounds__(PUT_T) void k_put_key(const uint8_t *__restrict__ ops, const uint8_t *__restrict__ keys,
                                                   const uint64_t *__restrict__ key_off, const uint64_t *__restrict__ val_off,
                                                   uint64_t n, unsigned long long *__restrict__ tab, uint32_t *__restrict__ best,
                                                   uint64_t tmask, uint32_t *__restrict__ tag, uint32_t *__restrict__ slot_of,
                                                   uint64_t *__restrict__ size, uint64_t *__restrict__ vlen,
                                                   uint64_t *__restrict__ nch, unsigned long long *__restrict__ totals) {
    __shared__ uint32_t T[256];   // the CRC-32/ISO-HDLC byte table, as k_get_probe derives it
    {
        uint32_t c = threadIdx.x;
#pragma unroll
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (POLY & (0u - (c & 1u)));
        T[threadIdx.x] = c;
    }
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * PUT_T + threadIdx.x;
    const bool active = i < n;
    bool is_set = false, is_del = false;
    if (active) {
        const uint64_t k0 = key_off[i], k1 = key_off[i + 1], v0 = val_off[i], v1 = val_off[i + 1];
        const uint32_t op = ops[i];
        uint32_t err = 0;
        if (k1 < k0 || k1 - k0 >= (1ull << 32) || v1 < v0 || v1 - v0 >= (1ull << 32)) err = PUT_ERR_OFF;
        else if (op > 1u) err = PUT_ERR_OP;
        else if (op == 1u && v1 != v0) err = PUT_ERR_DELVAL;
        else if (!put_utf8_ok(keys + k0, k1 - k0)) err = PUT_ERR_UTF8;
        if (err) {   // the call answers KVR_EINVAL and changes nothing
            atomicOr(&totals[3], (unsigned long long)err);
            tag[i] = 0;
            slot_of[i] = 0;
            size[i] = 0;
            vlen[i] = 0;
            nch[i] = 0;
        } else {
            const uint32_t klen = (uint32_t)(k1 - k0);
            const uint64_t vl = v1 - v0;
            const uint8_t *kp = keys + k0;
            uint32_t crc = 0xFFFFFFFFu;
            uint32_t b = 0;
            for (; b + 8 <= klen; b += 8) {
                uint32_t x[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) x[q] = kp[b + q];
#pragma unroll
                for (int q = 0; q < 8; ++q) crc = (crc >> 8) ^ T[(crc ^ x[q]) & 255u];
            }
            for (; b < klen; ++b) crc = (crc >> 8) ^ T[(crc ^ kp[b]) & 255u];
            const uint32_t t = ~crc;
            is_set = op == 0u;
            is_del = !is_set;
            tag[i] = t;
            size[i] = 5ull + klen + (is_set ? 4ull + vl : 0ull);   // engine.rs:169-173 / :191-193
            vlen[i] = vl;
            nch[i] = (vl + ETAG_CH - 1) / ETAG_CH;
            // in-batch last writer: the first op to claim an entry represents its key; every op of
            // that key raises the entry's maximum.  An entry never changes once claimed, so a stale
            // read of an empty one only leads to a CAS that returns the claim.
            const unsigned long long me = ((unsigned long long)t << 32) | (uint32_t)i;
            for (uint64_t h = ix_hash(t) & tmask;; h = (h + 1) & tmask) {
                unsigned long long e = tab[h];
                if (e == PUT_EMPTY) {
                    e = atomicCAS(&tab[h], PUT_EMPTY, me);
                    if (e == PUT_EMPTY) e = me;
                }
                if ((uint32_t)(e >> 32) != t) continue;
                const uint32_t r = (uint32_t)e;
                if (r != (uint32_t)i) {
                    const uint64_t r0 = key_off[r], r1 = key_off[r + 1];
                    if (r1 - r0 != (uint64_t)klen || !bytes_eq(keys + r0, kp, klen)) continue;   // a colliding key
                }
                atomicMax(&best[h], (uint32_t)i + 1u);
                slot_of[i] = (uint32_t)h;
                break;
            }
        }
    }
    const unsigned long long bs = __ballot(is_set), bd = __ballot(is_del);
    if ((threadIdx.x & 63u) == 0) {
        if (bs) atomicAdd(&totals[4], (unsigned long long)__popcll(bs));
        if (bd) atomicAdd(&totals[5], (unsigned long long)__popcll(bd));
    }
}

// flags[0 .. n_live) arrive as 1 (keep); flags[n_live + i] = op i is a batch-last SET
__global__ __launch_bounds__(PUT_T) void k_put_probe(const uint8_t *__restrict__ ops, const uint8_t *__restrict__ keys,
                                                     const uint64_t *__restrict__ key_off, uint64_t n,
                                                     const uint32_t *__restrict__ best, const uint32_t *__restrict__ tag,
                                                     const uint32_t *__restrict__ slot_of, const kvr_tuple *__restrict__ live,
                                                     uint64_t n_live, const uint32_t *__restrict__ slots, uint64_t n_slots,
                                                     const SegDesc *__restrict__ segs, uint32_t *__restrict__ flags,
                                                     unsigned long long *__restrict__ totals) {
    const uint64_t i = (uint64_t)blockIdx.x * PUT_T + threadIdx.x;
    bool sup = false, newset = false;
    if (i < n) {
        const bool last = best[slot_of[i]] == (uint32_t)i + 1u;
        if (last) {
            const uint64_t k0 = key_off[i];
            const uint32_t klen = (uint32_t)(key_off[i + 1] - k0), t = tag[i];
            const uint8_t *kp = keys + k0;
            const uint64_t mask = n_slots - 1;
            uint64_t h = ix_hash(t) & mask;
            for (uint64_t probe = 0; probe < n_slots; ++probe, h = (h + 1) & mask) {   // k_get_probe's walk
                const uint32_t v = slots[h];
                if (v == 0) break;
                if (v == IX_DEAD || (uint64_t)v > n_live) continue;
                const uint4 *tp = reinterpret_cast<const uint4 *>(live + (v - 1u));
                const uint4 a = tp[0], c = tp[1];
                if (c.z != t || a.w != klen) continue;
                const uint64_t rec_off = (uint64_t)a.x | ((uint64_t)a.y << 32);
                if (!bytes_eq(segs[a.z].base + rec_off + 5, kp, klen)) continue;
                flags[v - 1u] = 0;   // one batch-last op per key: no other lane writes this flag
                sup = true;
                break;
            }
            newset = ops[i] == 0;
        }
        flags[n_live + i] = newset ? 1u : 0u;
    }
    const unsigned long long b0 = __ballot(sup), b1 = __ballot(newset);
    if ((threadIdx.x & 63u) == 0) {
        if (b0) atomicAdd(&totals[6], (unsigned long long)__popcll(b0));
        if (b1) atomicAdd(&totals[7], (unsigned long long)__popcll(b1));
    }
}

__global__ void k_put_totals(const uint64_t *__restrict__ off, const uint64_t *__restrict__ cpre,
                             const uint64_t *__restrict__ val_off, uint64_t n, unsigned long long *__restrict__ totals) {
    if (threadIdx.x || blockIdx.x) return;
    totals[0] = off[n];
    totals[1] = n;
    totals[2] = cpre[n];
    totals[8] = val_off[n];
}

// len bytes from sp to dst by one wave: the 16-B aligned part of the destination as 16 B per lane
// (five source dwords funnel-shifted, as k_gather_r), the bytes before and after it one per lane.
// Only bytes of [dst, dst + len) are written: a neighbouring record's wave owns the rest of a
// shared 16-B word.
__device__ __forceinline__ void put_copy(uint8_t *dst, const uint8_t *sp, uint64_t len, int lane) {
    if (len == 0) return;
    const uint64_t da = reinterpret_cast<uint64_t>(dst), src = reinterpret_cast<uint64_t>(sp);
    uint64_t a0 = ((da + 15) & ~15ull) - da, a1;
    if (((da + 15) & ~15ull) >= ((da + len) & ~15ull)) { a0 = len; a1 = len; }   // no whole 16-B word (len < 32)
    else a1 = ((da + len) & ~15ull) - da;
    {
        const uint64_t nh = a0, nt = len - a1;   // head [0, a0), tail [a1, len): fewer than 32 and 16
        if ((uint64_t)lane < nh) dst[lane] = sp[lane];
        if ((uint64_t)lane < nt) dst[a1 + lane] = sp[a1 + lane];
    }
    for (uint64_t xb = a0; xb < a1; xb += 4 * 1024) {
        uint32_t d[4][5];
        uint32_t sh[4];
        bool on[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint64_t x = xb + (uint64_t)u * 1024 + 16u * (uint32_t)lane;
            on[u] = x < a1;
            const uint64_t sa = src + (on[u] ? x : 0);
            const uint32_t *b = reinterpret_cast<const uint32_t *>(sa & ~3ull);
            sh[u] = (uint32_t)sa & 3u;
            if (on[u]) {
#pragma unroll
                for (int q = 0; q < 4; ++q) d[u][q] = b[q];
                d[u][4] = sh[u] ? b[4] : 0u;   // b[4] holds byte sa + 15 when sh != 0
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!on[u]) continue;
            const uint64_t x = xb + (uint64_t)u * 1024 + 16u * (uint32_t)lane;
            uint4 v;
            v.x = __builtin_amdgcn_alignbyte(d[u][1], d[u][0], sh[u]);
            v.y = __builtin_amdgcn_alignbyte(d[u][2], d[u][1], sh[u]);
            v.z = __builtin_amdgcn_alignbyte(d[u][3], d[u][2], sh[u]);
            v.w = __builtin_amdgcn_alignbyte(d[u][4], d[u][3], sh[u]);
            *reinterpret_cast<uint4 *>(dst + x) = v;
        }
    }
}

// one wave per record (grid-stride): record j to out[off[j] ..)
__global__ void __launch_bounds__(CT_GATHER) k_put_frame(const uint8_t *__restrict__ ops, const uint8_t *__restrict__ keys,
                                                         const uint64_t *__restrict__ key_off, const uint8_t *__restrict__ vals,
                                                         const uint64_t *__restrict__ val_off, const uint64_t *__restrict__ off,
                                                         uint64_t n, uint8_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (CT_GATHER / 64);
    const uint64_t w0 = (uint64_t)blockIdx.x * (CT_GATHER / 64) + (uint64_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t j = w0; j < n; j += waves) {
        const uint32_t op = ops[j];
        const uint64_t k0 = key_off[j];
        const uint32_t klen = (uint32_t)(key_off[j + 1] - k0);
        uint8_t *dst = out + off[j];
        if (lane == 0) dst[0] = (uint8_t)op;
        if (lane >= 1 && lane < 5) dst[lane] = (uint8_t)(klen >> (8 * (lane - 1)));
        put_copy(dst + 5, keys + k0, klen, lane);
        if (op == 0) {
            const uint64_t v0 = val_off[j];
            const uint32_t vl = (uint32_t)(val_off[j + 1] - v0);
            if (lane < 4) dst[5 + (uint64_t)klen + lane] = (uint8_t)(vl >> (8 * lane));
            put_copy(dst + 9 + (uint64_t)klen, vals + v0, vl, lane);
        }
    }
}

// tuples[i]: what kvr_replay emits for record i of the active segment
__global__ void k_put_tuples(const uint8_t *__restrict__ ops, const uint64_t *__restrict__ key_off,
                             const uint64_t *__restrict__ vlen, const uint64_t *__restrict__ off,
                             const uint32_t *__restrict__ crc, const uint32_t *__restrict__ tag, uint64_t n,
                             uint64_t base_off, uint32_t seg_idx, kvr_tuple *__restrict__ tup) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t ro = base_off + off[i];
    const uint32_t op = ops[i];
    uint4 a, b;
    a.x = (uint32_t)ro;
    a.y = (uint32_t)(ro >> 32);
    a.z = seg_idx;
    a.w = (uint32_t)(key_off[i + 1] - key_off[i]);
    b.x = op ? 0u : (uint32_t)vlen[i];
    b.y = op ? 0u : crc[i];
    b.z = tag[i];
    b.w = op;   // op, flags 0, reserved 0
    uint4 *o = reinterpret_cast<uint4 *>(tup + i);
    o[0] = a;
    o[1] = b;
}

// the new live list: the old entries still flagged, in order, then the batch-last SETs
__global__ void k_put_scatter(const kvr_tuple *__restrict__ live, uint64_t n_live, const kvr_tuple *__restrict__ tup,
                              uint64_t n, const uint32_t *__restrict__ flags, const uint32_t *__restrict__ pos,
                              kvr_tuple *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_live + n || !flags[i]) return;
    const uint4 *s = reinterpret_cast<const uint4 *>(i < n_live ? live + i : tup + (i - n_live));
    uint4 *o = reinterpret_cast<uint4 *>(out + pos[i]);
    const uint4 a = s[0], b = s[1];
    o[0] = a;
    o[1] = b;
}

// the key table over the new live list (cleared before): live keys are distinct, so an entry is
// placed at the first free slot of its probe sequence without a key compare
__global__ void k_put_table(const kvr_tuple *__restrict__ live, uint64_t n_live, uint32_t *__restrict__ slots,
                            uint64_t n_slots) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_live) return;
    const uint64_t mask = n_slots - 1;
    for (uint64_t h = ix_hash(live[j].key_tag) & mask;; h = (h + 1) & mask)
        if (atomicCAS(&slots[h], 0u, (uint32_t)j + 1u) == 0u) break;
}

// the device segment table with room for entry idx: DevBuf::ensure does not keep contents, so a
// larger table is allocated beside the old one and the entries before idx are copied over
int put_seg_room(kvr_ctx *c, size_t idx) {
    if (c->segs.p && c->segs.n > idx) return KVR_OK;
    DevBuf<SegDesc> nb;
    if (nb.ensure(std::max<size_t>(2 * (idx + 1), 16))) return KVR_ENOMEM;
    const size_t keep = c->segs.p ? std::min(c->segs.n, idx) : 0;
    HIPCHK(hipMemsetAsync(nb.p, 0, nb.n * sizeof(SegDesc), c->stream));
    if (keep) HIPCHK(hipMemcpyAsync(nb.p, c->segs.p, keep * sizeof(SegDesc), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->segs.release();
    c->segs = nb;
    c->up_segs_p = nullptr;   // a later replay uploads its own descriptors
    return KVR_OK;
}

// entry idx of the device segment table = a segment of len bytes at base (which: the host copy the
// queued transfer reads; a call's two uploads use one each, so neither is rewritten while in flight)
int put_seg_entry(kvr_ctx *c, int which, size_t idx, const uint8_t *base, uint64_t len) {
    SegDesc &d = c->p_desc[which];
    d = SegDesc{};
    d.base = base;
    d.len = len;
    d.d0 = (uint32_t)(reinterpret_cast<uintptr_t>(base) & 15u);
    HIPCHK(hipMemcpyAsync(c->segs.p + idx, &d, sizeof(SegDesc), hipMemcpyHostToDevice, c->stream));
    c->up_segs_p = nullptr;
    return KVR_OK;
}

bool put_active(const kvr_ctx *c) { return c->ix_valid && c->ix_slots && c->p_open && c->p_epoch == c->ix_epoch; }

}  // namespace

extern "C" {

int kvr_last_put_stats(const kvr_ctx *c, kvr_put_stats *out) {
    if (!c || !out) return KVR_EINVAL;
    *out = c->pstats;
    return KVR_OK;
}

int kvr_active_segment(const kvr_ctx *c, uint64_t *seg_id, uint32_t *seg_idx, uint64_t *len, const uint8_t **d_base) {
    if (!c || !put_active(c)) return KVR_EINVAL;
    if (seg_id) *seg_id = c->p_seg_id;
    if (seg_idx) *seg_idx = c->p_idx;
    if (len) *len = c->p_len;
    if (d_base) *d_base = c->p_act.p;
    return KVR_OK;
}

int kvr_put_batch(kvr_ctx *c, uint64_t seg_id, const uint8_t *ops, const uint8_t *keys, const uint64_t *key_off,
                  const uint8_t *vals, const uint64_t *val_off, size_t n, uint32_t flags, uint8_t *out, uint64_t out_cap,
                  uint64_t *out_len, kvr_tuple *tuples, uint64_t *seg_off) {
    if (!c || !out_len) return KVR_EINVAL;
    if (flags & ~(KVR_KEYS_ON_DEVICE | KVR_VALS_ON_DEVICE | KVR_OUT_ON_DEVICE)) return KVR_EINVAL;
    const bool dev_keys = flags & KVR_KEYS_ON_DEVICE, dev_vals = flags & KVR_VALS_ON_DEVICE, dev_out = flags & KVR_OUT_ON_DEVICE;
    *out_len = 0;
    if (!c->ix_valid || c->ix_slots == 0) return KVR_EINVAL;   // no key table (or a later call replaced it)
    const bool have = put_active(c);
    if (have ? seg_id < c->p_seg_id : (c->ix_nsegs && seg_id <= c->ix_last_id)) return KVR_EINVAL;
    const bool same = have && seg_id == c->p_seg_id;
    const uint64_t base_off = same ? c->p_len : 0;
    if (seg_off) *seg_off = base_off;
    if (n == 0) return KVR_OK;
    const uint64_t n_live = c->ix_live;
    if (n >= 0x7FFFFFFFull || n_live + n + 1 >= 0x7FFFFFFFull) return KVR_EINVAL;   // (the scans count in int)
    if (!ops || !key_off || !val_off || (out_cap && !out)) return KVR_EINVAL;
    if (!dev_keys) {
        for (size_t i = 0; i < n; ++i)
            if (key_off[i + 1] < key_off[i] || key_off[i + 1] - key_off[i] >= (1ull << 32)) return KVR_EINVAL;
        if (key_off[n] && !keys) return KVR_EINVAL;
        for (size_t i = 0; i < n; ++i)   // the reference takes &str (engine.rs:157, :182)
            if (!put_utf8_ok(keys + key_off[i], key_off[i + 1] - key_off[i])) return KVR_EINVAL;
    } else if (!keys) {
        return KVR_EINVAL;
    }
    if (!dev_vals) {
        for (size_t i = 0; i < n; ++i) {
            if (val_off[i + 1] < val_off[i] || val_off[i + 1] - val_off[i] >= (1ull << 32)) return KVR_EINVAL;
            if (ops[i] > 1 || (ops[i] == KVR_OP_DEL && val_off[i + 1] != val_off[i])) return KVR_EINVAL;
        }
        if (val_off[n] && !vals) return KVR_EINVAL;
    } else if (!vals) {
        return KVR_EINVAL;
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (!c->p_ev[0])
        for (auto &e : c->p_ev) HIPCHK(hipEventCreate(&e));

    // the scratch of this call
    uint64_t M = 16;
    while (M < 2 * (uint64_t)n) M <<= 1;   // the in-batch table: at least 2 n entries
    const uint64_t nf = n_live + n;         // flags: the old live entries, then the ops
    if (c->p_tab.ensure(M) || c->p_best.ensure(M) || c->p_tag.ensure(n) || c->p_slot.ensure(n) || c->p_size.ensure(n + 1) ||
        c->p_off.ensure(n + 1) || c->p_vlen.ensure(n + 1) || c->p_nch.ensure(n + 1) || c->p_cpre.ensure(n + 1) ||
        c->p_flags.ensure(nf + 1) || c->p_pos.ensure(nf + 1) || c->p_tot.ensure(PUT_NTOT) || c->p_crc.ensure(n) ||
        c->p_tup.ensure(n))
        return KVR_ENOMEM;
    const uint8_t *d_ops = ops, *d_keys = keys, *d_vals = vals;
    const uint64_t *d_koff = key_off, *d_voff = val_off;
    if (!dev_keys) {
        const uint64_t kb = key_off[n];
        if (c->p_keys.ensure(kb + 16) || c->p_koff.ensure(n + 1)) return KVR_ENOMEM;
        if (kb) HIPCHK(hipMemcpyAsync(c->p_keys.p, keys, kb, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(c->p_koff.p, key_off, (n + 1) * 8, hipMemcpyHostToDevice, st));
        d_keys = c->p_keys.p;
        d_koff = c->p_koff.p;
    }
    if (!dev_vals) {
        const uint64_t vb = val_off[n];
        if (c->p_vals.ensure(vb + 16) || c->p_voff.ensure(n + 1) || c->p_ops.ensure(n)) return KVR_ENOMEM;
        if (vb) HIPCHK(hipMemcpyAsync(c->p_vals.p, vals, vb, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(c->p_voff.p, val_off, (n + 1) * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(c->p_ops.p, ops, n, hipMemcpyHostToDevice, st));
        d_vals = c->p_vals.p;
        d_voff = c->p_voff.p;
        d_ops = c->p_ops.p;
    }
    size_t tb1 = 0, tb2 = 0;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb1, c->p_size.p, c->p_off.p, (int)(n + 1), st));
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, c->p_flags.p, c->p_pos.p, (int)(nf + 1), st));
    if (c->p_tmp.n < std::max(tb1, tb2) && c->p_tmp.ensure(std::max(tb1, tb2))) return KVR_ENOMEM;
    unsigned long long *d_tot = reinterpret_cast<unsigned long long *>(c->p_tot.p);
    const uint32_t g = (uint32_t)((n + PUT_T - 1) / PUT_T);

    // 1. keys, sizes, the in-batch last writers, the live entries they supersede
    HIPCHK(hipMemsetAsync(c->p_tab.p, 0xFF, M * 8, st));
    HIPCHK(hipMemsetAsync(c->p_best.p, 0, M * 4, st));
    HIPCHK(hipMemsetAsync(c->p_tot.p, 0, PUT_NTOT * 8, st));
    HIPCHK(hipMemsetAsync(c->p_size.p + n, 0, 8, st));
    HIPCHK(hipMemsetAsync(c->p_nch.p + n, 0, 8, st));
    if (n_live) HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->p_flags.p), 1, n_live, st));
    HIPCHK(hipMemsetAsync(c->p_flags.p + nf, 0, 4, st));
    HIPCHK(hipEventRecord(c->p_ev[0], st));
    hipLaunchKernelGGL(k_put_key, dim3(g), dim3(PUT_T), 0, st, d_ops, d_keys, d_koff, d_voff, (uint64_t)n, c->p_tab.p,
                       c->p_best.p, M - 1, c->p_tag.p, c->p_slot.p, c->p_size.p, c->p_vlen.p, c->p_nch.p, d_tot);
    HIPCHK(hipGetLastError());
    size_t tb = c->p_tmp.n;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(c->p_tmp.p, tb, c->p_size.p, c->p_off.p, (int)(n + 1), st));
    tb = c->p_tmp.n;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(c->p_tmp.p, tb, c->p_nch.p, c->p_cpre.p, (int)(n + 1), st));
    hipLaunchKernelGGL(k_put_probe, dim3(g), dim3(PUT_T), 0, st, d_ops, d_keys, d_koff, (uint64_t)n, c->p_best.p, c->p_tag.p,
                       c->p_slot.p, c->lout.p, n_live, c->islots.p, c->ix_slots, c->segs.p, c->p_flags.p, d_tot);
    hipLaunchKernelGGL(k_put_totals, dim3(1), dim3(64), 0, st, c->p_off.p, c->p_cpre.p, d_voff, (uint64_t)n, d_tot);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->p_ev[1], st));
    uint64_t tot[PUT_NTOT] = {};
    HIPCHK(hipMemcpyAsync(tot, c->p_tot.p, sizeof(tot), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (tot[3]) return KVR_EINVAL;   // device inputs: offsets, an op byte, a DEL with a value, a key that is not UTF-8
    const uint64_t total = tot[0], nch = tot[2], n_sup = tot[6], n_newset = tot[7], vals_end = tot[8];
    *out_len = total;
    if (total > out_cap) return KVR_CAPACITY;
    if (nch >= 0xFFFFFFFFull || vals_end >= (1ull << 48)) return KVR_EINVAL;   // (k_etag_map's descriptors)
    const uint64_t n_new = n_live - n_sup + n_newset;
    if (n_new >= 0xFFFFFFFFull) return KVR_EINVAL;
    const uint64_t ns_new = index_slots(n_new);

    // 2. the active segment: the same one (grown with its contents when it is full), the first one
    // after an index build, or the next one (in p_next until this call succeeds)
    const uint32_t seg_idx = !have ? (uint32_t)c->ix_nsegs : same ? c->p_idx : c->p_idx + 1u;
    DevBuf<uint8_t> *act = have && !same ? &c->p_next : &c->p_act;
    const uint64_t need = base_off + total + 16;
    if (same && act->n < need) {
        DevBuf<uint8_t> nb;
        if (nb.ensure(std::max<uint64_t>(2 * need, 1ull << 20))) return KVR_ENOMEM;
        if (c->p_len) HIPCHK(hipMemcpyAsync(nb.p, act->p, c->p_len, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        act->release();
        *act = nb;
        const int rc = put_seg_entry(c, 0, seg_idx, act->p, c->p_len);   // the segment moved: same bytes, new base
        if (rc != KVR_OK) return rc;
    } else if (!same && act->ensure(std::max<uint64_t>(2 * need, 1ull << 20))) {
        return KVR_ENOMEM;
    }
    if (!have) {   // the segments closed under an earlier index are gone with it
        for (auto &b : c->p_closed) b.release();
        c->p_closed.clear();
    }
    if (c->p_live.ensure(n_new) || c->p_slots.ensure(ns_new)) return KVR_ENOMEM;
    int rc = put_seg_room(c, seg_idx);
    if (rc != KVR_OK) return rc;
    uint8_t *d_rec = act->p + base_off;

    // 3. framing
    HIPCHK(hipEventRecord(c->p_ev[2], st));
    hipLaunchKernelGGL(k_put_frame, dim3((uint32_t)std::min<uint64_t>((uint64_t)c->n_cu * 16, (n + 3) / 4)), dim3(CT_GATHER), 0,
                       st, d_ops, d_keys, d_koff, d_vals, d_voff, c->p_off.p, (uint64_t)n, d_rec);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->p_ev[3], st));

    // 4. value CRCs (the ETags) over the input arena, tuples
    rc = etag_launch(c, d_vals, vals_end, d_voff, c->p_vlen.p, c->p_cpre.p, n, nch, nullptr, c->p_crc.p);
    if (rc != KVR_OK) return rc;
    hipLaunchKernelGGL(k_put_tuples, dim3(g), dim3(PUT_T), 0, st, d_ops, d_koff, c->p_vlen.p, c->p_off.p, c->p_crc.p,
                       c->p_tag.p, (uint64_t)n, base_off, seg_idx, c->p_tup.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->p_ev[4], st));

    // 5. the new live list and its table, beside the old ones
    tb = c->p_tmp.n;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(c->p_tmp.p, tb, c->p_flags.p, c->p_pos.p, (int)(nf + 1), st));
    HIPCHK(hipMemsetAsync(c->p_slots.p, 0, ns_new * 4, st));
    hipLaunchKernelGGL(k_put_scatter, dim3((uint32_t)((nf + 255) / 256)), dim3(256), 0, st, c->lout.p, n_live, c->p_tup.p,
                       (uint64_t)n, c->p_flags.p, c->p_pos.p, c->p_live.p);
    if (n_new)
        hipLaunchKernelGGL(k_put_table, dim3((uint32_t)((n_new + 255) / 256)), dim3(256), 0, st, c->p_live.p, n_new,
                           c->p_slots.p, ns_new);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->p_ev[5], st));
    rc = put_seg_entry(c, 1, seg_idx, act->p, base_off + total);
    if (rc != KVR_OK) return rc;
    const hipMemcpyKind k = dev_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (total) HIPCHK(hipMemcpyAsync(out, d_rec, total, k, st));
    if (tuples) HIPCHK(hipMemcpyAsync(tuples, c->p_tup.p, n * sizeof(kvr_tuple), k, st));
    HIPCHK(hipStreamSynchronize(st));

    // 6. everything succeeded: the new state replaces the old
    std::swap(c->lout, c->p_live);
    std::swap(c->islots, c->p_slots);
    if (have && !same) {
        c->p_closed.push_back(c->p_act);
        c->p_act = c->p_next;
        c->p_next = DevBuf<uint8_t>{};
    }
    c->ix_live = n_new;
    c->ix_slots = ns_new;
    c->ix_epoch = ++index_epochs;
    c->p_open = true;
    c->p_epoch = c->ix_epoch;
    c->p_seg_id = seg_id;
    c->p_idx = seg_idx;
    c->p_len = base_off + total;
    c->pstats = kvr_put_stats{};   // (a failed call leaves the last successful call's statistics)
    c->pstats.ms_frame = ev_ms(c->p_ev[2], c->p_ev[3]);
    c->pstats.ms_crc = ev_ms(c->p_ev[3], c->p_ev[4]);
    c->pstats.ms_index = ev_ms(c->p_ev[0], c->p_ev[1]) + ev_ms(c->p_ev[4], c->p_ev[5]);
    c->pstats.n_ops = n;
    c->pstats.n_set = tot[4];
    c->pstats.n_del = tot[5];
    c->pstats.bytes_out = total;
    c->pstats.n_superseded = n_sup;
    c->pstats.n_live = n_new;
    c->pstats.n_slots = ns_new;
    return KVR_OK;
}

}  // extern "C"
