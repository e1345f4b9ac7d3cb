/*
 * kvr_get.hip — batched lookups and value gather on the device, included by kvr_api.hip.
 *
 * KVStore::get (engine.rs:200-202) for n keys at once against the index kvr_replay_index /
 * kvr_ingest_index left in HBM: the live list (lout), the key table (islots) and the segment
 * bytes are read where they are, nothing is rebuilt and nothing of them is written.
 *   k_get_probe     one query per lane: CRC-32 of the key, kvr_index_find's probe, the key bytes
 *                   compared in the segment -> live_idx, value length, value address
 *   ExclusiveSum    value lengths -> val_off[0 .. n]
 *   k_gather_r      the compaction's one-wave-per-record byte gather, unchanged: value i to
 *                   vals[val_off[i] .. val_off[i + 1])
 *   KVR_GET_VERIFY  k_get_expected (the tuples' crc32) + the batch ETag kernels over the packed
 *                   output + k_get_bad
 * Byte traffic per key: 8 B offsets + the key, one 4-B slot and one 32-B tuple per probe step
 * (random), the key bytes in the segment once (random), 24 B of outputs; the gather reads and
 * writes every value byte once.
 */

namespace {

constexpr int GET_T = 256;   // one query per lane; the 256 threads also derive the CRC byte table
constexpr uint32_t GET_ERR_KEY = 1u;   // totals[4]: key_off decreasing, or a key of 2^32 bytes or more

// totals (5 x u64): [0] value bytes, [1] n (k_gather_r's pair), [2] verify chunks, [3] keys found,
// [4] GET_ERR_*
__global__ __launch_bounds__(GET_T) void k_get_probe(const uint8_t *__restrict__ keys, const uint64_t *__restrict__ key_off,
                                                     uint64_t n, const kvr_tuple *__restrict__ live, uint64_t n_live,
                                                     const uint32_t *__restrict__ slots, uint64_t n_slots,
                                                     const SegDesc *__restrict__ segs, int64_t *__restrict__ live_idx,
                                                     uint64_t *__restrict__ vlen, uint64_t *__restrict__ l_src,
                                                     unsigned long long *__restrict__ totals) {
    // the CRC-32/ISO-HDLC byte table, one entry per thread (8 shift / XOR steps): no upload, and no
    // tie to the replay's replicated table layout
    __shared__ uint32_t T[256];
    {
        uint32_t c = threadIdx.x;
#pragma unroll
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (POLY & (0u - (c & 1u)));
        T[threadIdx.x] = c;
    }
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * GET_T + threadIdx.x;
    const bool active = i < n;
    int64_t found = -1;
    uint64_t val_len = 0, val_src = 0;
    if (active) {
        const uint64_t k0 = key_off[i], k1 = key_off[i + 1];
        if (k1 < k0 || k1 - k0 >= (1ull << 32)) {
            atomicOr(&totals[4], (unsigned long long)GET_ERR_KEY);   // the call answers KVR_EINVAL
        } else {
            const uint32_t klen = (uint32_t)(k1 - k0);
            const uint8_t *kp = keys + k0;
            // key tag = kvr_crc32(0, key, klen): byte-serial, 8 byte loads issued together; only
            // bytes of [k0, k1) are read
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
            const uint32_t tag = ~crc;
            // kvr_index_find's probe: 0 ends it, IX_DEAD is passed over, a live entry is compared
            // by tag, then length, then the key bytes in the segment (read only after both
            // matched, so inside the record).  Lanes leave at different steps: no wave-level
            // operation in here.
            const uint64_t mask = n_slots - 1;
            uint64_t h = ix_hash(tag) & mask;
            for (uint64_t probe = 0; probe < n_slots; ++probe, h = (h + 1) & mask) {
                const uint32_t v = slots[h];
                if (v == 0) break;
                if (v == IX_DEAD || (uint64_t)v > n_live) continue;
                const uint4 *tp = reinterpret_cast<const uint4 *>(live + (v - 1u));
                const uint4 a = tp[0], c = tp[1];   // {rec_off lo, hi, seg_idx, key_len}, {val_len, crc32, key_tag, op ..}
                if (c.z != tag || a.w != klen) continue;
                const uint64_t rec_off = (uint64_t)a.x | ((uint64_t)a.y << 32);
                const uint8_t *rec = segs[a.z].base + rec_off;
                if (!bytes_eq(rec + 5, kp, klen)) continue;
                found = (int64_t)(v - 1u);
                val_len = c.x;
                val_src = reinterpret_cast<uint64_t>(rec + 9 + klen);   // [op][klen][key][vlen][value]
                break;
            }
        }
        live_idx[i] = found;
        vlen[i] = val_len;
        l_src[i] = val_src;
    }
    const unsigned long long hits = __ballot(found >= 0);
    if ((threadIdx.x & 63u) == 0 && hits) atomicAdd(&totals[3], (unsigned long long)__popcll(hits));
}

// verify: value i's chunk count for the ETag kernels (an entry past the end for the scan's total)
__global__ void k_get_nch(const uint64_t *__restrict__ vlen, uint64_t n, uint64_t *__restrict__ nch) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) nch[i] = i < n ? (vlen[i] + ETAG_CH - 1) / ETAG_CH : 0;
}

__global__ void k_get_totals(const uint64_t *__restrict__ off, const uint64_t *__restrict__ cpre, uint64_t n,
                             unsigned long long *__restrict__ totals) {
    if (threadIdx.x || blockIdx.x) return;
    totals[0] = off[n];
    totals[1] = n;
    totals[2] = cpre ? cpre[n] : 0;
}

// verify: the CRC the replay stored with each found key's final SET; a miss has no bytes and
// expects crc32("") = 0
__global__ void k_get_expected(const kvr_tuple *__restrict__ live, const int64_t *__restrict__ live_idx, uint64_t n,
                               uint32_t *__restrict__ expected) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t j = live_idx[i];
    expected[i] = j >= 0 ? live[j].crc32 : 0u;
}

__global__ void k_get_bad(const uint32_t *__restrict__ crc, const uint32_t *__restrict__ expected, uint64_t n,
                          uint8_t *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) bad[i] = crc[i] != expected[i] ? 1 : 0;
}

}  // namespace

extern "C" {

uint64_t kvr_index_epoch(const kvr_ctx *c) { return c && c->ix_valid && c->ix_slots ? c->ix_epoch : 0; }

int kvr_last_get_stats(const kvr_ctx *c, kvr_get_stats *out) {
    if (!c || !out) return KVR_EINVAL;
    *out = c->gstats;
    return KVR_OK;
}

int kvr_get_batch(kvr_ctx *c, const uint8_t *keys, const uint64_t *key_off, size_t n, uint32_t flags, int64_t *live_idx,
                  uint64_t *val_off, uint8_t *vals, uint64_t vals_cap, uint64_t *val_bytes, uint8_t *bad,
                  uint64_t *n_crc_fail) {
    if (!c || !val_bytes) return KVR_EINVAL;
    if (flags & ~(KVR_KEYS_ON_DEVICE | KVR_OUT_ON_DEVICE | KVR_GET_LOCATE_ONLY | KVR_GET_VERIFY)) return KVR_EINVAL;
    const bool locate = flags & KVR_GET_LOCATE_ONLY, verify = flags & KVR_GET_VERIFY;
    const bool dev_keys = flags & KVR_KEYS_ON_DEVICE, dev_out = flags & KVR_OUT_ON_DEVICE;
    if (locate && verify) return KVR_EINVAL;   // nothing gathered, nothing to verify
    *val_bytes = 0;
    if (n_crc_fail) *n_crc_fail = 0;
    if (!c->ix_valid || c->ix_slots == 0) return KVR_EINVAL;   // no key table (or a later call replaced it)
    memset(&c->gstats, 0, sizeof(c->gstats));
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (n == 0) {
        if (val_off && dev_out) {
            HIPCHK(hipMemsetAsync(val_off, 0, 8, st));
            HIPCHK(hipStreamSynchronize(st));
        } else if (val_off) {
            val_off[0] = 0;
        }
        return KVR_OK;
    }
    if (!key_off || !live_idx || !val_off || (!locate && vals_cap && !vals)) return KVR_EINVAL;
    if (n >= 0x7FFFFFFFull) return KVR_EINVAL;   // (the scans count in int)
    if (!dev_keys) {
        for (size_t i = 0; i < n; ++i)
            if (key_off[i + 1] < key_off[i] || key_off[i + 1] - key_off[i] >= (1ull << 32)) return KVR_EINVAL;
        if (key_off[n] && !keys) return KVR_EINVAL;
    } else if (!keys) {
        return KVR_EINVAL;
    }
    if (!c->g_ev[0])
        for (auto &e : c->g_ev) HIPCHK(hipEventCreate(&e));
    if (c->g_tot.ensure(5) || c->g_vlen.ensure(n + 1) || c->g_src.ensure(n) || (!dev_out && c->g_idx.ensure(n)) ||
        (!dev_out && c->g_off.ensure(n + 1)) || (verify && (c->g_nch.ensure(n + 1) || c->g_cpre.ensure(n + 1))))
        return KVR_ENOMEM;
    const uint8_t *d_keys = keys;
    const uint64_t *d_koff = key_off;
    if (!dev_keys) {
        const uint64_t kb = key_off[n];
        if (c->g_keys.ensure(kb + 1) || c->g_koff.ensure(n + 1)) return KVR_ENOMEM;
        if (kb) HIPCHK(hipMemcpyAsync(c->g_keys.p, keys, kb, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(c->g_koff.p, key_off, (n + 1) * 8, hipMemcpyHostToDevice, st));
        d_keys = c->g_keys.p;
        d_koff = c->g_koff.p;
    }
    int64_t *d_idx = dev_out ? live_idx : c->g_idx.p;
    uint64_t *d_off = dev_out ? val_off : c->g_off.p;
    unsigned long long *d_tot = reinterpret_cast<unsigned long long *>(c->g_tot.p);
    const uint32_t g = (uint32_t)((n + GET_T - 1) / GET_T), g1 = (uint32_t)((n + GET_T) / GET_T);
    size_t tb = 0;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, c->g_vlen.p, d_off, (int)(n + 1), st));
    if (c->g_tmp.n < tb && c->g_tmp.ensure(tb)) return KVR_ENOMEM;

    // 1. probe, offsets, totals
    HIPCHK(hipMemsetAsync(c->g_tot.p, 0, 5 * 8, st));
    HIPCHK(hipMemsetAsync(c->g_vlen.p + n, 0, 8, st));
    HIPCHK(hipEventRecord(c->g_ev[0], st));
    hipLaunchKernelGGL(k_get_probe, dim3(g), dim3(GET_T), 0, st, d_keys, d_koff, (uint64_t)n, c->lout.p, c->ix_live,
                       c->islots.p, c->ix_slots, c->segs.p, d_idx, c->g_vlen.p, c->g_src.p, d_tot);
    HIPCHK(hipGetLastError());
    tb = c->g_tmp.n;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(c->g_tmp.p, tb, c->g_vlen.p, d_off, (int)(n + 1), st));
    if (verify) {
        hipLaunchKernelGGL(k_get_nch, dim3(g1), dim3(GET_T), 0, st, c->g_vlen.p, (uint64_t)n, c->g_nch.p);
        tb = c->g_tmp.n;
        HIPCHK(hipcub::DeviceScan::ExclusiveSum(c->g_tmp.p, tb, c->g_nch.p, c->g_cpre.p, (int)(n + 1), st));
    }
    hipLaunchKernelGGL(k_get_totals, dim3(1), dim3(64), 0, st, d_off, verify ? c->g_cpre.p : (const uint64_t *)nullptr,
                       (uint64_t)n, d_tot);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->g_ev[1], st));
    uint64_t tot[5] = {};
    HIPCHK(hipMemcpyAsync(tot, c->g_tot.p, sizeof(tot), hipMemcpyDeviceToHost, st));
    if (!dev_out) {
        HIPCHK(hipMemcpyAsync(live_idx, d_idx, n * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(val_off, d_off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    c->gstats.ms_probe = ev_ms(c->g_ev[0], c->g_ev[1]);
    c->gstats.n_keys = n;
    if (tot[4]) return KVR_EINVAL;   // device key_off: decreasing, or a key of 2^32 bytes or more
    const uint64_t total = tot[0], nch = tot[2];
    *val_bytes = total;
    c->gstats.n_found = tot[3];
    c->gstats.val_bytes = total;
    if (locate) return KVR_OK;
    if (total > vals_cap) return KVR_CAPACITY;
    if (verify && (nch >= 0xFFFFFFFFull || total >= (1ull << 48))) return KVR_EINVAL;   // (k_etag_map's descriptors)

    // 2. gather: value i to vals[val_off[i] ..), clipped at the output's capacity
    HIPCHK(hipEventRecord(c->g_ev[2], st));
    // (straight into a device output when it is 8-B aligned, as kvr_compact's; else through staging)
    const bool direct = dev_out && !(reinterpret_cast<uintptr_t>(vals) & 7u);
    uint8_t *d_vals = vals;
    uint64_t d_cap = vals_cap;
    if (!direct) {
        if (c->g_vals.ensure(total + 16)) return KVR_ENOMEM;
        d_vals = c->g_vals.p;
        d_cap = total;
    }
    if (total)
        hipLaunchKernelGGL(k_gather_r, dim3((uint32_t)c->n_cu * 16), dim3(CT_GATHER), 0, st, c->g_src.p, d_off, c->g_tot.p,
                           d_vals, d_cap);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->g_ev[3], st));

    // 3. verify on read: CRC-32 of every gathered value against its tuple's
    uint64_t fails = 0;
    if (verify) {
        if (c->g_exp.ensure(n) || c->g_crc.ensure(n) || (bad && !dev_out && c->g_bad.ensure(n))) return KVR_ENOMEM;
        hipLaunchKernelGGL(k_get_expected, dim3(g), dim3(GET_T), 0, st, c->lout.p, d_idx, (uint64_t)n, c->g_exp.p);
        HIPCHK(hipGetLastError());
        const int rc = etag_launch(c, d_vals, total, d_off, c->g_vlen.p, c->g_cpre.p, n, nch, c->g_exp.p, c->g_crc.p);
        if (rc != KVR_OK) return rc;
        uint8_t *d_bad = !bad ? nullptr : dev_out ? bad : c->g_bad.p;
        if (d_bad) {
            hipLaunchKernelGGL(k_get_bad, dim3(g), dim3(GET_T), 0, st, c->g_crc.p, c->g_exp.p, (uint64_t)n, d_bad);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(c->g_ev[4], st));
        HIPCHK(hipMemcpyAsync(&fails, c->e_fail.p, 8, hipMemcpyDeviceToHost, st));
        if (bad && !dev_out) HIPCHK(hipMemcpyAsync(bad, d_bad, n, hipMemcpyDeviceToHost, st));
    }
    if (!direct && total)
        HIPCHK(hipMemcpyAsync(vals, d_vals, total, dev_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    c->gstats.ms_gather = ev_ms(c->g_ev[2], c->g_ev[3]);
    if (verify) c->gstats.ms_verify = ev_ms(c->g_ev[3], c->g_ev[4]);
    c->gstats.n_crc_fail = fails;
    if (n_crc_fail) *n_crc_fail = fails;
    return KVR_OK;
}

}  // extern "C"
