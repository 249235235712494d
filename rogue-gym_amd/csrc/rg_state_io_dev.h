// rg_state_io_dev.h -- the device side of writing ONE state record (rg_state_io.h), shared by the units that write records: rg_state_io.hip (rg_state_save /
// rg_state_load) and rg_archive.hip (the archive's record writers, librogue_gym_archive.so).  The io_* helpers, and the per-record bodies of the two save
// kernels: io_rec_save is what one WAVE does for one record, io_words_save what one WORKGROUP does for up to IO_WPB records.  Device only; include behind
// rg_device.h.
#pragma once
#include "rg_state_io.h"

#define IO_RPB 4     // records per block of the record kernels (a wave each)
#define IO_WPB 64    // records per block of the word kernels
#define IO_CH 64     // words per LDS pass of the word kernels
#define IO_THREADS 256

// env of record r: ids[r] (or r), -1 if out of range (device-side ids are the caller's to get right; a wrong one must still not write out of bounds)
__device__ __forceinline__ int io_env(const int32_t *ids, int r, int n) {
    const int e = ids ? ids[r] : r;
    return (e >= 0 && e < n) ? e : -1;
}

// `bytes` from src to dst by one wave, with the widest access both addresses allow; dst[bytes, pad_to) is zeroed (the record's padding on save)
__device__ __forceinline__ void io_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t bytes, uint32_t pad_to, int lane) {
    const uintptr_t al = (uintptr_t)dst | (uintptr_t)src;
    uint32_t done = 0;
    if ((al & 15) == 0) {
        const uint32_t n16 = bytes >> 4;
        for (uint32_t i = lane; i < n16; i += WAVE) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src)[i];
        done = n16 << 4;
    } else if ((al & 3) == 0) {
        const uint32_t n4 = bytes >> 2;
        for (uint32_t i = lane; i < n4; i += WAVE) reinterpret_cast<uint32_t *>(dst)[i] = reinterpret_cast<const uint32_t *>(src)[i];
        done = n4 << 2;
    }
    for (uint32_t i = done + lane; i < bytes; i += WAVE) dst[i] = src[i];
    for (uint32_t i = bytes + lane; i < pad_to; i += WAVE) dst[i] = 0;
}

// the dist cache's slot sections, slot by slot: a slot that holds no state (`live` bit clear) is written as zeros, whatever an earlier episode left in it
__device__ __forceinline__ void io_copy_slots(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t bytes, uint32_t live, int lane) {
    const uint32_t sb = bytes / RG_DIST_SLOTS;
    for (uint32_t s = 0; s < RG_DIST_SLOTS; s++) {
        if ((live >> s) & 1u) io_copy(dst + s * sb, src + s * sb, sb, sb, lane);
        else if (((uintptr_t)(dst + s * sb) & 15) == 0) {
            for (uint32_t i = lane; i < (sb >> 4); i += WAVE) reinterpret_cast<uint4 *>(dst + s * sb)[i] = make_uint4(0, 0, 0, 0);
            for (uint32_t i = (sb & ~15u) + lane; i < sb; i += WAVE) dst[s * sb + i] = 0;
        } else io_copy(dst + s * sb, src, 0, sb, lane);
    }
    for (uint32_t i = bytes + lane; i < RG_STATE_PAD16(bytes); i += WAVE) dst[i] = 0;
}

__device__ __forceinline__ uint32_t io_ld(uint64_t d, int e) {
    const uintptr_t p = (uintptr_t)(d & RG_IO_DESC_PTR_MASK);
    const uint32_t lg = (uint32_t)(d >> RG_IO_DESC_LG_SHIFT) & 3u;
    if (lg == 2) return reinterpret_cast<const uint32_t *>(p)[e];
    if (lg == 1) return reinterpret_cast<const uint16_t *>(p)[e];
    return reinterpret_cast<const uint8_t *>(p)[e];
}
__device__ __forceinline__ void io_st(uint64_t d, int e, uint32_t v) {
    const uintptr_t p = (uintptr_t)(d & RG_IO_DESC_PTR_MASK);
    const uint32_t lg = (uint32_t)(d >> RG_IO_DESC_LG_SHIFT) & 3u;
    if (lg == 2) reinterpret_cast<uint32_t *>(p)[e] = v;
    else if (lg == 1) reinterpret_cast<uint16_t *>(p)[e] = (uint16_t)v;
    else reinterpret_cast<uint8_t *>(p)[e] = (uint8_t)v;
}

// ---- save: one record ----
// One wave writes env e's record at `rec`: header + the env-contiguous sections + the key log (the words of the SoA arrays: io_words_save)
__device__ __forceinline__ void io_rec_save(const RgState &S, const RgIoLayout &L, int e, uint8_t *__restrict__ rec, int lane) {
    uint32_t klen = RG_KLOG_PARTIAL, cur = 0;  // (a handle without a key log: the episode's keys are unknown)
    if (S.klog) { cur = S.klog_cur[e]; klen = S.klog_len[(size_t)cur * S.n + e]; }
    if (lane < 16) {
        const uint32_t hd[10] = {RG_STATE_MAGIC, RG_STATE_VERSION, L.R, L.H | (L.W << 16), L.rooms, L.sections, L.fp_lo, L.fp_hi, L.klog_cap, klen};
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 10; i++) v = lane == i ? hd[i] : v;
        reinterpret_cast<uint32_t *>(rec)[lane] = v;
    }
    const size_t hw = L.hw;
    io_copy(rec + L.o_cell, reinterpret_cast<const uint8_t *>(S.cell + (size_t)e * hw), L.hw * 2, RG_STATE_PAD16(L.hw * 2), lane);
    io_copy(rec + L.o_screen, S.screen + (size_t)e * hw, L.hw, RG_STATE_PAD16(L.hw), lane);
    io_copy(rec + L.o_hist, S.hist + (size_t)e * hw, L.hw, RG_STATE_PAD16(L.hw), lane);
    // (canonical records: only the slots of the dist cache's ring, and of those only the saved masks, are state -- a rebuilt env's cache is empty)
    uint32_t ring = 0;
    {
        const uint32_t head = S.dc_head[e], len = S.dc_len[e];
        for (uint32_t s = 0; s < RG_DIST_SLOTS; s++) ring |= ((s >= head ? s - head : s + RG_DIST_SLOTS - head) < len ? 1u : 0u) << s;
    }
    if (L.sections & RG_SEC_DCMAP) io_copy_slots(rec + L.o_dcmap, reinterpret_cast<const uint8_t *>(S.dc_map) + (size_t)e * L.b_dcmap, L.b_dcmap, ring, lane);
    if (L.sections & RG_SEC_DCWALK) io_copy_slots(rec + L.o_dcwalk, reinterpret_cast<const uint8_t *>(S.dc_walk) + (size_t)e * L.b_dcwalk, L.b_dcwalk, ring & S.dc_own[e], lane);
    io_copy(rec + L.o_status, reinterpret_cast<const uint8_t *>(S.status + (size_t)e * 10), 40, 48, lane);
    if (L.sections & RG_SEC_OBSREC) io_copy(rec + L.o_obsrec, reinterpret_cast<const uint8_t *>(S.obs_rec) + (size_t)e * L.b_obsrec, L.b_obsrec, RG_STATE_PAD16(L.b_obsrec), lane);
    for (uint32_t i = L.o_words + 4 * L.n_words + lane; i < L.base; i += WAVE) rec[i] = 0;  // (the word section's padding; the words: io_words_save)
    if (L.klog_cap) {
        const uint32_t nk = klen < L.klog_cap ? klen : L.klog_cap;
        io_copy(rec + L.base, S.klog + ((size_t)e * 2 + cur) * L.klog_cap, nk, RG_STATE_PAD16(L.klog_cap), lane);
    }
}

// One workgroup writes the word sections of up to IO_WPB records: env[l] is record l's env (-1: none), DST gives record l's first byte, the first nr
// records exist.  A field is read with lane = env and transposed through `tile` (LDS, [IO_WPB][IO_CH + 1]: odd row pitch, both the column writes and the
// row reads are conflict-free), so that the record side is written in whole record lines.  Every thread of the workgroup calls it, behind a barrier that
// made env[] visible.
template <class DST>
__device__ __forceinline__ void io_words_save(const RgIoLayout &L, const uint64_t *__restrict__ desc, const uint32_t *__restrict__ guard, uint32_t *tile, const int *env,
                                              uint32_t nr, const DST &dst, int t) {
    for (uint32_t c0 = 0; c0 < L.n_words; c0 += IO_CH) {
        const uint32_t cn = L.n_words - c0 < IO_CH ? L.n_words - c0 : IO_CH;
        for (uint32_t i = t; i < IO_WPB * cn; i += IO_THREADS) {  // one field per wave-row: lane = env
            const uint32_t w = i / IO_WPB, l = i % IO_WPB;
            const int e = env[l];
            uint32_t v = 0;
            if (e >= 0) {
                const uint64_t d = desc[c0 + w];
                v = io_ld(d, e);
                if (d & RG_IO_DESC_FLAGS) v &= ~(RG_FLAG_SCR_CHANGED | RG_FLAG_ERR_MASK);  // handle-local bits
                const uint32_t gd = guard[c0 + w];
                if (gd & RG_IO_GUARD_RING) {  // a dist-cache key outside the ring
                    const uint32_t head = io_ld(desc[(gd & 0xffffffu) - 1], e), len = io_ld(desc[gd & 0xffffffu], e), sl = (gd >> RG_IO_GUARD_SHIFT) & 15u;
                    if ((sl >= head ? sl - head : sl + RG_DIST_SLOTS - head) >= len) v = 0;
                } else if (gd && !((io_ld(desc[(gd & 0xffffffu) - 1], e) >> (gd >> RG_IO_GUARD_SHIFT)) & 1u)) v = 0;  // an empty slot's stale word
            }
            tile[l * (IO_CH + 1) + w] = v;
        }
        __syncthreads();
        for (uint32_t i = t; i < nr * cn; i += IO_THREADS) {  // record lines: consecutive threads, consecutive words of one record
            const uint32_t l = i / cn, w = i - l * cn;
            if (env[l] >= 0) reinterpret_cast<uint32_t *>(dst(l) + L.o_words)[c0 + w] = tile[l * (IO_CH + 1) + w];
        }
        __syncthreads();
    }
}
