// rg_state_io.h -- layout of a STATE RECORD: one env's running game as a fixed-size, position-independent byte string (rg_state_save / rg_state_load,
// include/rogue_gym_hip.h).  The host computes the layout (rg_api_state.cpp state_layout); the kernels (rg_state_io.hip) take it as a kernel argument.
//
//   [0, 64)            header: u32 words {magic, RG_STATE_VERSION, R, H | W << 16, rooms, sections, fingerprint lo, fingerprint hi, klog cap, klog len, 0 ...}
//   o_cell             cell    u16 [H*W]
//   o_screen, o_hist   screen / history mirrors u8 [H*W]
//   o_dcmap            dist maps u16 [RG_DIST_SLOTS][H*W]                     (configs with enemies; zero for a slot outside the cache's ring)
//   o_dcwalk           saved walkable masks u32 [RG_DIST_SLOTS][H][walk words]   (the partial-map grid class; zero for a slot without a saved mask)
//   o_status           status mirror i32 [10]
//   o_obsrec           observation record u32 [RG_OBS_REC_WORDS(rooms)]        (grids the fused observation pass handles)
//   o_words            the env's words of the SoA arrays, one u32 each (narrow fields zero-extended), in the order of the descriptor table
//   base               the running episode's key log: klog cap bytes (0 when logging is off), zero past the logged length
// Every section starts 16-byte aligned and its padding is zero, so equal states give equal bytes.
#pragma once
#include <cstdint>

#define RG_STATE_MAGIC 0x54534752u   // "RGST"
#define RG_STATE_VERSION 1u
#define RG_STATE_HDR_BYTES 64u
#define RG_STATE_PAD16(b) (((b) + 15u) & ~15u)
// klog length bit: the key log of this episode is incomplete (the record it was restored from did not hold all its keys, or was saved without a log);
// as a length it exceeds every capacity, so rg_history_keys reports the log as truncated
#define RG_KLOG_PARTIAL 0x80000000u

// header `sections` bits: the optional arrays the record carries (they follow from the config, except for development knobs)
#define RG_SEC_DCMAP 1u
#define RG_SEC_DCWALK 2u
#define RG_SEC_OBSREC 4u
#define RG_SEC_OVL 8u

// word descriptor (u64, one per word of the o_words section): the address of env 0's element in bits 0..55, log2 of its size in bits 56..57,
// RG_IO_DESC_FLAGS on the flag word (its handle-local bits are cleared on save).  Env e's element lies e elements further.
#define RG_IO_DESC_PTR_MASK ((1ull << 56) - 1ull)
#define RG_IO_DESC_LG_SHIFT 56
#define RG_IO_DESC_FLAGS (1ull << 58)
// word guard (u32, one per word; 0 = none): (index of the guard word + 1) | bit << RG_IO_GUARD_SHIFT -- the word is stored as 0 unless that bit of the guard
// word is set (the hp / exp of a dead monster's slot, the amount of an absent gold: stale values that are not state)
#define RG_IO_GUARD_SHIFT 24
// ring guard (a dist-cache key): (index of the dc_head word + 1) | slot << RG_IO_GUARD_SHIFT | RG_IO_GUARD_RING -- the word is stored as 0 unless the slot is one of
// the dc_len (the word after dc_head) slots of the FIFO ring that starts at dc_head: a slot outside the ring holds whatever an earlier episode left there
#define RG_IO_GUARD_RING 0x80000000u

struct RgIoLayout {
    uint32_t R;         // record bytes of this handle
    uint32_t base;      // bytes before the key-log section (= its offset): the part every record of a config must agree on
    uint32_t hw, H, W, rooms, sections;
    uint32_t o_cell, o_screen, o_hist, o_dcmap, o_dcwalk, o_status, o_obsrec, o_words;
    uint32_t b_dcmap, b_dcwalk, b_obsrec;
    uint32_t n_words;
    uint32_t klog_cap;  // this handle's key-log capacity (0: logging off)
    uint32_t fp_lo, fp_hi;  // config fingerprint
};
