// rg_rows.h -- a grid as bit rows, one row per lane, and the choice of kernel instance for a grid: what k_path (rg_path.hip) and k_route (rg_route.hip) share.
//
// Device code for those two translation units only.  Everything here is a static inline template, so each kernel keeps its own instantiations and
// the resource tests keep telling the two families apart; the step and observation kernels, whose register counts are pinned, do not see this file.
#pragma once
#include <type_traits>
#include "rg_device.h"

// one-lane DPP shifts (as rg_kernels.hip has them for itself).  Whole wave: lane i <- lane i -+ 1 ...
static __device__ __forceinline__ uint32_t wave_shr1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false); }  // lane i <- lane i-1
static __device__ __forceinline__ uint32_t wave_shl1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, false); }  // lane i <- lane i+1
// ... and inside a DPP row of 16 lanes, zeros shifted in at the row's ends (bound_ctrl): with H <= 16 a group IS a DPP row, and "no neighbour" is free
static __device__ __forceinline__ uint32_t row_shr1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true); }
static __device__ __forceinline__ uint32_t row_shl1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x101, 0xf, 0xf, true); }

// a grid row as WN 32-bit words, cell x = bit x & 31 of word x >> 5
template <int WN> struct Row { uint32_t w[WN]; };
template <int WN> static __device__ __forceinline__ Row<WN> r_zero() {
    Row<WN> r;
#pragma unroll
    for (int k = 0; k < WN; k++) r.w[k] = 0u;
    return r;
}
template <int WN> static __device__ __forceinline__ Row<WN> r_shl1(const Row<WN> &a) {  // cell x-1 -> x
    Row<WN> r;
#pragma unroll
    for (int k = 0; k < WN; k++) r.w[k] = (a.w[k] << 1) | (k > 0 ? a.w[k > 0 ? k - 1 : 0] >> 31 : 0u);
    return r;
}
template <int WN> static __device__ __forceinline__ Row<WN> r_shr1(const Row<WN> &a) {  // cell x+1 -> x
    Row<WN> r;
#pragma unroll
    for (int k = 0; k < WN; k++) r.w[k] = (a.w[k] >> 1) | (k + 1 < WN ? a.w[k + 1 < WN ? k + 1 : k] << 31 : 0u);
    return r;
}
// the same masks of the row above (UP: lane - 1) or below; ROW16: a group is a DPP row, else a select keeps the groups (and the wave's ends) apart
template <int WN, bool ROW16, bool UP> static __device__ __forceinline__ Row<WN> r_neighbour(const Row<WN> &a, bool there) {
    Row<WN> r;
#pragma unroll
    for (int k = 0; k < WN; k++) {
        if (ROW16) r.w[k] = UP ? row_shr1(a.w[k]) : row_shl1(a.w[k]);
        else { const uint32_t v = UP ? wave_shr1(a.w[k]) : wave_shl1(a.w[k]); r.w[k] = there ? v : 0u; }
    }
    return r;
}
// the player's cell as (word, bit of that word); pw = -1: not in my row
struct Spot { int pw; uint32_t pb; };
template <int WN> static __device__ __forceinline__ bool r_at(const Row<WN> &a, const Spot &p) {  // is the spot's bit set in a?  (a select per word)
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < WN; k++) v |= p.pw == k ? a.w[k] : 0u;
    return (v & p.pb) != 0;
}
template <int WN> static __device__ __forceinline__ void r_put(Row<WN> &a, int x, bool v) {  // bit x of a = v: a select per word, never an indexed word
#pragma unroll
    for (int k = 0; k < WN; k++) a.w[k] = (a.w[k] & ~(((x >> 5) == k ? 1u : 0u) << (x & 31))) | (((x >> 5) == k && v ? 1u : 0u) << (x & 31));
}

// host side: the instance for a W x H grid.  f(wn, gs) gets the words per row (W <= RG_MAX_W = 160 = 5 words) and the lanes per env as
// std::integral_constants
template <class F> static void rows_dispatch(int W, int H, F f) {
    auto by_height = [&](auto wn) {
        if (H <= 16) f(wn, std::integral_constant<int, 16>());
        else if (H <= 32) f(wn, std::integral_constant<int, 32>());
        else f(wn, std::integral_constant<int, 64>());
    };
    if (W <= 32) by_height(std::integral_constant<int, 1>());
    else if (W <= 64) by_height(std::integral_constant<int, 2>());
    else if (W <= 96) by_height(std::integral_constant<int, 3>());
    else by_height(std::integral_constant<int, 5>());
}
