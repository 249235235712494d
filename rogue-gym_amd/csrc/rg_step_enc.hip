// rg_step_enc.hip -- k_step_enc: the step kernel of the headline class, compiled for that class alone (gfx950).  A library of its own
// (librogue_gym_stepenc.so, which librogue_gym_hip.so links: units.sh), as the fix-up pass, the novelty pass and the cell archive are: the kernel set and the
// register counts the resource tests pin in the other code objects stay what they are, k_step_w32<false, true>'s among them.
//
// The kernel is k_step_w32<false, true> (rg_kernels.hip) -- stair blocks, index-order blocks, helper blocks, one call site of step_wave<0, 0, false, true>, the
// same RgState fields, LDS layout and launch arguments -- with the grid a compile-time constant: 32 columns, 16 rows, 512 cells.  The turn code is not copied:
// this unit includes rg_kernels.hip, which keeps its own kernels and launchers out of it (RG_STEP_ENC_UNIT).  The room count stays a run-time value (fixed, it
// unrolls the slot loops).  rgk_step (rg_kernels.hip) launches it where rgk_step_enc_capable holds for the config and rgk_step_enc_takes for the launch (it pre-streams the gray images: S->enc_out);
// every other launch is what it was.  What the constants are worth in the built code and on the GPU: profiles/r13_experiments.txt.
#define RG_STEP_ENC_UNIT
#define STEP_ENC_W 32
#define STEP_ENC_H 16
#define RG_GRID_W(c) STEP_ENC_W  // (rg_device.h: what the turn code reads for c.width and c.height)
#define RG_GRID_H(c) STEP_ENC_H
#include "rg_kernels.hip"

__global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_step_enc(RgState S, const RgState *__restrict__ SPd, RgConfig c, const uint8_t *__restrict__ keys, int use_spares, int stage_off, int epw, int parity) {
    // the class: the values rgk_step_enc_capable checked on the host, here as constants the turn code folds
    S.hw = STEP_ENC_W * STEP_ENC_H;  // (S is this kernel's own copy of the argument; c.width and c.height: RG_GRID_W, RG_GRID_H)
    // ... and the state of the launch that rgk_step_enc_takes checked: the arrays every handle that pre-streams has, spares in use, stair blocks at the front
    // of the grid, no kept spares, and neither of the two diagnostic services -- a handle with the action history (rg_history_enable) or the wave profile
    // (rg_prof) switched on stays on the generic instance.  The profile's marks are not free where nobody reads them: Prof's clock words are scalar
    // registers held through the whole turn, and every mark ends a basic block (profiles/r13_experiments.txt: +1.0 % on `value` without them).
    __builtin_assume(S.ovl != nullptr);
    __builtin_assume(S.obs_rec != nullptr);
    __builtin_assume(S.nx_state != nullptr);
    __builtin_assume(S.enc_out != nullptr);
    __builtin_assume(S.stats != nullptr);
    __builtin_assume(parity >= 0);
    use_spares = 1;
    S.keep_spares = 0;
    S.klog = nullptr;
#ifndef STEP_ENC_PROF  // (a variant build with -DSTEP_ENC_PROF keeps the marks: tools/microbench.py prof1 on this kernel)
    S.prof = nullptr;
#endif
    const int first_helper = (int)gridDim.x - S.enc_helpers;
    if ((int)blockIdx.x >= first_helper) { enc_helper(S, (int)blockIdx.x - first_helper, S.enc_helpers); return; }
    RG_STEP_BLOCK_BODY(0, 0, false, true)
}
#undef RG_STEP_BLOCK_BODY

// ---------------------------------------------------------------------------------------------
#include "rg_launch.h"  // host-callable launchers: defined here against the prototypes the host units call them by
// ---------------------------------------------------------------------------------------------
#ifndef RG_BUILD_ID
#define RG_BUILD_ID "unstamped"
#endif
extern "C" {
// the build id of this library, readable from the file as librogue_gym_hip.so's is (rg_api.cpp rg_build_id)
const char *rgk_step_enc_build_id(void) { static const char id[] = "RGBUILDID:" RG_BUILD_ID; return id + 10; }
// the class the kernel is compiled for: the capped W <= 32 class with the 32-room generator (rgk_step's own test) on a grid of exactly 32 x 16 cells.  A 16 x 32
// grid has 512 cells too and stays on the generic instance.
int rgk_step_enc_capable(const RgConfig *c) {
    const int nr = c->room_num_x * c->room_num_y;
    return (c->width == STEP_ENC_W && c->height == STEP_ENC_H && nr >= 1 && nr <= 32) ? 1 : 0;
}
// the launches of the class this kernel takes: what its text assumes about the handle's state (k_step_enc, above).  Everything else of the class -- a handle
// without spares or next-level structures, kept spares, no stair blocks, the action history or the wave profile switched on -- is the generic instance's.
int rgk_step_enc_takes(const RgState *S, int use_spares, int parity) {
#ifndef STEP_ENC_PROF
    if (S->prof) return 0;
#endif
    return (S->enc_out && S->ovl && S->obs_rec && S->nx_state && S->stats && !S->klog && !S->keep_spares && use_spares == 1 && parity >= 0) ? 1 : 0;
}
// rgk_step's launch of the pre-streaming instance, under another kernel: the grid, the LDS size and every argument are rgk_step's
void rgk_step_enc(const RgState *S, const RgState *SP_dev, const RgConfig *c, const uint8_t *keys, int use_spares, int stage_off, int epw, int parity, int blocks, size_t smem,
                  hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    rg_launch(k_step_enc, dim3(blocks), dim3(WAVE), smem, st, ev0, ev1, *S, SP_dev, *c, keys, use_spares, stage_off, epw, parity);
}
}
