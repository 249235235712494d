"""The budget of the built pixel kernel (rogue-gym_amd/csrc/rg_pixels.hip), read from the code objects inside librogue_gym_hip.so: no scratch, no spills, at
most 128 registers (four waves per SIMD), an LDS request that lets 16 one-wave blocks reside on a CU for every shape the launcher serves -- and the code
objects of the other units where they were."""
import ctypes as C

import pytest

from test_kernel_resources import kernel_metadata

LDS_PER_CU = 160 * 1024
BLOCKS_PER_CU = 16   # one-wave blocks: four waves on each of the four SIMDs


def test_budget_of_every_pixels_kernel():
    md = kernel_metadata()
    px = {k: m for k, m in md.items() if "k_pixels" in k}
    assert len(px) == 1, sorted(px)   # channels, tile height, window and screen size are run-time arguments
    for k, m in sorted(px.items()):
        print(k, m)
        assert m["private_segment_fixed_size"] == 0, (k, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
        assert m["agpr_count"] == 0, (k, m)
        assert m["vgpr_count"] <= 128, (k, m)
        for other in ("k_path", "k_route", "k_obs", "k_step", "k_crop", "k_regen", "k_action_mask", "k_monsters", "k_episode", "k_objects"):
            assert other not in k, (k, other)


def test_lds_request_lets_four_waves_per_simd_reside():
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    f = inner.load_library().rgk_pixels_lds
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_int)] * 2
    shapes = [(16, 32), (17, 33), (24, 80), (33, 97), (48, 160)]
    windows = [(-1, 0), (0, 0), (5, 5), (1, 7), (47, 159), (12, 40)]
    unstaged = 0
    for H, W in shapes:
        for ry, rx in windows:
            for th in (8, 13, 16):
                for ch in (1, 3):
                    run, staged = C.c_int(0), C.c_int(0)
                    lds = f(H, W, th, ch, ry, rx, C.byref(run), C.byref(staged))
                    assert 0 < lds <= LDS_PER_CU // BLOCKS_PER_CU, (H, W, ry, rx, th, ch, lds)
                    assert 1 <= run.value <= 64
                    unstaged += not staged.value
                    hc, wc = (H, W) if ry < 0 else (2 * ry + 1, 2 * rx + 1)
                    assert run.value * ch * hc * th * wc < 1 << 30
    assert unstaged < len(shapes) * len(windows) * 6 // 4   # only the largest boxes go unstaged
    run, staged = C.c_int(0), C.c_int(0)
    assert f(16, 32, 8, 1, 5, 5, C.byref(run), C.byref(staged)) and staged.value == 1   # the training shape is staged


PINNED = {  # kernel-name fragment -> vgpr_count of the units this change does not touch, as built from the parent commit
    '_Z10k_monstersILi16EEv7MonView': 136,
    '_Z10k_monstersILi4EEv7MonView': 58,
    '_Z10k_monstersILi8EEv7MonView': 81,
    '_Z10k_step_w32ILb0ELb0EEv7RgStatePKS0_8RgConfigPKhiiii': 247,
    '_Z10k_step_w32ILb0ELb1EEv7RgStatePKS0_8RgConfigPKhiiii': 248,
    '_Z10k_step_w32ILb1ELb0EEv7RgStatePKS0_8RgConfigPKhiiii': 251,
    '_Z11k_obs_resid7RgState8RgConfigPf': 54,
    '_Z11k_obs_typedILi0ELi1EEvPKhS1_PKiPjS4_iiiijiiPDv4_j': 60,
    '_Z11k_obs_typedILi0ELi2EEvPKhS1_PKiPjS4_iiiijiiPDv4_j': 59,
    '_Z11k_obs_typedILi1ELi1EEvPKhS1_PKiPjS4_iiiijiiPDv4_j': 87,
    '_Z11k_obs_typedILi1ELi2EEvPKhS1_PKiPjS4_iiiijiiPDv4_j': 86,
    '_Z11k_obs_typedILi2ELi3EEvPKhS1_PKiPjS4_iiiijiiPDv4_j': 108,
    '_Z11k_step_huge7RgStatePKS_8RgConfigPKhiiii': 349,
    '_Z12k_build_listILi0EEv7RgState8RgConfigPKiPKjPh': 126,
    '_Z12k_build_listILi1EEv7RgState8RgConfigPKiPKjPh': 127,
    '_Z12k_build_listILi2EEv7RgState8RgConfigPKiPKjPh': 133,
    '_Z12k_crop_typedILi0ELi0EEvPKtPKiPKhS5_PjS3_iiii13CropTypedArgsPhPiS6_': 38,   # (the f32 crop: an instance of k_crop_typed since k_obs_crop was folded into it)
    '_Z12k_crop_typedILi0ELi1EEvPKtPKiPKhS5_PjS3_iiii13CropTypedArgsPhPiS6_': 40,
    '_Z12k_crop_typedILi0ELi2EEvPKtPKiPKhS5_PjS3_iiii13CropTypedArgsPhPiS6_': 40,
    '_Z12k_crop_typedILi1ELi0EEvPKtPKiPKhS5_PjS3_iiii13CropTypedArgsPhPiS6_': 44,
    '_Z12k_crop_typedILi1ELi1EEvPKtPKiPKhS5_PjS3_iiii13CropTypedArgsPhPiS6_': 46,
    '_Z12k_crop_typedILi1ELi2EEvPKtPKiPKhS5_PjS3_iiii13CropTypedArgsPhPiS6_': 46,
    '_Z12k_crop_typedILi2ELi3EEvPKtPKiPKhS5_PjS3_iiii13CropTypedArgsPhPiS6_': 44,
    '_Z12k_lanes_scanPKjiPjPi': 27,
    '_Z12k_obs_stream7RgState8RgConfigPfi': 61,
    '_Z12k_regen_gatePKjjPj': 4,
    '_Z12k_regen_huge7RgState8RgConfigiii': 107,
    '_Z13k_action_maskPKtPKjS0_PKiiiii8MaskKeysPhS6_mm': 36,
    '_Z13k_gather_keysPKhPKiPhi': 4,
    '_Z13k_probe_clockPyi': 8,
    '_Z13k_regen_lanes7RgState8RgConfigPKjPKiiiiiiiiPy': 117,
    '_Z14k_scatter_rowsPKhPhPKiii': 18,
    '_Z14k_state_stairs7RgState10RgIoLayoutPh': 10,
    '_Z15k_debug_descendILi0EEv7RgState8RgConfig': 149,
    '_Z15k_debug_descendILi1EEv7RgState8RgConfig': 150,
    '_Z15k_debug_descendILi2EEv7RgState8RgConfig': 159,
    '_Z15k_encode_scalarPKhS0_PKiPjS3_iimmiijiiPfS2_': 23,
    '_Z15k_reset_compactPKhiPiPj': 6,
    '_Z16k_state_rec_load7RgState10RgIoLayoutPKiiPKhjPhS5_': 70,
    '_Z16k_state_rec_save7RgState10RgIoLayoutPKiiPh': 100,
    '_Z18k_state_words_loadi10RgIoLayoutPKmPKjPKiiPKhjS7_': 18,
    '_Z18k_state_words_savei10RgIoLayoutPKmPKjPKiiPh': 20,
    '_Z5k_obsILi0ELb0ELb0EEv7RgState8RgConfigjiPfPjiiii': 79,
    '_Z5k_obsILi0ELb0ELb1EEv7RgState8RgConfigjiPfPjiiii': 81,
    '_Z5k_obsILi0ELb1ELb0EEv7RgState8RgConfigjiPfPjiiii': 80,
    '_Z5k_obsILi1ELb0ELb0EEv7RgState8RgConfigjiPfPjiiii': 94,
    '_Z5k_obsILi1ELb0ELb1EEv7RgState8RgConfigjiPfPjiiii': 95,
    '_Z5k_obsILi1ELb1ELb0EEv7RgState8RgConfigjiPfPjiiii': 102,
    '_Z6k_grayPKhS0_PKiiimmijiPfS2_': 49,
    '_Z6k_packPKhS0_PKiPKfPKjiiiPj': 17,
    '_Z6k_pathILi1ELi16ELb0EEvPKtPKjS1_PKiiiijS5_PtPiPh': 36,
    '_Z6k_pathILi1ELi16ELb1EEvPKtPKjS1_PKiiiijS5_PtPiPh': 37,
    '_Z6k_pathILi1ELi32ELb0EEvPKtPKjS1_PKiiiijS5_PtPiPh': 36,
    '_Z6k_pathILi1ELi32ELb1EEvPKtPKjS1_PKiiiijS5_PtPiPh': 47,
    '_Z6k_pathILi1ELi64ELb0EEvPKtPKjS1_PKiiiijS5_PtPiPh': 35,
    '_Z6k_pathILi1ELi64ELb1EEvPKtPKjS1_PKiiiijS5_PtPiPh': 46,
    '_Z6k_pathILi2ELi16ELb0EEvPKtPKjS1_PKiiiijS5_PtPiPh': 39,
    '_Z6k_pathILi2ELi16ELb1EEvPKtPKjS1_PKiiiijS5_PtPiPh': 67,
    '_Z6k_pathILi2ELi32ELb0EEvPKtPKjS1_PKiiiijS5_PtPiPh': 39,
    '_Z6k_pathILi2ELi32ELb1EEvPKtPKjS1_PKiiiijS5_PtPiPh': 64,
    '_Z6k_pathILi2ELi64ELb0EEvPKtPKjS1_PKiiiijS5_PtPiPh': 38,
    '_Z6k_pathILi2ELi64ELb1EEvPKtPKjS1_PKiiiijS5_PtPiPh': 63,
    '_Z6k_pathILi3ELi16ELb0EEvPKtPKjS1_PKiiiijS5_PtPiPh': 54,
    '_Z6k_pathILi3ELi16ELb1EEvPKtPKjS1_PKiiiijS5_PtPiPh': 93,
    '_Z6k_pathILi3ELi32ELb0EEvPKtPKjS1_PKiiiijS5_PtPiPh': 54,
    '_Z6k_pathILi3ELi32ELb1EEvPKtPKjS1_PKiiiijS5_PtPiPh': 93,
    '_Z6k_pathILi3ELi64ELb0EEvPKtPKjS1_PKiiiijS5_PtPiPh': 51,
    '_Z6k_pathILi3ELi64ELb1EEvPKtPKjS1_PKiiiijS5_PtPiPh': 92,
    '_Z6k_pathILi5ELi16ELb0EEvPKtPKjS1_PKiiiijS5_PtPiPh': 83,
    '_Z6k_pathILi5ELi16ELb1EEvPKtPKjS1_PKiiiijS5_PtPiPh': 100,
    '_Z6k_pathILi5ELi32ELb0EEvPKtPKjS1_PKiiiijS5_PtPiPh': 83,
    '_Z6k_pathILi5ELi32ELb1EEvPKtPKjS1_PKiiiijS5_PtPiPh': 100,
    '_Z6k_pathILi5ELi64ELb0EEvPKtPKjS1_PKiiiijS5_PtPiPh': 81,
    '_Z6k_pathILi5ELi64ELb1EEvPKtPKjS1_PKiiiijS5_PtPiPh': 99,
    '_Z6k_stepILi1ELb0EEv7RgStatePKS0_8RgConfigPKhiiii': 273,
    '_Z6k_stepILi2ELb0EEv7RgStatePKS0_8RgConfigPKhiiii': 301,
    '_Z6k_stepILi2ELb1EEv7RgStatePKS0_8RgConfigPKhiiii': 305,
    '_Z6k_stepILi3ELb0EEv7RgStatePKS0_8RgConfigPKhiiii': 290,
    '_Z6k_stepILi4ELb0EEv7RgStatePKS0_8RgConfigPKhiiii': 338,
    '_Z7k_buildILi0EEv7RgState8RgConfig': 130,
    '_Z7k_buildILi1EEv7RgState8RgConfig': 130,
    '_Z7k_buildILi2EEv7RgState8RgConfig': 110,
    '_Z7k_regenILi0EEv7RgState8RgConfigiii': 103,
    '_Z7k_regenILi1EEv7RgState8RgConfigiii': 104,
    '_Z7k_routeILi1ELi16EEvPKtPKjS1_PKiiiijjjS5_PiPhS7_': 45,
    '_Z7k_routeILi1ELi32EEvPKtPKjS1_PKiiiijjjS5_PiPhS7_': 45,
    '_Z7k_routeILi1ELi64EEvPKtPKjS1_PKiiiijjjS5_PiPhS7_': 44,
    '_Z7k_routeILi2ELi16EEvPKtPKjS1_PKiiiijjjS5_PiPhS7_': 50,
    '_Z7k_routeILi2ELi32EEvPKtPKjS1_PKiiiijjjS5_PiPhS7_': 50,
    '_Z7k_routeILi2ELi64EEvPKtPKjS1_PKiiiijjjS5_PiPhS7_': 49,
    '_Z7k_routeILi3ELi16EEvPKtPKjS1_PKiiiijjjS5_PiPhS7_': 66,
    '_Z7k_routeILi3ELi32EEvPKtPKjS1_PKiiiijjjS5_PiPhS7_': 66,
    '_Z7k_routeILi3ELi64EEvPKtPKjS1_PKiiiijjjS5_PiPhS7_': 64,
    '_Z7k_routeILi5ELi16EEvPKtPKjS1_PKiiiijjjS5_PiPhS7_': 100,
    '_Z7k_routeILi5ELi32EEvPKtPKjS1_PKiiiijjjS5_PiPhS7_': 100,
    '_Z7k_routeILi5ELi64EEvPKtPKjS1_PKiiiijjjS5_PiPhS7_': 98,
    '_Z8k_exportPKjS0_S0_S0_PjmmmS1_S1_S1_S1_S1_': 22,
    '_Z8k_redraw7RgState8RgConfig': 47,
    '_Z8k_render7RgState8RgConfig': 26,
    '_Z8k_symbolPKhS0_PKiPjS3_iimmiijiPfS2_': 50,
    '_Z9k_episodeILb0EEv6EpView9RgEpisode': 18,
    '_Z9k_episodeILb1EEv6EpView9RgEpisode': 51,
    '_Z9k_objectsILi1ELi16EEvPKtPKjS1_PKiiiijjiPDv4_jS7_': 48,
    '_Z9k_objectsILi1ELi32EEvPKtPKjS1_PKiiiijjiPDv4_jS7_': 48,
    '_Z9k_objectsILi1ELi64EEvPKtPKjS1_PKiiiijjiPDv4_jS7_': 46,
    '_Z9k_objectsILi2ELi16EEvPKtPKjS1_PKiiiijjiPDv4_jS7_': 60,
    '_Z9k_objectsILi2ELi32EEvPKtPKjS1_PKiiiijjiPDv4_jS7_': 60,
    '_Z9k_objectsILi2ELi64EEvPKtPKjS1_PKiiiijjiPDv4_jS7_': 58,
    '_Z9k_objectsILi3ELi16EEvPKtPKjS1_PKiiiijjiPDv4_jS7_': 72,
    '_Z9k_objectsILi3ELi32EEvPKtPKjS1_PKiiiijjiPDv4_jS7_': 73,
    '_Z9k_objectsILi3ELi64EEvPKtPKjS1_PKiiiijjiPDv4_jS7_': 71,
    '_Z9k_objectsILi5ELi16EEvPKtPKjS1_PKiiiijjiPDv4_jS7_': 101,
    '_Z9k_objectsILi5ELi32EEvPKtPKjS1_PKiiiijjiPDv4_jS7_': 102,
    '_Z9k_objectsILi5ELi64EEvPKtPKjS1_PKiiiijjiPDv4_jS7_': 100,
}


def test_register_counts_of_the_other_units_are_where_they_were():
    md = kernel_metadata()
    assert PINNED, "the pinned table is empty"
    for frag, want in PINNED.items():
        ks = [k for k in md if k == frag]
        assert len(ks) == 1, frag
        assert md[ks[0]]["vgpr_count"] == want, (frag, md[ks[0]], want)
    others = {k for k in md if "k_pixels" not in k}
    assert others == set(PINNED), sorted(others ^ set(PINNED))
