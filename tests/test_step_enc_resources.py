"""The budget of the headline class's step kernel (rogue-gym_amd/csrc/rg_step_enc.hip), read from the code object inside librogue_gym_stepenc.so (a library of its
own, which both main libraries link): exactly one kernel lives there, k_step_enc, at 256 registers or fewer (two step waves per SIMD; built: 234), without
AGPRs, register spills to memory or scratch, and with fewer scalar-register spills than the generic instance it stands in for -- and the library carries the
build id of the checked-out sources, is found beside the main ones, comes from the one unit list, and its class test says what the dispatch needs it to."""
import ctypes as C
import os
import subprocess

import test_kernel_resources as tkr
from test_novelty_resources import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rogue-gym_amd", "csrc")
ENC_SO = os.path.join(ROOT, "rogue-gym_amd", "librogue_gym_stepenc.so")
DEV_SO = os.path.join(ROOT, "rogue-gym_amd", "variants", "librogue_gym_hip_dev.so")
GENERIC = "_Z10k_step_w32ILb0ELb1EEv7RgStatePKS0_8RgConfigPKhiiii"   # k_step_w32<false, true>


def test_one_kernel_and_its_budget():
    md = kernel_metadata(ENC_SO)
    assert len(md) == 1 and "k_step_enc" in list(md)[0], sorted(md)   # nothing else lives in this library: rg_kernels.hip keeps its own kernels out of the unit
    main = kernel_metadata(tkr.SO)
    assert not [k for k in main if "k_step_enc" in k]   # ... and the kernel nowhere else
    assert GENERIC in main   # the generic instance stays compiled: every other launch that pre-streams is still its
    (name, m), = md.items()
    print(name, m, "generic:", main[GENERIC])
    assert m["vgpr_count"] <= 256 and m["agpr_count"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, ("scratch memory", m)
    assert m["sgpr_spill_count"] < main[GENERIC]["sgpr_spill_count"], (m, main[GENERIC])   # (built: 517 against 694)


def test_the_library_is_built_from_the_checked_out_sources_and_found_beside_the_main_ones():
    import __graft_entry__ as g
    g.build()
    assert g.library_id(ENC_SO) == g.source_id()
    readelf = os.path.join(tkr.LLVM, "llvm-readelf")
    if os.path.exists(readelf):
        dyn = subprocess.run([readelf, "-d", tkr.SO], check=True, capture_output=True, text=True).stdout
        assert "librogue_gym_stepenc.so" in dyn and "$ORIGIN" in dyn, dyn
        dyn = subprocess.run([readelf, "-d", DEV_SO], check=True, capture_output=True, text=True).stdout
        assert "librogue_gym_stepenc.so" in dyn and "$ORIGIN/.." in dyn, dyn


def test_one_unit_list_builds_the_library():
    assert 'STEPENC_UNITS="rg_step_enc.hip:-O3"' in open(os.path.join(CSRC, "units.sh")).read()
    for f in (os.path.join(CSRC, "build.sh"), os.path.join(ROOT, "__graft_entry__.py"), os.path.join(ROOT, "tools", "build_variant.sh")):
        assert "STEPENC_UNITS" in open(f).read(), f
    # the turn code is one text: the unit includes rg_kernels.hip, defines one kernel and no device function of its own, and reads no environment variable
    unit = open(os.path.join(CSRC, "rg_step_enc.hip")).read()
    assert "#define RG_STEP_ENC_UNIT" in unit and '#include "rg_kernels.hip"' in unit
    assert unit.count("__global__") == 1 and "__device__" not in unit
    assert "getenv" not in unit and "RG_DEV_ENV" not in unit


def _config(width, height, rooms_x, rooms_y):
    """An RgConfig (csrc/rg_config.h) with the four fields the class test reads: width, height at words 0 and 1, room_num_x, room_num_y at words 3 and 4."""
    words = (C.c_int32 * 1024)()
    words[0], words[1], words[3], words[4] = width, height, rooms_x, rooms_y
    return words


def test_the_class_the_kernel_is_compiled_for():
    import __graft_entry__ as g
    g.build()
    head = open(os.path.join(CSRC, "rg_config.h")).read()
    assert "    int32_t width, height;\n    int32_t hide_dungeon;\n    int32_t room_num_x, room_num_y," in head, "RgConfig no longer starts with the words _config fills"
    f = C.CDLL(ENC_SO).rgk_step_enc_capable
    f.restype = C.c_int
    f.argtypes = [C.c_void_p]
    assert f(_config(32, 16, 2, 2)) == 1     # the mini dungeon
    assert f(_config(32, 16, 8, 4)) == 1     # 32 rooms: the room count is a run-time value of the kernel
    assert f(_config(16, 32, 2, 2)) == 0     # 512 cells, but 16 columns of 32 rows
    assert f(_config(32, 20, 2, 2)) == 0
    assert f(_config(80, 24, 3, 3)) == 0     # the default dungeon
    assert f(_config(32, 16, 11, 3)) == 0    # 33 rooms: the 64-room generator's class
