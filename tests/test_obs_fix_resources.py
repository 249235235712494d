"""The budget of the group-wise fix-up pass (rogue-gym_amd/csrc/rg_obs_fix.hip), read from the code object inside librogue_gym_obsfix.so (a library of its own,
which both main libraries link): exactly one kernel lives there, k_obs_fix, at 64 registers or fewer (eight waves per SIMD; built: 43), without AGPRs, spills
or scratch -- and the library carries the build id of the checked-out sources, is found beside the main one, comes from the one unit list, and its launcher
divides by the group the kernel was compiled for."""
import ctypes as C
import os
import re
import subprocess

import test_kernel_resources as tkr
from test_novelty_resources import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rogue-gym_amd", "csrc")
FIX_SO = os.path.join(ROOT, "rogue-gym_amd", "librogue_gym_obsfix.so")
DEV_SO = os.path.join(ROOT, "rogue-gym_amd", "variants", "librogue_gym_hip_dev.so")


def test_one_kernel_and_its_budget():
    md = kernel_metadata(FIX_SO)
    assert len(md) == 1 and "k_obs_fix" in list(md)[0], sorted(md)   # nothing else lives in this library
    assert not [k for k in kernel_metadata(tkr.SO) if "k_obs_fix" in k]   # ... and the kernel nowhere else
    (name, m), = md.items()
    print(name, m)
    assert m["vgpr_count"] <= 64 and m["agpr_count"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, ("scratch memory", m)


def test_the_library_is_built_from_the_checked_out_sources_and_found_beside_the_main_ones():
    import __graft_entry__ as g
    g.build()
    assert g.library_id(FIX_SO) == g.source_id()
    readelf = os.path.join(tkr.LLVM, "llvm-readelf")
    if os.path.exists(readelf):
        dyn = subprocess.run([readelf, "-d", tkr.SO], check=True, capture_output=True, text=True).stdout
        assert "librogue_gym_obsfix.so" in dyn and "$ORIGIN" in dyn, dyn
        dyn = subprocess.run([readelf, "-d", DEV_SO], check=True, capture_output=True, text=True).stdout
        assert "librogue_gym_obsfix.so" in dyn and "$ORIGIN/.." in dyn, dyn


def test_one_unit_list_builds_the_library():
    assert 'OBSFIX_UNITS="rg_obs_fix.hip:-Os"' in open(os.path.join(CSRC, "units.sh")).read()
    for f in (os.path.join(CSRC, "build.sh"), os.path.join(ROOT, "__graft_entry__.py"), os.path.join(ROOT, "tools", "build_variant.sh")):
        assert "OBSFIX_UNITS" in open(f).read(), f
    # the shared device code is one text: both units include it, neither keeps a copy
    for f in ("rg_obs.hip", "rg_obs_fix.hip"):
        text = open(os.path.join(CSRC, f)).read()
        assert '#include "rg_obs_dev.h"' in text and "define RG_OBS_REDRAW_ENV" not in text, f
    assert "define RG_OBS_REDRAW_ENV" in open(os.path.join(CSRC, "rg_obs_dev.h")).read()
    assert "getenv" not in open(os.path.join(CSRC, "rg_obs_fix.hip")).read()


def test_the_launcher_divides_by_the_group_of_the_source():
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    inner.load_library()   # (loads librogue_gym_obsfix.so with it)
    m = re.search(r"^#define OBS_FIX_GROUP (\d+)$", open(os.path.join(CSRC, "rg_obs_fix.hip")).read(), re.M)
    assert m, "OBS_FIX_GROUP is no longer a plain constant"
    group = int(m.group(1))
    assert group == 8   # (the sweep's choice, profiles/r12_experiments.txt; tests/test_gpu_obs_fix.py counts its groups by this)
    f = C.CDLL(FIX_SO).rgk_obs_fix_blocks
    f.restype = C.c_int
    f.argtypes = [C.c_int]
    for n in (1, 15, 16, 17, 82, 4160, 65536, 65537):
        assert f(n) == -(-n // group), (n, f(n))
    assert f(0) == 1   # an empty batch still launches a (guarded) block: a grid of 0 is a launch error
