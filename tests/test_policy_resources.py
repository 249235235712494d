"""The budget of the built action kernel (rogue-gym_amd/csrc/rg_policy.hip), read from the code object inside librogue_gym_policy.so (a library of its own, which
librogue_gym_hip.so links): exactly the three k_act instances and nothing else, no scratch, no spills, no AGPRs, k_action_mask's register bound -- and the
product and the development library find the new library beside them."""
import os
import subprocess

import test_kernel_resources as tkr
from test_novelty_resources import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rogue-gym_amd")
POL_SO = os.path.join(PKG, "librogue_gym_policy.so")
DEV_SO = os.path.join(PKG, "variants", "librogue_gym_hip_dev.so")
OTHERS = [os.path.join(PKG, "librogue_gym_%s.so" % n) for n in ("hip", "novelty", "archive", "obsfix", "stepenc")]


def test_budget_of_the_action_kernel():
    md = kernel_metadata(POL_SO)
    want = ["k_actILi%dEE" % dt for dt in (0, 1, 2)]   # RG_OBS_F32, RG_OBS_F16, RG_OBS_BF16
    assert len(md) == len(want), sorted(md)            # nothing else lives in this library
    for tag in want:
        hit = [k for k in md if tag in k]
        assert len(hit) == 1, (tag, sorted(md))
        m = md[hit[0]]
        print(hit[0], m)
        assert m["private_segment_fixed_size"] == 0, (hit[0], m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (hit[0], m)
        assert m["agpr_count"] == 0, (hit[0], m)
        assert m["vgpr_count"] <= 128, (hit[0], m)     # the bound k_action_mask carries
        for other in ("k_step", "k_obs", "k_path", "k_route", "k_regen", "k_crop_typed", "k_action_mask", "k_episode", "k_monsters", "k_objects", "k_pixels", "k_nov_"):
            assert other not in hit[0], (hit[0], other)
    for so in OTHERS:                                  # ... and the kernel nowhere else
        assert not [k for k in kernel_metadata(so) if "k_act" in k and "k_action_mask" not in k], so


def test_the_policy_library_is_built_from_the_checked_out_sources_and_found_beside_the_main_one():
    import __graft_entry__ as g
    g.build()
    assert g.library_id(POL_SO) == g.source_id()
    readelf = os.path.join(tkr.LLVM, "llvm-readelf")
    if os.path.exists(readelf):
        dyn = subprocess.run([readelf, "-d", tkr.SO], check=True, capture_output=True, text=True).stdout
        assert "librogue_gym_policy.so" in dyn and "$ORIGIN" in dyn, dyn
        dyn = subprocess.run([readelf, "-d", DEV_SO], check=True, capture_output=True, text=True).stdout
        assert "librogue_gym_policy.so" in dyn and "$ORIGIN/.." in dyn, dyn


def test_every_build_path_makes_and_links_the_policy_library():
    csrc = os.path.join(PKG, "csrc")
    assert 'POLICY_UNITS="rg_policy.hip:-O3"' in open(os.path.join(csrc, "units.sh")).read()
    for f in (os.path.join(csrc, "build.sh"), os.path.join(ROOT, "__graft_entry__.py")):
        text = open(f).read()
        assert "POLICY_UNITS" in text and "rogue_gym_policy" in text, f
    assert "-lrogue_gym_policy" in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()   # (a variant links the product's own policy library)


def test_the_policy_sources_read_no_environment_variable():
    csrc = os.path.join(PKG, "csrc")
    for f in ("rg_policy.h", "rg_policy.hip"):
        assert "getenv" not in open(os.path.join(csrc, f)).read(), f
    unit = open(os.path.join(csrc, "rg_api_readers.cpp")).read()
    assert "rg_act_host" in unit and "getenv" not in unit and "RG_DEV_ENV" not in unit
