"""The budget of the built learner kernels (rogue-gym_amd/csrc/rg_policy_grad.hip), read from the code object inside librogue_gym_learn.so (a library of its own,
which librogue_gym_hip.so links): exactly the six k_pg_eval / k_pg_grad instances and nothing else, no scratch, no spills, no AGPRs, k_action_mask's register
bound -- no other library holds them, every build path makes and links the library, and the new sources read no environment variable."""
import os
import subprocess

import test_kernel_resources as tkr
from test_novelty_resources import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rogue-gym_amd")
LEARN_SO = os.path.join(PKG, "librogue_gym_learn.so")
DEV_SO = os.path.join(PKG, "variants", "librogue_gym_hip_dev.so")
OTHERS = [os.path.join(PKG, "librogue_gym_%s.so" % n) for n in ("hip", "novelty", "archive", "obsfix", "stepenc", "policy")]


def test_budget_of_the_learner_kernels():
    import __graft_entry__ as g
    g.build()
    md = kernel_metadata(LEARN_SO)
    want = ["k_pg_%sILi%dEE" % (k, dt) for k in ("eval", "grad") for dt in (0, 1, 2)]   # RG_OBS_F32, RG_OBS_F16, RG_OBS_BF16
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
        for other in ("k_act", "k_step", "k_obs", "k_path", "k_route", "k_regen", "k_crop_typed", "k_episode", "k_monsters", "k_objects", "k_pixels", "k_nov_"):
            assert other not in hit[0], (hit[0], other)
    for so in OTHERS:                                  # ... and the kernels nowhere else
        assert not [k for k in kernel_metadata(so) if "k_pg_" in k], so


def test_the_learn_library_is_built_from_the_checked_out_sources_and_found_beside_the_main_one():
    import __graft_entry__ as g
    g.build()
    assert g.library_id(LEARN_SO) == g.source_id()
    readelf = os.path.join(tkr.LLVM, "llvm-readelf")
    if os.path.exists(readelf):
        dyn = subprocess.run([readelf, "-d", tkr.SO], check=True, capture_output=True, text=True).stdout
        assert "librogue_gym_learn.so" in dyn and "$ORIGIN" in dyn, dyn
        dyn = subprocess.run([readelf, "-d", DEV_SO], check=True, capture_output=True, text=True).stdout
        assert "librogue_gym_learn.so" in dyn and "$ORIGIN/.." in dyn, dyn
        sym = subprocess.run([readelf, "--dyn-syms", "-W", LEARN_SO], check=True, capture_output=True, text=True).stdout
        assert "rgk_learn_build_id" in sym and "rgk_pg_eval" in sym and "rgk_pg_grad" in sym


def test_every_build_path_makes_and_links_the_learn_library():
    csrc = os.path.join(PKG, "csrc")
    units = open(os.path.join(csrc, "units.sh")).read()
    assert 'LEARN_UNITS="rg_policy_grad.hip:-O3"' in units and "rg_api_learn.cpp:-O2" in units
    for f in (os.path.join(csrc, "build.sh"), os.path.join(ROOT, "__graft_entry__.py")):
        text = open(f).read()
        assert "LEARN_UNITS" in text and "rogue_gym_learn" in text, f
    assert "-lrogue_gym_learn" in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()   # (a variant links the product's own learn library)
    assert "librogue_gym_learn.so" in open(os.path.join(ROOT, "README.md")).read()


def test_the_learner_sources_read_no_environment_variable():
    csrc = os.path.join(PKG, "csrc")
    for f in ("rg_policy_grad.h", "rg_policy_grad.hip", "rg_api_learn.cpp"):
        text = open(os.path.join(csrc, f)).read()
        assert "getenv" not in text and "RG_DEV_ENV" not in text, f
    assert "rg_policy_grad_host" in open(os.path.join(csrc, "rg_api_learn.cpp")).read()
