"""The budget of the built archive kernels (rogue-gym_amd/csrc/rg_archive.hip), read from the code object inside librogue_gym_archive.so (the pass is a library
of its own, which librogue_gym_hip.so links): exactly the archive kernels live there and nowhere else, no scratch, no spills, no AGPRs, register counts under
caps set from the built ones -- and the library carries the build id of the checked-out sources and is found beside the main one."""
import os

import test_kernel_resources as tkr
from test_novelty_resources import NOV_SO, kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARC_SO = os.path.join(ROOT, "rogue-gym_amd", "librogue_gym_archive.so")

# built: k_arc_offer 15, k_arc_bidders 14, k_arc_winners 12, k_arc_rec 100 (rg_state_save's k_state_rec_save: 100), k_arc_words 20 (k_state_words_save: 20),
# k_arc_gather 10, k_arc_chosen 4.  The caps: the small kernels far below what would cost a wave slot; the two record writers a margin of eight over the bodies
# they share with rg_state_save's kernels, still 4 waves per SIMD for the record writer (<= 128) and 8 for the rest (<= 64).
CAPS = {"k_arc_offer": 32, "k_arc_bidders": 32, "k_arc_winners": 32, "k_arc_rec": 108, "k_arc_words": 32, "k_arc_gather": 32, "k_arc_chosen": 32}


def test_budget_of_the_archive_kernels():
    md = kernel_metadata(ARC_SO)
    arc = {k: m for k, m in md.items() if "k_arc_" in k}
    assert set(arc) == set(md), sorted(set(md) - set(arc))   # nothing else lives in this library
    for so in (tkr.SO, NOV_SO):                              # ... and the archive nowhere else
        assert not [k for k in kernel_metadata(so) if "k_arc_" in k], so
    assert len(arc) == len(CAPS), sorted(arc)
    for tag, cap in CAPS.items():
        hit = [k for k in arc if tag in k]   # (no name is the beginning of another)
        assert len(hit) == 1, (tag, sorted(arc))
        print(hit[0], arc[hit[0]])
        assert arc[hit[0]]["vgpr_count"] <= cap, (hit[0], arc[hit[0]])
    for k, m in sorted(arc.items()):
        assert m["private_segment_fixed_size"] == 0, (k, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
        assert m["agpr_count"] == 0, (k, m)
        for other in ("k_step", "k_obs", "k_state_", "k_nov_", "k_path", "k_route", "k_regen", "k_crop_typed", "k_action_mask", "k_episode", "k_monsters", "k_objects", "k_pixels"):
            assert other not in k, (k, other)


def test_the_archive_library_is_built_from_the_checked_out_sources_and_found_beside_the_main_one():
    import subprocess
    import __graft_entry__ as g
    g.build()
    assert g.library_id(ARC_SO) == g.source_id()
    readelf = os.path.join(tkr.LLVM, "llvm-readelf")
    if os.path.exists(readelf):
        dyn = subprocess.run([readelf, "-d", tkr.SO], check=True, capture_output=True, text=True).stdout
        assert "librogue_gym_archive.so" in dyn and "$ORIGIN" in dyn, dyn
        dev = os.path.join(ROOT, "rogue-gym_amd", "variants", "librogue_gym_hip_dev.so")
        dyn = subprocess.run([readelf, "-d", dev], check=True, capture_output=True, text=True).stdout
        assert "librogue_gym_archive.so" in dyn and "$ORIGIN/.." in dyn, dyn


def test_one_unit_list_builds_the_archive_library():
    csrc = os.path.join(ROOT, "rogue-gym_amd", "csrc")
    assert 'ARCHIVE_UNITS="rg_archive.hip:-O3"' in open(os.path.join(csrc, "units.sh")).read()
    for f in (os.path.join(csrc, "build.sh"), os.path.join(ROOT, "__graft_entry__.py")):
        assert "ARCHIVE_UNITS" in open(f).read(), f
    assert "-lrogue_gym_archive" in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()


def test_the_archive_sources_read_no_environment_variable():
    csrc = os.path.join(ROOT, "rogue-gym_amd", "csrc")
    for f in ("rg_archive.h", "rg_archive.hip", "rg_state_io_dev.h", "rg_api_state.cpp"):
        text = open(os.path.join(csrc, f)).read()
        assert "getenv" not in text and "RG_DEV_ENV" not in text, f
    assert "rg_archive_offer_host" in open(os.path.join(csrc, "rg_api_state.cpp")).read()
    py = open(os.path.join(ROOT, "rogue-gym_amd", "rogue_gym", "envs", "device.py")).read()
    assert "archive_restore" in py and "environ" not in py and "getenv" not in py
