"""The budget of the built novelty kernels (rogue-gym_amd/csrc/rg_novelty.hip), read from the code object inside librogue_gym_novelty.so (the pass is a library of its own, which librogue_gym_hip.so links): every instance exists,
no scratch, no spills, no AGPRs, few registers, no name that a resource test of another kernel family would count -- and the product
reads no environment variable it did not read before."""
import os

import test_kernel_resources as tkr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOV_SO = os.path.join(ROOT, "rogue-gym_amd", "librogue_gym_novelty.so")


def kernel_metadata(so):
    """test_kernel_resources.kernel_metadata() of another library."""
    keep, tkr.SO = tkr.SO, so
    try:
        return tkr.kernel_metadata()
    finally:
        tkr.SO = keep


def test_budget_of_the_novelty_kernels():
    md = kernel_metadata(NOV_SO)
    nov = {k: m for k, m in md.items() if "k_nov_" in k}
    assert set(nov) == set(md), sorted(set(md) - set(nov))   # nothing else lives in this library
    assert not [k for k in kernel_metadata(tkr.SO) if "k_nov_" in k]   # ... and the pass nowhere else
    # the hash for 16, 32 and 64 lanes per env, each with 16-byte loads and byte by byte; the insert with and without the POS hash; the read-back
    want = ["k_nov_hashILi%dELb%dEE" % (g, w) for g in (16, 32, 64) for w in (0, 1)] + ["k_nov_insertILb0EE", "k_nov_insertILb1EE", "k_nov_count"]
    assert len(nov) == len(want), sorted(nov)
    for tag in want:
        hit = [k for k in nov if tag in k]
        assert len(hit) == 1, (tag, sorted(nov))
        print(hit[0], nov[hit[0]])
        # built: 26 registers for the byte-wise hash, 17 for the wide one, 18 for the insert, 4 for the read-back; a margin on each, far below what would cost a wave slot
        assert nov[hit[0]]["vgpr_count"] <= 40, (hit[0], nov[hit[0]])
    for k, m in sorted(nov.items()):
        assert m["private_segment_fixed_size"] == 0, (k, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
        assert m["agpr_count"] == 0, (k, m)
        for other in ("k_step", "k_obs", "k_path", "k_route", "k_regen", "k_crop_typed", "k_action_mask", "k_episode", "k_monsters", "k_objects", "k_pixels"):
            assert other not in k, (k, other)


def test_the_novelty_library_is_built_from_the_checked_out_sources_and_found_beside_the_main_one():
    import subprocess
    import __graft_entry__ as g
    g.build()
    assert g.library_id(NOV_SO) == g.source_id()
    readelf = os.path.join(tkr.LLVM, "llvm-readelf")
    if os.path.exists(readelf):
        dyn = subprocess.run([readelf, "-d", tkr.SO], check=True, capture_output=True, text=True).stdout
        assert "librogue_gym_novelty.so" in dyn and "$ORIGIN" in dyn, dyn


def test_the_novelty_sources_read_no_environment_variable():
    csrc = os.path.join(ROOT, "rogue-gym_amd", "csrc")
    for f in ("rg_novelty.h", "rg_novelty.hip"):
        assert "getenv" not in open(os.path.join(csrc, f)).read(), f
    # the host unit of the entry points reads none either, anywhere in it; the product-wide list of knobs is tests/test_cabi_load.py's, which this change leaves as it is
    unit = open(os.path.join(csrc, "rg_api_episode.cpp")).read()
    assert "rg_novelty_clear" in unit and "getenv" not in unit and "RG_DEV_ENV" not in unit
    py = open(os.path.join(ROOT, "rogue-gym_amd", "rogue_gym", "envs", "device.py")).read()
    assert "environ" not in py and "getenv" not in py
