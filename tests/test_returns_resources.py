"""The budget of the built returns kernels (rogue-gym_amd/csrc/rg_returns.hip), read from the code object inside librogue_gym_returns.so (a library of its own,
which librogue_gym_hip.so links): exactly the k_gae / k_vtrace instances the source names -- which optional arrays are present, which outputs -- and nothing
else, no scratch, no spills, no AGPRs, at most 128 VGPRs; no other library holds them, every build path makes and links the library, and the new sources read
no environment variable."""
import os
import subprocess

import test_kernel_resources as tkr
from test_novelty_resources import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rogue-gym_amd")
RETURNS_SO = os.path.join(PKG, "librogue_gym_returns.so")
DEV_SO = os.path.join(PKG, "variants", "librogue_gym_hip_dev.so")
OTHERS = [os.path.join(PKG, "librogue_gym_%s.so" % n) for n in ("hip", "novelty", "archive", "obsfix", "stepenc", "policy", "learn")]
VALUE, DONE, TRUNC, TV = 1, 2, 4, 8
ARRAYS = [0, DONE, TRUNC, DONE | TRUNC, TRUNC | TV, DONE | TRUNC | TV]       # (trunc_value needs trunc)


def test_budget_of_the_returns_kernels():
    import __graft_entry__ as g
    g.build()
    md = kernel_metadata(RETURNS_SO)
    # <arrays, outputs (1, 2, both), envs per lane (the product: 1)>; k_gae with and without its value row, k_vtrace always with it
    want = ["k_gaeILi%dELi%dELi1EE" % (f | v, o) for f in ARRAYS for v in (0, VALUE) for o in (1, 2, 3)]
    want += ["k_vtraceILi%dELi%dELi1EE" % (f, o) for f in ARRAYS for o in (1, 2, 3)]
    assert len(md) == len(want) == 54, sorted(md)         # nothing else lives in this library
    for tag in want:
        hit = [k for k in md if tag in k]
        assert len(hit) == 1, (tag, sorted(md))
        m = md[hit[0]]
        print(hit[0], m)
        assert m["private_segment_fixed_size"] == 0, (hit[0], m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (hit[0], m)
        assert m["agpr_count"] == 0, (hit[0], m)
        assert m["vgpr_count"] <= 128, (hit[0], m)
        assert m.get("group_segment_fixed_size", 0) == 0, (hit[0], m)     # a pipeline in registers: no LDS
    for so in OTHERS:                                     # ... and the kernels nowhere else
        assert not [k for k in kernel_metadata(so) if "k_gae" in k or "k_vtrace" in k], so


def test_the_returns_library_is_built_from_the_checked_out_sources_and_found_beside_the_main_one():
    import __graft_entry__ as g
    g.build()
    assert g.library_id(RETURNS_SO) == g.source_id()
    readelf = os.path.join(tkr.LLVM, "llvm-readelf")
    if os.path.exists(readelf):
        dyn = subprocess.run([readelf, "-d", tkr.SO], check=True, capture_output=True, text=True).stdout
        assert "librogue_gym_returns.so" in dyn and "$ORIGIN" in dyn, dyn
        dyn = subprocess.run([readelf, "-d", DEV_SO], check=True, capture_output=True, text=True).stdout
        assert "librogue_gym_returns.so" in dyn and "$ORIGIN/.." in dyn, dyn
        sym = subprocess.run([readelf, "--dyn-syms", "-W", RETURNS_SO], check=True, capture_output=True, text=True).stdout
        assert "rgk_returns_build_id" in sym and "rgk_gae" in sym and "rgk_vtrace" in sym
        # the main library refers to the launchers weakly: a build of the host units linked without this library still loads (tests/rule_mutants.py)
        und = [ln for ln in subprocess.run([readelf, "--dyn-syms", "-W", tkr.SO], check=True, capture_output=True, text=True).stdout.splitlines()
               if ln.split()[-1:] in (["rgk_gae"], ["rgk_vtrace"])]
        assert len(und) == 2 and all("WEAK" in ln and "UND" in ln for ln in und), und


def test_every_build_path_makes_and_links_the_returns_library():
    csrc = os.path.join(PKG, "csrc")
    units = open(os.path.join(csrc, "units.sh")).read()
    assert 'RETURNS_UNITS="rg_returns.hip:-O3"' in units
    for f in (os.path.join(csrc, "build.sh"), os.path.join(ROOT, "__graft_entry__.py")):
        text = open(f).read()
        assert "RETURNS_UNITS" in text and "rogue_gym_returns" in text, f
    assert "-lrogue_gym_returns" in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()   # (a variant links the product's own returns library)
    assert "librogue_gym_returns.so" in open(os.path.join(ROOT, "README.md")).read()


def test_the_returns_sources_read_no_environment_variable():
    csrc = os.path.join(PKG, "csrc")
    for f in ("rg_returns.h", "rg_returns.hip", "rg_api_learn.cpp"):
        text = open(os.path.join(csrc, f)).read()
        assert "getenv" not in text and "RG_DEV_ENV" not in text, f
    assert "rg_vtrace_host" in open(os.path.join(csrc, "rg_api_learn.cpp")).read()
