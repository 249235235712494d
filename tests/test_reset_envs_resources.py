"""The kernels of the partial reset (rg_kernels.hip k_reset_compact / k_build_list), read from the built library like tests/test_kernel_resources.py (no
GPU needed): they are there, a list-driven build needs no more scratch memory and spills no more than k_build of the same generator instance in the
same library, and the compaction uses none."""
import re

from test_kernel_resources import kernel_metadata


def test_list_build_costs_no_more_than_k_build():
    md = kernel_metadata()
    for gm in (0, 1, 2):
        build = [k for k in md if re.search(r"7k_buildILi%dEE" % gm, k)]
        lst = [k for k in md if re.search(r"k_build_listILi%dEE" % gm, k)]
        assert len(build) == 1 and len(lst) == 1, (gm, sorted(md))
        b, m = md[build[0]], md[lst[0]]
        assert m["private_segment_fixed_size"] <= b["private_segment_fixed_size"], (lst[0], m, b)
        assert m["vgpr_spill_count"] <= b["vgpr_spill_count"] and m["sgpr_spill_count"] <= b["sgpr_spill_count"], (lst[0], m, b)
        assert m["agpr_count"] == 0, (lst[0], m)


def test_compaction_uses_no_scratch():
    md = kernel_metadata()
    ks = [k for k in md if "k_reset_compact" in k]
    assert len(ks) == 1, sorted(md)
    m = md[ks[0]]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (ks[0], m)
