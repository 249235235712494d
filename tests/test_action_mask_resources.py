"""The budget of k_action_mask (rogue-gym_amd/csrc/rg_action_mask.hip), read from the built code objects: no scratch, no spills, no AGPRs, the register
bound the typed-crop kernels carry -- and a name none of the existing resource tests counts by."""
import os
import re

from test_kernel_resources import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_action_mask_kernel_budget_and_name():
    md = kernel_metadata()
    src = open(os.path.join(ROOT, "rogue-gym_amd", "csrc", "rg_action_mask.hip")).read()
    defined = re.findall(r"__global__\s+void\s+(?:__launch_bounds__\(\w+\)\s+)?(\w+)\(", src)
    assert defined == ["k_action_mask"], defined  # one kernel, no template: one instance
    mine = [k for k in md if "k_action_mask" in k]
    assert len(mine) == len(defined), mine
    for k in mine:
        m = md[k]
        print(k, m)
        assert m["private_segment_fixed_size"] == 0, (k, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
        assert m["agpr_count"] == 0 and m["vgpr_count"] <= 128, (k, m)
        for part in ("k_obs", "k_step", "k_crop_typed", "k_regen"):
            assert part not in k, (k, part)
