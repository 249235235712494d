"""The budget of the built route kernels (rogue-gym_amd/csrc/rg_route.hip), read from the code objects inside librogue_gym_hip.so: no scratch, no spills, no
AGPRs, at most 128 registers per instance -- and no name that a resource test of another kernel family would count."""
from test_kernel_resources import kernel_metadata


def test_budget_of_every_route_kernel():
    md = kernel_metadata()
    route = {k: m for k, m in md.items() if "k_route" in k}
    # per row-word count (1, 2, 3, 5) and group size (16, 32, 64 lanes); mode and goal words are run-time arguments
    assert len(route) == 12, sorted(route)
    for wn in (1, 2, 3, 5):
        for gs in (16, 32, 64):
            assert any("k_routeILi%dELi%dEE" % (wn, gs) in k for k in route), (wn, gs, sorted(route))
    for k, m in sorted(route.items()):
        print(k, m)
        assert m["private_segment_fixed_size"] == 0, (k, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
        assert m["agpr_count"] == 0, (k, m)
        assert m["vgpr_count"] <= 128, (k, m)
        for other in ("k_path", "k_obs", "k_step", "k_crop_typed", "k_regen", "k_action_mask"):
            assert other not in k, (k, other)
