"""The budget of the built object-table kernels (rogue-gym_amd/csrc/rg_objects.hip), read from the code objects inside librogue_gym_hip.so: no scratch, no
spills, no AGPRs, at most 128 registers per instance (four waves per SIMD) -- and no name that a resource test of another kernel family would count."""
from test_kernel_resources import kernel_metadata


def test_budget_of_every_objects_kernel():
    md = kernel_metadata()
    objs = {k: m for k, m in md.items() if "k_objects" in k}
    # per row-word count (1, 2, 3, 5) and group size (16, 32, 64 lanes); kinds, mode and cap are run-time arguments
    assert len(objs) == 12, sorted(objs)
    for wn in (1, 2, 3, 5):
        for gs in (16, 32, 64):
            assert any("k_objectsILi%dELi%dEE" % (wn, gs) in k for k in objs), (wn, gs, sorted(objs))
    for k, m in sorted(objs.items()):
        print(k, m)
        assert m["private_segment_fixed_size"] == 0, (k, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
        assert m["agpr_count"] == 0, (k, m)
        assert m["vgpr_count"] <= 128, (k, m)   # 512 / 128 = four waves per SIMD, the occupancy the kernel asks for
        for other in ("k_path", "k_route", "k_obs", "k_step", "k_crop_typed", "k_regen", "k_action_mask", "k_monsters", "k_episode"):
            assert other not in k, (k, other)
