"""The budget of the built episode kernels (rogue-gym_amd/csrc/rg_episode.hip), read from the code objects inside librogue_gym_hip.so: both instances exist,
no scratch, no spills, no AGPRs, few registers -- and no name that a resource test of another kernel family would count."""
from test_kernel_resources import kernel_metadata


def test_budget_of_both_episode_kernels():
    md = kernel_metadata()
    ep = {k: m for k, m in md.items() if "k_episode" in k}
    assert len(ep) == 2, sorted(ep)
    # built: 18 registers for the scalars-only instance, 51 with the scout bitmap (four 16-byte loads in flight per lane); a small margin on each
    for tag, bound in (("k_episodeILb0EE", 24), ("k_episodeILb1EE", 56)):
        hit = [k for k in ep if tag in k]
        assert len(hit) == 1, (tag, sorted(ep))
        print(hit[0], ep[hit[0]])
        assert ep[hit[0]]["vgpr_count"] <= bound, (hit[0], ep[hit[0]])
    for k, m in sorted(ep.items()):
        assert m["private_segment_fixed_size"] == 0, (k, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
        assert m["agpr_count"] == 0, (k, m)
        for other in ("k_step", "k_obs", "k_path", "k_route", "k_regen", "k_crop_typed", "k_action_mask"):
            assert other not in k, (k, other)
