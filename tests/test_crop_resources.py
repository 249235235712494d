"""The f32 crop kernel (rg_crop_typed.hip k_crop_typed with RG_OBS_F32 elements: rg_obs_crop), read from the built library like
tests/test_kernel_resources.py (no GPU needed): both instances are there, and none uses scratch memory, spills or AGPRs."""
from test_kernel_resources import kernel_metadata


def test_crop_kernel_uses_no_scratch():
    md = kernel_metadata()
    ks = [k for k in md if "k_crop_typedILi0ELi0E" in k or "k_crop_typedILi1ELi0E" in k]
    assert len(ks) == 2, sorted(md)  # gray and one-hot
    for k in ks:
        m = md[k]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, ("scratch memory in", k, m)
        assert m["agpr_count"] == 0 and m["vgpr_count"] <= 128, (k, m)
