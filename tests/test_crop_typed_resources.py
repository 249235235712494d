"""Registers and scratch of the crop kernels (k_crop_typed in rg_crop_typed.hip: f32 / f16 / bf16 windows, u8 symbol-id windows), read from the built
library's code objects (no GPU needed).  tests/test_crop_resources.py checks the two f32 instances by themselves, and tests/test_obs_typed_resources.py
counts the k_obs_typed instances by name and pins the register counts of the f32 crop and of rg_obs.hip's kernels."""
from test_kernel_resources import kernel_metadata

# kind, RG_OBS_* type of every compiled instance: gray and one-hot in f32 (0), f16 (1) and bf16 (2), symbol ids in u8 (3)
TYPED = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 3)]


def test_exactly_the_seven_crop_instances_without_scratch_spills_or_agprs():
    md = kernel_metadata()
    for kind, dt in TYPED:
        names = [k for k in md if "k_crop_typedILi%dELi%dE" % (kind, dt) in k]
        assert len(names) == 1, (kind, dt, sorted(k for k in md if "k_crop_typed" in k))
        m = md[names[0]]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["agpr_count"] == 0, (names[0], m)
        assert m["vgpr_count"] <= 128, (names[0], m)
    assert len([k for k in md if "k_crop_typed" in k]) == len(TYPED)


def test_the_typed_crop_is_not_counted_among_the_earlier_kernels():
    """The name carries neither substring the earlier resource tests count by."""
    md = kernel_metadata()
    for k in md:
        if "k_crop_typed" in k:
            assert "k_obs_crop" not in k and "k_obs_typed" not in k, k
