"""Registers and scratch of the typed observation kernels (k_obs_typed: f16 / bf16 images, u8 symbol ids), read from the built library's code objects
(no GPU needed), and the register counts of the observation kernels that were there before them: adding the typed instances to the translation unit
must leave those -- the headline's kernels among them -- exactly as the compiler made them without."""
import re

from test_kernel_resources import kernel_metadata

# kind, RG_OBS_* type of every compiled instance: gray and one-hot in f16 (1) and bf16 (2), symbol ids in u8 (3)
TYPED = [(0, 1), (0, 2), (1, 1), (1, 2), (2, 3)]

# vgpr_count, sgpr_spill_count of the pre-existing kernels of rg_obs.hip in a build of the commit before the typed kernels (same compiler, same flags).
# The f32 crop is the RG_OBS_F32 instance of k_crop_typed (rg_crop_typed.hip): no more registers than the kernel it replaced (k_obs_crop: 40 and 44).
BEFORE = {
    r"k_obsILi0ELb0ELb0E": (79, 0),
    r"k_obsILi0ELb0ELb1E": (81, 2),
    r"k_obsILi0ELb1ELb0E": (80, 2),
    r"k_obsILi1ELb0ELb0E": (94, 11),
    r"k_obsILi1ELb0ELb1E": (95, 13),
    r"k_obsILi1ELb1ELb0E": (102, 14),
    r"k_obs_stream": (61, 0),
    r"k_crop_typedILi0ELi0E": (38, 0),
    r"k_crop_typedILi1ELi0E": (44, 0),
    r"\d+k_gray": (49, 0),
    r"\d+k_symbol": (50, 0),
    r"\d+k_render": (26, 0),
    r"k_encode_scalar": (23, 0),
}


def test_typed_instances_exist_without_scratch_spills_or_agprs():
    md = kernel_metadata()
    for kind, dt in TYPED:
        names = [k for k in md if "k_obs_typedILi%dELi%dE" % (kind, dt) in k]
        assert len(names) == 1, (kind, dt, sorted(k for k in md if "k_obs_typed" in k))
        m = md[names[0]]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["agpr_count"] == 0, (names[0], m)
        assert m["vgpr_count"] <= 128, (names[0], m)  # four 64-lane waves per SIMD at the least
    assert len([k for k in md if "k_obs_typed" in k]) == len(TYPED)
    sweep = [k for k in md if "k_redraw" in k]  # the Redraw sweep in front of the typed pass
    assert len(sweep) == 1, sweep
    m = md[sweep[0]]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["agpr_count"] == 0 and m["vgpr_count"] <= 64, m


def test_earlier_observation_kernels_keep_their_registers():
    md = kernel_metadata()
    for pat, (vgpr, sspill) in BEFORE.items():
        names = [k for k in md if re.search(pat, k)]
        assert len(names) == 1, (pat, names)
        m = md[names[0]]
        assert (m["vgpr_count"], m["sgpr_spill_count"], m["vgpr_spill_count"], m["agpr_count"], m["private_segment_fixed_size"]) == (vgpr, sspill, 0, 0, 0), (names[0], m)
