"""The state-record kernels (rg_state_io.hip: rg_state_save / rg_state_load), read from the built library like tests/test_kernel_resources.py (no GPU
needed): all five are there, and none uses scratch memory or spills."""
from test_kernel_resources import kernel_metadata


def test_state_record_kernels_use_no_scratch():
    md = kernel_metadata()
    names = ("k_state_rec_save", "k_state_words_save", "k_state_rec_load", "k_state_words_load", "k_state_stairs")
    for name in names:
        ks = [k for k in md if name in k]
        assert len(ks) == 1, (name, sorted(md))
        m = md[ks[0]]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, ("scratch memory in", ks[0], m)
        assert m["agpr_count"] == 0 and m["vgpr_count"] <= 128, (ks[0], m)
