"""The register / scratch budget of k_obs_stream, read from the built library like tests/test_kernel_resources.py (no GPU needed).

A wave holds the mirror words of its run (OBS_RUN envs x 2 words) and of the next one in registers: 61 registers at 4 envs per run, eight waves per
SIMD -- what the 16 384 waves of a 65 536-env batch need to be resident at once (runs of 8 envs: 84 registers, 16: 134, both slower).  No scratch."""
from test_kernel_resources import kernel_metadata


def test_stream_kernel_registers_and_no_scratch():
    md = kernel_metadata()
    ks = [k for k in md if "k_obs_stream" in k]
    assert ks, sorted(md)
    for k in ks:
        m = md[k]
        assert m["vgpr_count"] <= 64 and m["agpr_count"] == 0, (k, m)
        assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, ("scratch memory in", k, m)
