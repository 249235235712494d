"""The register / scratch budget of the tail encode's two kernels, read from the built library like tests/test_kernel_resources.py (no GPU needed).

k_step_w32<false, true> is the capped step kernel plus, at the end of every wave, the encode of its envs' gray images in batches of 8 envs -- two batches
of mirror words in registers.  It must stay inside the cap the other instances live under (256 registers = two waves per SIMD, every block of a 65 536-env
launch resident from t = 0) without scratch memory.  k_obs_resid serves the envs the tails left; it holds no run of mirror words, so it must not need more
registers than k_obs_stream, the pass it replaces behind such a launch: 64 (tests/test_obs_stream_resources.py; the built parent takes 61), eight waves
per SIMD."""
from test_kernel_resources import kernel_metadata


def test_enc_instance_of_the_capped_step_kernel():
    md = kernel_metadata()
    enc = [k for k in md if "k_step_w32ILb0ELb1E" in k]   # k_step_w32<BND = false, ENC = true>
    assert len(enc) == 1, sorted(md)
    m = md[enc[0]]
    assert m["vgpr_count"] <= 256 and m["agpr_count"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, ("scratch memory", m)
    # the instances without the encode are there as before
    assert [k for k in md if "k_step_w32ILb0ELb0E" in k] and [k for k in md if "k_step_w32ILb1ELb0E" in k], sorted(md)


def test_residual_pass_registers_and_no_scratch():
    md = kernel_metadata()
    ks = [k for k in md if "k_obs_resid" in k]
    assert len(ks) == 1, sorted(md)
    m = md[ks[0]]
    assert m["vgpr_count"] <= 64 and m["agpr_count"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, ("scratch memory", m)
