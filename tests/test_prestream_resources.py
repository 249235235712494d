"""The pre-streamed encode's footprint, read from the sources and the built library like tests/test_tail_encode_resources.py (no GPU needed).

k_step_w32<false, true> now carries the helper blocks' streaming loop (two runs of four envs' mirror words in registers) beside the turn, and the turn
carries a 16-bit line mask from mirror_update to its tail.  It must stay inside the cap the other instances live under -- 256 registers, two waves per SIMD:
the helpers run in the wave slots that cap leaves free -- without scratch memory and without AGPRs.  k_obs_resid, now the fix-up pass, keeps its pin: 64
registers, eight waves per SIMD, no scratch."""
import os
import re

from test_kernel_resources import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rogue-gym_amd", "csrc")


def test_enc_rows_replaces_the_stamps():
    state = open(os.path.join(CSRC, "rg_state.h")).read()
    assert re.search(r"uint16_t\s*\*\s*enc_rows\s*;", state), "RgState::enc_rows u16 [n] is missing"
    for gone in ("enc_stamp", "enc_step", "enc_cut"):
        assert gone not in state, gone
    kernels = open(os.path.join(CSRC, "rg_kernels.hip")).read()
    assert "S.enc_rows[" in kernels and "s_memrealtime() - enc_t0" not in kernels
    assert "S.enc_rows[" in open(os.path.join(CSRC, "rg_obs.hip")).read()
    assert "S.enc_rows" in open(os.path.join(CSRC, "rg_api.cpp")).read()


def test_enc_instance_stays_under_the_cap():
    md = kernel_metadata()
    enc = [k for k in md if "k_step_w32ILb0ELb1E" in k]   # k_step_w32<BND = false, ENC = true>
    assert len(enc) == 1, sorted(md)
    m = md[enc[0]]
    assert m["vgpr_count"] <= 256 and m["agpr_count"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, ("scratch memory", m)


def test_fix_up_pass_registers_and_no_scratch():
    md = kernel_metadata()
    ks = [k for k in md if "k_obs_resid" in k]
    assert len(ks) == 1, sorted(md)
    m = md[ks[0]]
    assert m["vgpr_count"] <= 64 and m["agpr_count"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, ("scratch memory", m)
