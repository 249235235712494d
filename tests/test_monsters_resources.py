"""The budget of the built monster-table kernels (rogue-gym_amd/csrc/rg_monsters.hip), read from the code objects inside librogue_gym_hip.so: the three
instances exist, no scratch, no spills, no AGPRs, no LDS -- the sorted list lives in registers -- and no name that a resource test of another kernel
family would count."""
import os
import re
import subprocess
import tempfile

import test_kernel_resources as kr
from test_kernel_resources import kernel_metadata


def lds_bytes(pattern):
    """{kernel name: .group_segment_fixed_size} of the kernels whose name holds `pattern`, from the same notes kernel_metadata reads (it keeps no LDS size)."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run([os.path.join(kr.LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", kr.SO, fat], check=True)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(kr.MAGIC), blob)]
        for i, s in enumerate(starts):
            part, co = os.path.join(d, "b%d.bin" % i), os.path.join(d, "b%d.co" % i)
            open(part, "wb").write(blob[s:(starts[i + 1] if i + 1 < len(starts) else len(blob))])
            subprocess.run([os.path.join(kr.LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + part, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            "--output=" + co], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            notes = subprocess.run([os.path.join(kr.LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for blk in notes.split("- .agpr_count:")[1:]:
                f = dict(re.findall(r"\.(group_segment_fixed_size|name):\s+(\S+)", blk))
                if pattern in f.get("name", ""):
                    out[f["name"]] = int(f["group_segment_fixed_size"])
    return out


def test_budget_of_the_monster_kernels():
    md = kernel_metadata()
    mon = {k: m for k, m in md.items() if "k_monsters" in k}
    assert len(mon) == 3, sorted(mon)
    # built: 58 registers for the 4-row list, 81 for 8 rows, 136 for 16 (three registers per row, four slots in flight); a small margin on each
    for tag, bound in (("k_monstersILi4EE", 64), ("k_monstersILi8EE", 88), ("k_monstersILi16EE", 144)):
        hit = [k for k in mon if tag in k]
        assert len(hit) == 1, (tag, sorted(mon))
        print(hit[0], mon[hit[0]])
        assert mon[hit[0]]["vgpr_count"] <= bound, (hit[0], mon[hit[0]])
    for k, m in sorted(mon.items()):
        assert m["private_segment_fixed_size"] == 0, (k, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
        assert m["agpr_count"] == 0, (k, m)
        for other in ("k_step", "k_obs", "k_path", "k_route", "k_regen", "k_crop_typed", "k_action_mask", "k_episode"):
            assert other not in k, (k, other)
    lds = lds_bytes("k_monsters")
    assert sorted(lds) == sorted(mon) and not any(lds.values()), lds
