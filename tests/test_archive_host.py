"""The archive rule without a GPU: rg_archive_offer_host -- the probe and the beats rule, one offer at a time on a host table -- against a Python dict
(tests/archive_util.py) over a few thousand seeded offers with the extreme scores and step counts, key 0, and a 1 024-cell table driven to overflow; the
entry's refusals; and the same rule source in a stand-alone program built with -fsanitize=address,undefined (tests/archive_host_main.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import archive_util as au

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORES = [au.I32_MIN, -1, 0, au.I32_MAX, 5, -70000]
STEPS = [0, au.U32_MAX, 1, 40, 1 << 31]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


class OneByOne:
    """The dict oracle for offers that arrive one at a time: key -> [score, steps, seen, when]."""

    def __init__(self):
        self.cells = {}

    def offer(self, key, score, steps, serial, admitted):
        key = key or 1
        if not admitted:
            assert key not in self.cells
            return 0
        c = self.cells.setdefault(key, [None, None, 0, 0])
        c[2] += 1
        if c[3] == 0 or au.beats(score, steps, c[0], c[1]):
            c[0], c[1], c[3] = score, steps, serial
            return 1
        return 0


def check_table(slots, ref):
    at = np.nonzero(slots["key"])[0]
    assert sorted(int(k) for k in slots["key"][at]) == sorted(ref.cells)
    for i in at:
        s = slots[i]
        assert [int(s["score"]), int(s["steps"]), int(s["seen"]), int(s["when"])] == ref.cells[int(s["key"])], hex(int(s["key"]))
        assert int(s["chosen"]) == 0 and int(s["zero"]) == 0
    rest = np.delete(slots, at)
    assert not rest.view(np.uint8).any()   # an empty slot is all zero


def test_seeded_offers_against_a_dict(lib):
    rng = np.random.RandomState(11)
    cells = 4096
    slots, ref = au.host_table(cells), OneByOne()
    keys = [0, 1, cells - 1, (1 << 64) - 1, 1 << 63] + [int(rng.randint(0, 1 << 62)) * 4 + int(rng.randint(0, 4)) for _ in range(300)]
    where = {}
    for i in range(6000):
        key = keys[int(rng.randint(0, len(keys)))]
        score = SCORES[int(rng.randint(0, len(SCORES)))] if rng.randint(0, 2) else int(rng.randint(-3, 4))
        steps = STEPS[int(rng.randint(0, len(STEPS)))] if rng.randint(0, 2) else int(rng.randint(0, 5))
        serial = 1 + i // 50
        rc, slot, stored = au.offer_host(lib, slots, key, score, steps, serial)
        assert rc == 0 and slot >= 0, lib.rg_last_error(None)
        assert int(slots["key"][slot]) == (key or 1)
        assert where.setdefault(key or 1, slot) == slot          # a key never moves
        assert stored == ref.offer(key, score, steps, serial, True), (i, hex(key), score, steps)
    check_table(slots, ref)
    assert 1 in ref.cells and ref.cells[1][2] > 0   # key 0 was offered as 1, together with key 1


def test_the_order_of_the_rule(lib):
    slots = au.host_table(1024)
    o = lambda score, steps, serial: au.offer_host(lib, slots, 77, score, steps, serial)[2]
    assert o(au.I32_MIN, au.U32_MAX, 1) == 1      # an empty slot is beaten by anything, the worst offer there is included
    assert o(au.I32_MIN, au.U32_MAX, 2) == 0      # equal (score, steps) from a later call replaces nothing
    assert o(au.I32_MIN, au.U32_MAX - 1, 2) == 1  # fewer steps at the same score
    assert o(-1, 50, 3) == 1 and o(-2, 0, 3) == 0 and o(0, au.U32_MAX, 4) == 1 and o(0, 0, 4) == 1 and o(0, 0, 5) == 0
    assert o(au.I32_MAX, 7, 6) == 1 and o(au.I32_MAX, 8, 7) == 0 and o(au.I32_MAX, 0, 8) == 1 and o(au.I32_MAX, 0, 9) == 0
    s = slots[77]
    assert (int(s["key"]), int(s["score"]), int(s["steps"]), int(s["seen"]), int(s["when"])) == (77, au.I32_MAX, 0, 12, 8)


def test_a_1024_cell_table_driven_to_overflow(lib):
    rng = np.random.RandomState(3)
    cells = 1024
    slots, ref = au.host_table(cells), OneByOne()
    keys = [int(k) for k in rng.randint(1, 1 << 62, 1400)]
    drops = 0
    for rnd in range(3):
        for i, key in enumerate(keys):
            score, steps = int(rng.randint(-5, 6)), int(rng.randint(0, 9))
            full = int(np.count_nonzero(slots["key"])) == cells
            rc, slot, stored = au.offer_host(lib, slots, key, score, steps, rnd + 1)
            assert rc == 0
            admitted = key in ref.cells or not full     # 1 024 probes of 1 024 slots: dropped iff the key is new and no slot is empty
            assert (slot >= 0) == admitted, (rnd, i)
            assert stored == ref.offer(key, score, steps, rnd + 1, admitted)
            drops += not admitted
    assert drops == 3 * (1400 - 1024) and len(ref.cells) == cells
    check_table(slots, ref)   # the stored keys stay exact


def test_probing_wraps_at_the_last_slot(lib):
    slots = au.host_table(8)
    got = [au.offer_host(lib, slots, k, 0, 0, 1)[1] for k in (0x107, 0x207, 0x307, 0x107, 0x10f)]
    assert got == [7, 0, 1, 7, 2]


def test_refusals_write_nothing(lib):
    slots = au.host_table(1024)
    import ctypes as C
    raw = np.zeros(1024 * 32 + 16, np.uint8)
    odd = raw.ctypes.data + (-raw.ctypes.data % 8) + 4   # four bytes past an 8-byte boundary
    slot, stored = C.c_int32(-7), C.c_int32(-7)
    for args, frag in [((None, 1024, 5, 0, 0, 1), "slots"), ((slots.ctypes.data, 1000, 5, 0, 0, 1), "cells"), ((slots.ctypes.data, 0, 5, 0, 0, 1), "cells"),
                       ((slots.ctypes.data, 1 << 25, 5, 0, 0, 1), "cells"), ((slots.ctypes.data, 1024, 5, 0, 0, 0), "serial"), ((odd, 1024, 5, 0, 0, 1), "aligned")]:
        assert lib.rg_archive_offer_host(*args, C.byref(slot), C.byref(stored)) != 0
        msg = lib.rg_last_error(None).decode()
        assert msg.startswith("rg_archive_offer_host: ") and frag in msg, msg
        assert slot.value == -7 and stored.value == -7 and not slots.view(np.uint8).any() and not raw.any()
    assert lib.rg_archive_offer_host(slots.ctypes.data, 1024, 5, 0, 0, 1, None, C.byref(stored)) != 0 and "slot" in lib.rg_last_error(None).decode()


def test_rule_source_under_address_and_undefined_sanitizers(tmp_path):
    """The same rule on exact-size heap tables in a stand-alone program of its own -- nothing sanitized is loaded into python."""
    cxx = shutil.which("g++") or shutil.which("clang++") or ("/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    if not os.path.exists(os.path.join(rocm_inc, "hip", "hip_runtime.h")):
        pytest.skip("no ROCm include directory (the rule header includes hip/hip_runtime.h for __host__ __device__)")
    exe = str(tmp_path / "archive_host_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []   # the runtimes inside the program (clang's default)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-D__HIP_PLATFORM_AMD__", "-I", rocm_inc, "-I", os.path.join(ROOT, "rogue-gym_amd", "csrc"), "-I", os.path.join(ROOT, "rogue-gym_amd"),
                    os.path.join(ROOT, "tests", "archive_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith(", 0 bad"), r.stdout
