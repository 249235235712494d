"""The novelty rule without a GPU: rg_novelty_hash_host against its numpy restatement (tests/novelty_util.py) on screens whose key is no multiple of 8 bytes,
blank screens, swapped cells, windows that overhang every edge and corner, the POS key and the level in the salt; the 0 -> 1 rule on the finishing step; the
episodic insert (rg_novelty_insert_host) at the wrap-around, over a stale generation and at the drop; the host entries' refusals -- and the same cases in a
stand-alone program around the rule's source built with -fsanitize=address,undefined (tests/novelty_host_main.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import novelty_util as nu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


def random_screen(rng, h, w):
    return rng.randint(0, 256, (h, w)).astype(np.uint8)


def both(lib, what, level, screen, px, py, ry=0, rx=0):
    rc, got = nu.hash_host(lib, what, level, screen, px, py, ry, rx)
    assert rc == 0, lib.rg_last_error(None)
    assert got == nu.state_hash(what, screen, level, px, py, ry, rx), (what, level, screen.shape, px, py, ry, rx)
    assert got != 0
    return got


@pytest.mark.parametrize("h,w", [(17, 33), (16, 32), (24, 80), (3, 1), (5, 7)])
def test_screen_hash_against_numpy(lib, h, w):
    """33x17: 495 key bytes, the last word padded with a zero byte; 1x3: one byte."""
    rng = np.random.RandomState(h * 1000 + w)
    for _ in range(4):
        s = random_screen(rng, h, w)
        both(lib, nu.SCREEN, int(rng.randint(0, 30)), s, int(rng.randint(0, w)), int(rng.randint(0, h)))
    # rows 0 and H-1 (the message line and the status line) are not part of the key, the player's cell neither
    s = random_screen(rng, h, w)
    a = both(lib, nu.SCREEN, 1, s, 0, 0)
    t = s.copy()
    t[0] ^= 0x55
    t[h - 1] ^= 0x33
    assert both(lib, nu.SCREEN, 1, t, w - 1, h - 1) == a


def test_blank_and_swapped_screens(lib):
    blank = np.full((17, 33), ord(" "), np.uint8)
    hb = both(lib, nu.SCREEN, 1, blank, 3, 3)
    assert both(lib, nu.SCREEN, 1, np.zeros((17, 33), np.uint8), 3, 3) != hb
    rng = np.random.RandomState(5)
    s = random_screen(rng, 17, 33)
    base = both(lib, nu.SCREEN, 1, s, 3, 3)
    seen = {base, hb}
    for (y0, x0), (y1, x1) in [((1, 0), (1, 1)), ((1, 0), (2, 0)), ((1, 7), (1, 8)), ((5, 5), (9, 30)), ((15, 31), (15, 32)), ((1, 0), (15, 32))]:
        t = s.copy()
        assert t[y0, x0] != t[y1, x1]
        t[y0, x0], t[y1, x1] = s[y1, x1], s[y0, x0]
        k = both(lib, nu.SCREEN, 1, t, 3, 3)
        assert k not in seen, "a swapped pair of cells kept the hash"   # (a sum of word terms WITHOUT the index would)
        seen.add(k)
    # two equal words in different places: the index separates them
    u = blank.copy()
    u[1, 0:8] = np.frombuffer(b"ABCDEFGH", np.uint8)
    v = blank.copy()
    v[1, 8:16] = np.frombuffer(b"ABCDEFGH", np.uint8)
    assert both(lib, nu.SCREEN, 1, u, 0, 0) != both(lib, nu.SCREEN, 1, v, 0, 0)


@pytest.mark.parametrize("h,w", [(17, 33), (16, 32)])
def test_crops_over_every_edge_and_corner(lib, h, w):
    rng = np.random.RandomState(w)
    s = random_screen(rng, h, w)
    centres = [(py, px) for py in (0, 1, h // 2, h - 2, h - 1) for px in (0, w // 2, w - 1)]
    for ry, rx in [(0, 0), (1, 1), (2, 3), (4, 4), (5, 0), (0, 6), (h - 1, w - 1), (47, 159)]:
        for py, px in centres:
            both(lib, nu.CROP, 2, s, px, py, ry, rx)
    # what overhangs is ' ', and rows 0 / H-1 count as outside: a window over the top edge does not see row 0
    t = s.copy()
    t[0] = ord(" ") ^ 0x7f
    assert both(lib, nu.CROP, 2, t, 4, 1, 2, 2) == both(lib, nu.CROP, 2, s, 4, 1, 2, 2)
    pad = np.full((5, 5), ord(" "), np.uint8)
    pad[2:, 2:] = s[1:4, 0:3]
    assert both(lib, nu.CROP, 2, s, 0, 1, 2, 2) == nu.hash_bytes(pad.tobytes(), nu.CROP, 2)
    # the window moves with the player
    assert both(lib, nu.CROP, 2, s, 5, 5, 2, 2) != both(lib, nu.CROP, 2, s, 6, 5, 2, 2)


def test_pos_key_and_the_level_in_the_salt(lib):
    s = random_screen(np.random.RandomState(1), 16, 32)
    seen = set()
    for px, py in [(0, 0), (1, 0), (0, 1), (31, 15), (15, 31 - 16), (7, 9), (9, 7)]:
        k = both(lib, nu.POS, 1, s, px, py)
        assert k == nu.hash_bytes(bytes([px, 0, py, 0, 0, 0, 0, 0]), nu.POS, 1)
        assert k not in seen
        seen.add(k)
    assert both(lib, nu.POS, 1, np.zeros_like(s), 7, 9) == both(lib, nu.POS, 1, s, 7, 9)   # the screen is not part of it
    for what, ry, rx in ((nu.POS, 0, 0), (nu.SCREEN, 0, 0), (nu.CROP, 2, 2)):
        per_level = {both(lib, what, lvl, s, 7, 9, ry, rx) for lvl in (0, 1, 2, 3, 26, 255, 256, 100000)}
        assert len(per_level) == 8, what
    # `what` and the length are in the salt: the same bytes under another `what` hash otherwise
    tiny = random_screen(np.random.RandomState(2), 3, 8)
    assert both(lib, nu.SCREEN, 1, tiny, 0, 0) != nu.hash_bytes(tiny[1].tobytes(), nu.POS, 1)
    assert nu.hash_bytes(b"\1\0\0\0\0\0\0\0", nu.CROP, 1) != nu.hash_bytes(b"\1", nu.CROP, 1)   # equal words after padding, another length


def test_the_batch_form_of_the_restatement_equals_the_plain_one():
    rng = np.random.RandomState(8)
    for h, w in ((16, 32), (17, 33), (24, 80)):
        screens = rng.randint(0, 256, (9, h, w)).astype(np.uint8)
        levels = rng.randint(1, 30, 9)
        centers = np.stack([rng.randint(0, h, 9), rng.randint(0, w, 9)], axis=1)
        centers[0], centers[1] = (0, 0), (h - 1, w - 1)
        for what, ry, rx in ((nu.POS, 0, 0), (nu.SCREEN, 0, 0), (nu.CROP, 2, 3), (nu.CROP, 20, 40)):
            got = nu.batch_hashes(what, screens, levels, centers, ry, rx)
            want = [nu.state_hash(what, screens[e], int(levels[e]), int(centers[e][1]), int(centers[e][0]), ry, rx) for e in range(9)]
            assert got.dtype == np.uint64 and got.tolist() == want, (h, w, what)


def test_the_value_api_counter_without_a_device(lib):
    """VisitCounter (behind RogueEnv.visit_count / ParallelRogueEnv.visit_counts): the host hash and a dict per env."""
    from rogue_gym_python._rogue_gym import VisitCounter
    a = np.full((2, 16, 32), ord("."), np.uint8)
    a[0, 5, 7] = a[1, 9, 30] = ord("@")
    for what, crop, radii in (("screen", None, (0, 0)), ("pos", None, (0, 0)), ("crop", 2, (2, 2)), ("crop", (1, 3), (1, 3))):
        vc = VisitCounter(2, what, crop)
        assert vc.visit(a, [1, 2], True).tolist() == [1, 1]
        assert vc.hashes.tolist() == [nu.state_hash(nu.WHATS[what], a[0], 1, 7, 5, *radii), nu.state_hash(nu.WHATS[what], a[1], 2, 30, 9, *radii)]
        assert vc.visit(a, [1, 2], [False, False]).tolist() == [2, 2]
        assert vc.visit(a, [1, 3], [False, False]).tolist() == [3, 1]      # another level is another state
        assert vc.visit(a, [1, 3], [True, False]).tolist() == [1, 2]       # a new episode empties that env's memory only
    with pytest.raises(ValueError):
        VisitCounter(1, "map")
    with pytest.raises(ValueError):
        VisitCounter(1, "pos", 2)
    with pytest.raises(RuntimeError, match="player"):
        VisitCounter(1, "pos").visit(np.zeros((1, 16, 32), np.uint8), [1], True)


def test_a_zero_hash_becomes_one(lib):
    f = lib.rg_novelty_finish_host
    for salt in (0, 1, 0x1234, (1760 << 32) | (3 << 8) | 2):
        m = int(nu.mix(np.array([salt], np.uint64))[0])
        acc = (-m) % (1 << 64)   # acc + mix(salt) = 0, and mix(0) = 0
        assert f(acc, salt) == 1 == nu.finish(np.array([acc], np.uint64), np.array([salt], np.uint64))
        assert f((acc + 1) % (1 << 64), salt) == nu.finish(np.array([(acc + 1) % (1 << 64)], np.uint64), np.array([salt], np.uint64)) not in (0, 1)
    rng = np.random.RandomState(3)
    for _ in range(64):
        acc, salt = (int(rng.randint(0, 1 << 62)) << 2 | 1 for _ in range(2))
        assert f(acc, salt) == nu.finish(np.array([acc], np.uint64), np.array([salt], np.uint64))


def test_episodic_insert_wraps_at_the_last_slot(lib):
    cap = 8
    slots, _keep = nu.host_table(cap)
    ref = nu.ProbeTable(cap)
    ref.gen = 5
    keys = [0x107, 0x207, 0x307, 0x107, 0x207, 0x10f, 0x307, 0x307]   # all start at slot 7: the second lands in slot 0, the third in slot 1
    for k in keys:
        rc, c = nu.insert_host(lib, slots, 5, k)
        assert rc == 0 and c == ref.insert(k), (hex(k), c)
    assert [int(slots["hash"][i]) for i in (7, 0, 1, 2)] == [0x107, 0x207, 0x307, 0x10f]
    assert [int(slots["count"][i]) for i in (7, 0, 1, 2)] == [2, 2, 3, 1] and (slots["gen"][[7, 0, 1, 2]] == 5).all()
    assert (slots["gen"][3:7] == 0).all() and (slots["hash"][3:7] == 0).all()


def test_a_stale_generation_is_an_empty_slot(lib):
    cap = 4
    slots, _keep = nu.host_table(cap)
    for k in (0x10, 0x20, 0x30, 0x40):
        assert nu.insert_host(lib, slots, 1, k) == (0, 1)
    assert nu.insert_host(lib, slots, 1, 0x20) == (0, 2)
    # generation 2: every slot is stale; the first probe takes slot 0 whatever it held, and the old counts do not leak
    assert nu.insert_host(lib, slots, 2, 0x20) == (0, 1)
    assert (int(slots["hash"][0]), int(slots["gen"][0]), int(slots["count"][0])) == (0x20, 2, 1)
    assert nu.insert_host(lib, slots, 2, 0x10) == (0, 1)            # slot 0 is current with another hash -> slot 1, stale, reused
    assert (int(slots["hash"][1]), int(slots["gen"][1])) == (0x10, 2)
    assert nu.insert_host(lib, slots, 2, 0x10) == (0, 2)
    assert (slots["gen"][2:] == 1).all()


def test_a_full_table_drops_the_visit(lib):
    cap = 4
    slots, _keep = nu.host_table(cap)
    ref = nu.ProbeTable(cap)
    ref.gen = 9
    for k in (1, 2, 3, 4, 5, 6, 1, 4, 5):
        rc, c = nu.insert_host(lib, slots, 9, k)
        assert rc == 0 and c == ref.insert(k), k
    before = slots.copy()
    assert nu.insert_host(lib, slots, 9, 77) == (0, 0) and ref.insert(77) == 0   # cap probes, neither a match nor an empty slot
    assert (slots == before).all()
    assert nu.insert_host(lib, slots, 9, 3) == (0, 2)               # what is in stays countable
    assert nu.insert_host(lib, slots, 10, 77) == (0, 1)             # and a new episode has room again


def test_host_refusals(lib):
    s = np.zeros((16, 32), np.uint8)
    out = C.c_uint64(0xABAB)
    def refused(frag, *a):
        rc = lib.rg_novelty_hash_host(*a, C.byref(out))
        msg = lib.rg_last_error(None).decode()
        assert rc != 0 and msg.startswith("rg_novelty_hash_host: ") and frag in msg, (a, msg)
        assert out.value == 0xABAB
    p = s.ctypes.data
    refused("what", 0, 1, 16, 32, p, 0, 0, 0, 0)
    refused("what", 4, 1, 16, 32, p, 0, 0, 0, 0)
    refused("radius", nu.POS, 1, 16, 32, p, 0, 0, 1, 0)
    refused("radius", nu.SCREEN, 1, 16, 32, p, 0, 0, 0, 1)
    refused("radius", nu.CROP, 1, 16, 32, p, 0, 0, 48, 1)
    refused("radius", nu.CROP, 1, 16, 32, p, 0, 0, 1, 160)
    refused("radius", nu.CROP, 1, 16, 32, p, 0, 0, -1, 1)
    refused("height", nu.SCREEN, 1, 2, 32, p, 0, 0, 0, 0)
    refused("height", nu.SCREEN, 1, 49, 32, p, 0, 0, 0, 0)
    refused("height", nu.SCREEN, 1, 16, 161, p, 0, 0, 0, 0)
    refused("player", nu.POS, 1, 16, 32, p, 32, 0, 0, 0)
    refused("player", nu.POS, 1, 16, 32, p, 0, 16, 0, 0)
    refused("level", nu.POS, -1, 16, 32, p, 0, 0, 0, 0)
    refused("screen", nu.SCREEN, 1, 16, 32, None, 0, 0, 0, 0)
    assert lib.rg_novelty_hash_host(nu.POS, 1, 16, 32, p, 0, 0, 0, 0, None) != 0 and "hash" in lib.rg_last_error(None).decode()
    slots, _keep = nu.host_table(8)
    cnt = C.c_uint32(7)
    for args, frag in [((None, 8, 1, 5), "slots"), ((slots.ctypes.data + 8, 4, 1, 5), "aligned"), ((slots.ctypes.data, 6, 1, 5), "cap"), ((slots.ctypes.data, 0, 1, 5), "cap"),
                       ((slots.ctypes.data, 1 << 17, 1, 5), "cap")]:
        assert lib.rg_novelty_insert_host(*args, C.byref(cnt)) != 0
        msg = lib.rg_last_error(None).decode()
        assert msg.startswith("rg_novelty_insert_host: ") and frag in msg, msg
        assert cnt.value == 7 and not slots["hash"].any()
    assert lib.rg_novelty_insert_host(slots.ctypes.data, 8, 1, 5, None) != 0 and "count" in lib.rg_last_error(None).decode()


def test_rule_source_under_address_and_undefined_sanitizers(tmp_path):
    """The same cases on exact-size heap buffers in a stand-alone program of its own -- nothing sanitized is loaded into python."""
    cxx = shutil.which("g++") or shutil.which("clang++") or ("/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    if not os.path.exists(os.path.join(rocm_inc, "hip", "hip_runtime.h")):
        pytest.skip("no ROCm include directory (the rule headers include hip/hip_runtime.h for __host__ __device__)")
    exe = str(tmp_path / "novelty_host_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []   # the runtimes inside the program (clang's default)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-D__HIP_PLATFORM_AMD__", "-I", rocm_inc, "-I", os.path.join(ROOT, "rogue-gym_amd", "csrc"), "-I", os.path.join(ROOT, "rogue-gym_amd"),
                    os.path.join(ROOT, "tests", "novelty_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith(", 0 bad"), r.stdout
