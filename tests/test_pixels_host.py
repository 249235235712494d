"""The pixel rule without a GPU: rg_pixels_host against its numpy restatement (tests/pixel_util.py) on screens of random bytes with random tilesets, the gray
weights, the built-in tileset, the refusals, RogueEnv.render's printing modes -- and a stand-alone program around the rule's source built with
-fsanitize=address,undefined."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pixel_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


@pytest.mark.parametrize("th", pu.TILE_HEIGHTS)
@pytest.mark.parametrize("channels", (1, 3))
def test_whole_screen_against_numpy(lib, th, channels):
    rng = np.random.RandomState(100 * th + channels)
    font, pal = pu.random_tileset(rng, th)
    for H, W in pu.SIZES:
        screen = pu.random_screen(rng, H, W)
        assert len(np.unique(screen)) > 200
        rc, out = pu.pixels_host(lib, font, pal, channels, screen)
        assert rc == 0, lib.rg_last_error(None)
        assert out.shape == (channels, H * th, W * 8)
        assert np.array_equal(out, pu.full_image(font, pal, screen, channels)), (th, channels, H, W)


@pytest.mark.parametrize("th", pu.TILE_HEIGHTS)
@pytest.mark.parametrize("channels", (1, 3))
def test_windows_equal_the_slice_of_the_padded_image(lib, th, channels):
    rng = np.random.RandomState(7 * th + channels)
    font, pal = pu.random_tileset(rng, th)
    H, W = 17, 33
    screen = pu.random_screen(rng, H, W)
    centres = [(cy, cx) for cy in (0, H // 2, H - 1) for cx in (0, W // 2, W - 1)]  # the four corners, the four edges, the middle
    for ry, rx in pu.WINDOWS:
        for cy, cx in centres:
            rc, out = pu.pixels_host(lib, font, pal, channels, screen, (cy, cx), (ry, rx))
            assert rc == 0, lib.rg_last_error(None)
            want = pu.crop_image(font, pal, screen, channels, cy, cx, ry, rx)
            assert out.shape == want.shape == (channels, (2 * ry + 1) * th, (2 * rx + 1) * 8)
            assert np.array_equal(out, want), (th, channels, ry, rx, cy, cx)
    # the padding is ' ' THROUGH the tileset: its ink shows beside the paper
    rc, out = pu.pixels_host(lib, font, pal, 3, screen, (0, 0), (1, 1))
    corner = out[:, :th, :8]
    assert (corner[:, 0, 0] == pal[0x20]).all() and (corner[:, 0, 7] == pal[0x20]).all()


def test_gray_weights(lib):
    assert pu.lum(np.array([255, 255, 255])) == 255 and pu.lum(np.array([0, 0, 0])) == 0
    assert pu.lum(np.array([255, 0, 0])) == (77 * 255 + 128) >> 8 == 77
    assert pu.lum(np.array([0, 255, 0])) == 149 and pu.lum(np.array([0, 0, 255])) == 29
    assert pu.lum(np.array([10, 20, 30])) == (770 + 3000 + 870 + 128) >> 8
    font = np.full((256, 8), 0xF0, np.uint8)   # left half ink, right half paper
    pal = np.zeros((257, 3), np.uint8)
    pal[ord("a")] = (255, 255, 255)
    pal[ord("b")] = (255, 0, 0)
    pal[256] = (0, 0, 255)
    rc, out = pu.pixels_host(lib, font, pal, 1, np.array([[ord("a"), ord("b")]], np.uint8))
    assert rc == 0
    assert out[0, 0].tolist() == [255] * 4 + [29] * 4 + [77] * 4 + [29] * 4


def test_builtin_tileset(lib):
    font, pal = pu.default_tileset(lib)
    assert font.shape == (256, 8)
    printable = list(range(0x21, 0x7F))
    for g in printable:
        assert font[g].any(), "glyph 0x%02x has no ink" % g
    assert len({font[g].tobytes() for g in printable}) == len(printable)
    for g in range(256):
        if g not in printable:
            assert not font[g].any(), "glyph 0x%02x is not blank" % g
    lum = pu.lum(pal)
    for g in printable:
        assert tuple(pal[g]) != tuple(pal[256]) and lum[g] != lum[256], g
    assert lum[256] < 64  # a dark paper
    groups = [b"-|", b"+", b"#", b".", b"*", b"%", b"@", b"ABCXYZ"]   # walls, doors, passages, floor, gold, stairs, the player, monsters: told apart
    colours = [{tuple(pal[g]) for g in grp} for grp in groups]
    assert all(len(c) == 1 for c in colours) and len({next(iter(c)) for c in colours}) == len(groups)
    # NULL tables mean the built-in
    screen = np.frombuffer(b"-|+#.*%@AZ~ ", np.uint8).reshape(2, 6)
    rc, out = pu.pixels_host(lib, None, None, 3, screen, th=0)
    assert rc == 0 and np.array_equal(out, pu.full_image(font, pal, screen, 3))
    from rogue_gym_python._rogue_gym import Tileset
    ts = Tileset.default()
    assert np.array_equal(ts.font, font) and np.array_equal(ts.palette, pal) and ts.th == 8
    assert np.array_equal(ts.render(screen, rgb=False), pu.full_image(font, pal, screen, 1))


def test_refusals_leave_the_output_untouched(lib):
    rng = np.random.RandomState(3)
    font, pal = pu.random_tileset(rng, 16)
    screen = pu.random_screen(rng, 16, 32)
    for kw, frag in [(dict(th=7), "th"), (dict(th=17), "th"), (dict(channels=2), "channels"), (dict(channels=0), "channels"), (dict(center=(16, 0), window=(1, 1)), "centre"),
                     (dict(center=(0, 32), window=(1, 1)), "centre"), (dict(center=(0, 0), window=(48, 1)), "radius"), (dict(center=(0, 0), window=(1, 160)), "radius"),
                     (dict(center=(0, 0), window=(1, -1)), "radius")]:
        out = np.full(4096, 0xAB, np.uint8)
        rc, _ = pu.pixels_host(lib, font, pal, kw.get("channels", 1), screen, kw.get("center"), kw.get("window"), out=out, th=kw.get("th"))
        msg = lib.rg_last_error(None).decode()
        assert rc != 0 and msg.startswith("rg_pixels_host: ") and frag in msg, (kw, msg)
        assert (out == 0xAB).all(), kw
    out = np.full(64, 0xAB, np.uint8)
    assert lib.rg_pixels_host(8, font.ctypes.data, pal.ctypes.data, 1, 16, 32, None, 0, 0, -1, 0, out.ctypes.data) != 0 and "screen" in lib.rg_last_error(None).decode()
    assert lib.rg_pixels_host(8, font.ctypes.data, pal.ctypes.data, 1, 16, 32, screen.ctypes.data, 0, 0, -1, 0, None) != 0 and "out" in lib.rg_last_error(None).decode()
    assert lib.rg_pixels_host(8, font.ctypes.data, pal.ctypes.data, 1, 49, 32, screen.ctypes.data, 0, 0, -1, 0, out.ctypes.data) != 0 and "H, W" in lib.rg_last_error(None).decode()
    assert (out == 0xAB).all()


def test_render_modes_keep_printing(capsys):
    from rogue_gym.envs import ParallelRogueEnv, RogueEnv
    from rogue_gym_python._rogue_gym import PlayerState
    assert RogueEnv.metadata["render.modes"] == ["human", "ascii", "rgb_array"] and ParallelRogueEnv.metadata is RogueEnv.metadata
    env = RogueEnv.__new__(RogueEnv)   # (no device here: a state value is enough for render)
    screen = np.full((16, 32), ord(" "), np.uint8)
    screen[3, 4:9] = np.frombuffer(b"-@.*-", np.uint8)
    env.result = PlayerState(screen, np.zeros_like(screen), np.array([1, 7, 12, 12, 16, 16, 1, 1, 0, 0], np.int32), 17, 0)
    for mode in ("human", "ascii"):
        assert env.render(mode) is None
        assert capsys.readouterr().out == repr(env.result) + "\n"
    frame = env.render("rgb_array")
    assert capsys.readouterr().out == ""
    import ctypes as C  # noqa: F401
    from rogue_gym_python import _rogue_gym as inner
    font, pal = pu.default_tileset(inner.load_library())
    assert frame.dtype == np.uint8 and frame.shape == (16 * 8, 32 * 8, 3)
    assert np.array_equal(frame, pu.full_image(font, pal, screen, 3).transpose(1, 2, 0))


def test_rule_source_under_address_and_undefined_sanitizers(tmp_path):
    """rg_pixels_host's source (csrc/rg_pixels.h) in a stand-alone program of its own -- nothing sanitized is loaded into python."""
    cxx = shutil.which("g++") or shutil.which("clang++") or ("/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "pixels_host_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []   # the runtimes inside the program (clang's default)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + ["-I", os.path.join(ROOT, "rogue-gym_amd", "csrc"),
                   os.path.join(ROOT, "tests", "pixels_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith(", 0 bad"), r.stdout
