"""The typed-crop entry points at the drop-in boundary (no GPU needed), and the numpy reference of their GPU tests: the f32 window of
parity_util.crop_window rounded with typed_util (16-bit kinds), and the window of symbol ids padded with 0, the id of ' ' (kind 2) -- each against
a plain per-cell loop on a 5x7 image, as tests/test_crop_window.py checks crop_window itself."""
import os
import re

import numpy as np
import pytest

import typed_util as tu
from parity_util import crop_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rg_obs_crop_typed", "rg_step_obs_crop_typed")


def typed_crop_reference(img_f32, cy, cx, ry, rx, kind, planes, with_hist, dtype):
    """The window rg_obs_crop_typed writes for one env.  Kinds 0 / 1: `img_f32` is the env's f32 image [C, H, W]; uint16 bit patterns
    [C, 2ry+1, 2rx+1] of the f32 window rounded to `dtype`.  Kind 2: `img_f32` is [1 + with_hist, H, W] holding the symbol ids (and the 0 / 1
    history plane) as numbers; uint8 [1 + with_hist, 2ry+1, 2rx+1], every plane padded with 0."""
    img = np.asarray(img_f32, np.float32)
    if kind == 2:
        assert dtype == tu.RG_OBS_U8 and img.shape[0] == 1 + int(bool(with_hist))
        return crop_window(img, cy, cx, ry, rx, 0, 1, with_hist).astype(np.uint8)
    return tu.bits16(crop_window(img, cy, cx, ry, rx, kind, planes, with_hist), dtype)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


def test_typed_crop_entry_points_are_declared_exported_and_bound(lib):
    from rogue_gym_python import _rogue_gym as inner
    hdr = open(os.path.join(ROOT, "include", "rogue_gym_hip.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, hdr, re.M), "%s is not declared in the header" % name
        assert hasattr(lib, name), "missing export %s" % name
        assert name in inner._INT_FUNCS, "%s is not in the ctypes table" % name
        assert getattr(lib, name).argtypes is not None, "%s has no ctypes signature" % name
    assert len(lib.rg_obs_crop_typed.argtypes) == 9 and len(lib.rg_step_obs_crop_typed.argtypes) == 11
    assert "Not typed (f32 only): the crop" not in hdr


def loop_reference(img, cy, cx, ry, rx, kind, planes, with_hist, dtype):
    c, h, w = img.shape
    nst = 0 if kind == 2 else c - planes - (1 if with_hist else 0)
    out = np.empty((c, 2 * ry + 1, 2 * rx + 1), np.uint8 if kind == 2 else np.uint16)
    for ch in range(c):
        for dy in range(2 * ry + 1):
            for dx in range(2 * rx + 1):
                y, x = cy - ry + dy, cx - rx + dx
                if 0 <= y < h and 0 <= x < w:
                    v = img[ch, y, x]
                elif kind == 2:
                    v = 0.0                                  # the id of ' ', never visited
                elif ch < planes:
                    v = 1.0 if (kind and ch == 0) else 0.0   # the encoding of ' '
                elif ch < planes + nst:
                    v = img[ch, 0, 0]                        # a status plane is one constant
                else:
                    v = 0.0
                out[ch, dy, dx] = int(v) if kind == 2 else tu.bits16(np.float32(v), dtype).reshape(-1)[0]
    return out


def image(kind, planes, nst, with_hist, h=5, w=7, seed=0):
    rng = np.random.RandomState(seed)
    if kind == 2:
        img = np.empty((1 + int(with_hist), h, w), np.float32)
        img[0] = rng.randint(0, 44, (h, w))
        img[0, 1, 2] = 255  # a glyph without a symbol
    else:
        img = np.empty((planes + nst + int(with_hist), h, w), np.float32)
        if kind:
            img[:planes] = np.eye(planes, dtype=np.float32)[rng.randint(0, planes, (h, w))].transpose(2, 0, 1)
        else:
            img[0] = (rng.randint(0, 43, (h, w)).astype(np.float32) / np.float32(43))
        for k in range(nst):
            img[planes + k] = float((70000, 257, 3, 65519)[k % 4])  # binary16 overflow, a bf16 tie, an exact value, the last finite f16 tie
    if with_hist:
        img[-1] = rng.randint(0, 2, (h, w))
    return img


@pytest.mark.parametrize("kind,planes,nst,with_hist,dtype", [
    (0, 1, 0, False, tu.RG_OBS_F16), (0, 1, 4, True, tu.RG_OBS_BF16), (1, 4, 0, False, tu.RG_OBS_BF16), (1, 4, 3, True, tu.RG_OBS_F16),
    (2, 1, 0, False, tu.RG_OBS_U8), (2, 1, 0, True, tu.RG_OBS_U8)])
def test_typed_crop_reference_matches_a_cell_loop(kind, planes, nst, with_hist, dtype):
    img = image(kind, planes, nst, with_hist)
    c, h, w = img.shape
    centres = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, 3), (h - 1, 3), (2, 0), (2, w - 1), (2, 3)]
    for ry, rx in ((0, 0), (1, 2), (3, 3), (6, 9), (2, 0), (0, 4)):
        for cy, cx in centres:
            got = typed_crop_reference(img, cy, cx, ry, rx, kind, planes, with_hist, dtype)
            exp = loop_reference(img, cy, cx, ry, rx, kind, planes, with_hist, dtype)
            assert got.shape == (c, 2 * ry + 1, 2 * rx + 1) and got.dtype == exp.dtype
            assert np.array_equal(got, exp), (ry, rx, cy, cx)


def test_id_window_keeps_255_and_pads_with_the_id_of_a_blank():
    img = image(2, 1, 0, True)
    win = typed_crop_reference(img, 1, 2, 1, 1, 2, 1, True, tu.RG_OBS_U8)
    assert win[0, 1, 1] == 255
    far = typed_crop_reference(img, 0, 0, 2, 2, 2, 1, True, tu.RG_OBS_U8)
    assert (far[:, :2, :] == 0).all() and (far[:, :, :2] == 0).all() and tu.symbol_ids(np.frombuffer(b" ", np.uint8))[0] == 0
