"""parity_util.crop_window (the expected crop of tests/test_gpu_obs_oracle.py) against a plain per-cell loop on small hand-made images: windows
at the corners and edges, wider and taller than the screen, gray and one-hot, with status planes and a history plane."""
import numpy as np
import pytest

from parity_util import crop_window


def loop_window(img, cy, cx, ry, rx, kind, planes, with_hist):
    c, h, w = img.shape
    nst = c - planes - (1 if with_hist else 0)
    out = np.empty((c, 2 * ry + 1, 2 * rx + 1), np.float32)
    for ch in range(c):
        for dy in range(2 * ry + 1):
            for dx in range(2 * rx + 1):
                y, x = cy - ry + dy, cx - rx + dx
                if 0 <= y < h and 0 <= x < w:
                    v = img[ch, y, x]
                elif ch < planes:
                    v = 1.0 if (kind and ch == 0) else 0.0   # the encoding of ' '
                elif ch < planes + nst:
                    v = img[ch, 0, 0]                        # a status plane is one constant
                else:
                    v = 0.0                                  # history: never visited
                out[ch, dy, dx] = v
    return out


def image(kind, planes, nst, with_hist, h=5, w=7, seed=0):
    rng = np.random.RandomState(seed)
    c = planes + nst + (1 if with_hist else 0)
    img = np.empty((c, h, w), np.float32)
    if kind:
        img[:planes] = np.eye(planes, dtype=np.float32)[rng.randint(0, planes, (h, w))].transpose(2, 0, 1)
    else:
        img[0] = rng.randint(0, 30, (h, w)) / 43.0
    for k in range(nst):
        img[planes + k] = float(rng.randint(1, 100))
    if with_hist:
        img[-1] = rng.randint(0, 2, (h, w))
    return img


@pytest.mark.parametrize("kind,planes,nst,with_hist", [(0, 1, 0, False), (0, 1, 9, True), (1, 4, 0, False), (1, 4, 2, True)])
def test_crop_window_matches_a_cell_loop(kind, planes, nst, with_hist):
    img = image(kind, planes, nst, with_hist)
    c, h, w = img.shape
    centres = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, 3), (h - 1, 3), (2, 0), (2, w - 1), (2, 3)]
    for ry, rx in ((0, 0), (1, 2), (3, 3), (6, 9), (2, 0), (0, 4)):
        for cy, cx in centres:
            got = crop_window(img, cy, cx, ry, rx, kind, planes, with_hist)
            exp = loop_window(img, cy, cx, ry, rx, kind, planes, with_hist)
            assert got.shape == (c, 2 * ry + 1, 2 * rx + 1)
            assert np.array_equal(got, exp), (ry, rx, cy, cx)


def test_crop_window_of_a_whole_screen_inside_is_a_slice():
    img = image(1, 3, 1, True, h=9, w=11, seed=2)
    assert np.array_equal(crop_window(img, 4, 5, 2, 3, 1, 3, True), img[:, 2:7, 2:9])
    assert np.array_equal(crop_window(img, 4, 5, 4, 5, 1, 3, True), img)
