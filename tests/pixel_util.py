"""The pixel rule restated in numpy (np.unpackbits of font[screen], np.where with the palette), and the random tilesets and screens the pixel tests share."""
import ctypes as C

import numpy as np

SIZES = ((16, 32), (17, 33), (24, 80), (33, 97))   # (H, W)
WINDOWS = ((0, 0), (5, 5), (1, 7), (47, 159))       # (ry, rx)
TILE_HEIGHTS = (8, 13, 16)


def lum(rgb):
    """(77 r + 150 g + 29 b + 128) >> 8 over the last axis."""
    rgb = np.asarray(rgb).astype(np.uint32)
    return ((77 * rgb[..., 0] + 150 * rgb[..., 1] + 29 * rgb[..., 2] + 128) >> 8).astype(np.uint8)


def random_tileset(rng, th):
    """(font u8 [256, th], palette u8 [257, 3]): random bits and colours; ' ' has ink, and its ink differs from the paper in every channel and in luminance, so
    that a padding cell rendered as anything but ' ' through the tileset shows."""
    font = rng.randint(0, 256, (256, th)).astype(np.uint8)
    pal = rng.randint(0, 256, (257, 3)).astype(np.uint8)
    font[0x20] |= 0x81
    pal[0x20] = (250, 5, 130)
    pal[256] = (3, 200, 40)
    return font, pal


def random_screen(rng, H, W):
    return rng.randint(0, 256, (H, W)).astype(np.uint8)


def full_image(font, pal, screen, channels):
    """u8 [C, H*th, W*8] of one screen u8 [H, W]."""
    H, W = screen.shape
    th = font.shape[1]
    ink = np.unpackbits(font[screen], axis=-1).reshape(H, W, th, 8).transpose(0, 2, 1, 3).reshape(H * th, W * 8).astype(bool)
    g = np.repeat(np.repeat(screen, th, axis=0), 8, axis=1)
    tab = pal if channels == 3 else lum(pal)[:, None]
    return np.stack([np.where(ink, tab[g, c], tab[256, c]) for c in range(channels)]).astype(np.uint8)


def crop_image(font, pal, screen, channels, cy, cx, ry, rx):
    """The window around (cy, cx): the slice of the full image of the screen padded with ' ' cells on every side."""
    th = font.shape[1]
    padded = np.pad(screen, ((ry, ry), (rx, rx)), constant_values=0x20)
    full = full_image(font, pal, padded, channels)
    return full[:, cy * th:(cy + 2 * ry + 1) * th, cx * 8:(cx + 2 * rx + 1) * 8]


def pixels_host(lib, font, pal, channels, screen, center=None, window=None, out=None, th=None):
    """rg_pixels_host; returns (rc, out).  font / pal None: NULL."""
    H, W = screen.shape
    rows = 8 if font is None else font.shape[1]   # (the built-in font is 8 rows high)
    th = rows if th is None else th
    ry, rx = (-1, 0) if window is None else window
    cy, cx = (0, 0) if center is None else center
    if out is None:
        out = np.zeros((channels, (H if window is None else 2 * ry + 1) * rows, (W if window is None else 2 * rx + 1) * 8), np.uint8)
    screen = np.ascontiguousarray(screen)
    rc = lib.rg_pixels_host(th, None if font is None else np.ascontiguousarray(font).ctypes.data, None if pal is None else np.ascontiguousarray(pal).ctypes.data, channels,
                            H, W, screen.ctypes.data, cy, cx, ry, rx, out.ctypes.data)
    return rc, out


def default_tileset(lib):
    th, font, pal = C.c_int(0), np.zeros(256 * 16, np.uint8), np.zeros((257, 3), np.uint8)
    assert lib.rg_tileset_default(C.byref(th), font.ctypes.data, pal.ctypes.data) == 0
    assert not font[256 * th.value:].any()
    return font[:256 * th.value].reshape(256, th.value).copy(), pal


def full_images(font, pal, screens, channels):
    """full_image for a batch u8 [N, H, W] -> u8 [N, C, H*th, W*8]."""
    N, H, W = screens.shape
    th = font.shape[1]
    ink = np.unpackbits(font[screens], axis=-1).reshape(N, H, W, th, 8).transpose(0, 1, 3, 2, 4).reshape(N, H * th, W * 8).astype(bool)
    g = np.repeat(np.repeat(screens, th, axis=1), 8, axis=2)
    tab = pal if channels == 3 else lum(pal)[:, None]
    return np.stack([np.where(ink, tab[g, c], tab[256, c]) for c in range(channels)], axis=1).astype(np.uint8)


def window_glyphs(screens, centers, ry, rx):
    """u8 [N, 2ry+1, 2rx+1]: the glyphs of each env's window around centers[e] = (cy, cx), ' ' outside the screen.  screens: [N, H, W] or a list of [H_e, W_e]."""
    out = np.full((len(screens), 2 * ry + 1, 2 * rx + 1), 0x20, np.uint8)
    for e, scr in enumerate(screens):
        cy, cx = int(centers[e][0]), int(centers[e][1])
        padded = np.pad(scr, ((ry, ry), (rx, rx)), constant_values=0x20)
        out[e] = padded[cy:cy + 2 * ry + 1, cx:cx + 2 * rx + 1]
    return out


def crop_images(font, pal, screens, channels, centers, ry, rx):
    """The windows of a batch: the rule applied to the windows' glyphs, which is the slice of each padded full image (crop_image says so for one screen)."""
    return full_images(font, pal, window_glyphs(screens, centers, ry, rx), channels)
