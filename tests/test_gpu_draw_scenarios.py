"""The drawn mirrors and every observation pass on constructed states against the second restatement's draw (tests/shadow_turn.py draw_screen / Mirror),
bit for bit.

tests/test_gpu_turn_scenarios.py compares the game state with the Shadow after every key, the mirrors only at the end and only between two handles of the
library.  Here all scenarios of a shape -- the turn scenarios as they are, then the draw scenarios (tests/draw_scenarios.py) -- go into one batch, one env each,
and every LANE, a handle of its own, plays the same keys.  After every key a lane makes only its own observer call and nothing else that reads or flushes the
mirrors, so the pass under test is the one that draws the pending Redraws.  Expected: the Shadow's Mirror (screen, history, status: redrawn only on Redraw,
refreshed only on StatusUpdated), and for the images the oracle's encoders run on that Mirror (oracle.pyoracle.encode_image).  Tolerance 0.

 1  rg_fetch_states, default handle                        mirror_update + k_render
 2  rg_fetch_states under ROGUE_GYM_HIP_NO_MIRROR_UPDATE   k_render, every Redraw
 3  rg_obs_gray(0, no hist)                                k_obs_stream at <= 512 cells, k_obs<gray> elsewhere
 4  rg_obs_symbol(0x1FF, with hist)                        the staged path; status and history planes show the stale status
 5  rg_step_obs_gray                                       on 32x16 the ENC instance of the step kernel and k_obs_resid
 6  rg_step_obs_typed: u8 symbol ids / f16 gray            k_redraw + k_obs_typed (a handle each); refused where H * W is no multiple of 16 / 8: asserted
 7  rg_step_obs_crop_typed: f32 gray / u8 ids              the crop kernel, radii that hang off the grid on every side (a handle each)
 8  rg_obs_bind, then rg_step + rg_obs_gray                the bound tensor
 9  rg_step_obs_pixels: gray / RGB, default tileset        the pixel pass (a handle each)

At the end of every lane rg_fetch_states equals the Mirror.  A scenario whose Shadow died drops out from its death key on (only those that claim it do:
tests/test_draw_scenarios_host.py).  No scenario shows a 'Z' (scenario_config: kinds A..L); the turn scenario "sleepers" shows an 'L', the config's last symbol,
which PlayerState::symbol_image refuses all the same (python/src/lib.rs:96-102): that env's one-hot image must raise, no other may.  No descents: the Shadow has no
generator (tests/test_oracle_shadow.py covers them on the CPU)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import draw_scenarios as ds
import pixel_util as pu
import state_util as su
import typed_util as tu
from oracle.pyoracle import OracleEnv, encode_image
from parity_util import crop_window
from test_gpu_turn_scenarios import make_handle

pytestmark = pytest.mark.gpu

FULL = 0x1FF


class Expected:
    """The scenarios of a shape played once on the Shadow: per key the key bytes, which envs are still compared, and the Mirror of every env."""

    def __init__(self, shape):
        self.shape, self.scs = shape, ds.all_scenarios(shape)
        self.W, self.H = su.SHAPES[shape][:2]
        traces = [ds.Trace(sc) for sc in self.scs]
        # Key 0 of every env is a NoOp, which changes no state (actions.rs:62): the record's pending Redraw (state_util.fill_record) is drawn by the lane's own
        # pass behind it, from the loaded state, as the Mirror drew it.  The scripts follow.
        n, T = len(traces), 1 + max(len(sc.keys) for sc in self.scs)
        self.n, self.T = n, T
        self.keys, self.alive = np.zeros((T, n), np.uint8), np.zeros((T, n), bool)
        self.screen, self.hist = np.full((T, n, self.H, self.W), 32, np.uint8), np.zeros((T, n, self.H, self.W), np.uint8)
        self.status, self.pos = np.zeros((T, n, 10), np.int64), np.zeros((T, n, 2), np.int64)
        for t in range(T):
            for i, tr in enumerate(traces):
                k, f = (".", tr.frames[0]) if t == 0 else tr.step()
                self.keys[t, i] = ord(k)
                if f is not None:
                    self.alive[t, i] = True
                    self.screen[t, i], self.hist[t, i], self.status[t, i], self.pos[t, i] = f.screen, f.hist, f.status, (f.pos[1], f.pos[0])
        self.died = [sc.name for sc, tr in zip(self.scs, traces) if tr.died_at is not None]
        self.stale = sum(f.stale_screen for tr in traces for f in tr.frames), sum(f.stale_status for tr in traces for f in tr.frames)
        self.symbols = OracleEnv(su.scenario_config(shape)).symbols
        self._gray = {}
        # PlayerState::symbol_image refuses a glyph whose symbol is not below symbols - 1 (python/src/lib.rs:96-102): with kinds A..L that is 'L', which the turn
        # scenario "sleepers" shows.  Such an env's one-hot image raises on both sides (as a 'Z' does in tests/test_gpu_obs_oracle.py) and is not compared.
        self.raises = self.alive & (tu.symbol_ids(self.screen) >= self.symbols - 1).any(axis=(2, 3))

    def gray(self, t):
        if t not in self._gray:
            self._gray[t] = np.stack([encode_image(0, self.screen[t, i], self.status[t, i], self.symbols) for i in range(self.n)])
        return self._gray[t]

    def symbol_planes(self, t):
        return np.stack([encode_image(1, self.screen[t, i], self.status[t, i], self.symbols, FULL, self.hist[t, i]) if self.alive[t, i] and not self.raises[t, i] else
                         np.zeros((self.symbols + 10, self.H, self.W), np.float32) for i in range(self.n)])


def where(exp, t, i):
    return "%s env %d (%s) key %d %r" % (exp.shape, i, exp.scs[i].name, t, chr(exp.keys[t, i]))


def text(a):
    return "\n".join(bytes(r).decode("latin-1") for r in a)


def drain(exp, hd, t, one_hot):
    """rg_sync behind a lane's call of key t.  It fails iff an env raised InvalidTile: a one-hot image or an id plane of a screen with a refused glyph.  An env
    that died holds a generated level whose screen the Shadow does not know: from the first death on only the failure that must come is asserted."""
    rc = hd.L.rg_sync(hd.h)
    if one_hot and exp.raises[t].any():
        assert rc != 0, "%s key %d: an env shows a refused glyph and rg_sync reports nothing" % (exp.shape, t)
    elif not one_hot or exp.alive[t].all():
        assert rc == 0, "%s key %d: rg_sync: %s" % (exp.shape, t, hd.L.rg_last_error(hd.h))


def same(exp, lane, what, t, got, want, skip=None):
    """got == want for every env still compared, bit for bit."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s %s: shape %s, expected %s" % (lane, what, got.shape, want.shape)
    live = exp.alive[t] if skip is None else exp.alive[t] & ~skip
    if np.array_equal(got[live], want[live]):
        return
    for i in np.nonzero(live)[0]:
        if not np.array_equal(got[i], want[i]):
            at = tuple(int(v) for v in np.argwhere(got[i] != want[i])[0])
            raise AssertionError("lane %s, %s: %s differs first at %s: %r, the Shadow's Mirror gives %r (%d values differ)\nthe Mirror's screen:\n%s%s" % (
                lane, where(exp, t, i), what, at, got[i][at], want[i][at], int((got[i] != want[i]).sum()), text(exp.screen[t, i]),
                "\nthe handle's:\n" + text(got[i]) if got[i].shape == exp.screen[t, i].shape and got.dtype == np.uint8 else ""))


def dev_empty(hd, shape, dtype):
    import torch

    return torch.empty(shape, dtype=dtype, device="cuda:%d" % hd.device)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def end_check(exp, lane, hd, one_hot=False):
    """rg_fetch_states equals the Mirror: screen, hist, status."""
    t = exp.T - 1
    screen, hist, status, _ = hd.fetch()
    same(exp, lane, "screen at the end", t, screen, exp.screen[t])
    same(exp, lane, "history at the end", t, hist, exp.hist[t])
    same(exp, lane, "status at the end", t, status.astype(np.int64), exp.status[t])
    if one_hot:   # (an id plane raises like a one-hot image, at the next rg_sync: an earlier key's may be pending)
        hd.L.rg_sync(hd.h)
    else:
        drain(exp, hd, t, False)
    hd.close()


def play(exp, lane, hd, observe, one_hot=False):
    """Every key of the batch on one lane; observe(t, keys) steps, makes the lane's observer call and compares."""
    for t in range(exp.T):
        observe(t, np.ascontiguousarray(exp.keys[t]))
    end_check(exp, lane, hd, one_hot)


def lane_handle(exp, env=None):
    hd = make_handle(exp.shape, exp.n, env)
    assert hd.symbols == exp.symbols
    su.inject(hd, [sc.state for sc in exp.scs])
    return hd


# ---- the lanes ------------------------------------------------------------------------------------------------------------------------
def lane_fetch(exp, lane, env=None):
    hd = lane_handle(exp, env)

    def observe(t, keys):
        hd.check(hd.L.rg_step(hd.h, keys.ctypes.data, 0))
        screen, hist, status, _ = hd.fetch()
        same(exp, lane, "screen", t, screen, exp.screen[t])
        same(exp, lane, "history", t, hist, exp.hist[t])
        same(exp, lane, "status", t, status.astype(np.int64), exp.status[t])
    play(exp, lane, hd, observe)


def lane_obs_gray(exp, lane):
    import torch

    hd = lane_handle(exp)
    out = dev_empty(hd, (exp.n, 1, exp.H, exp.W), torch.float32)

    def observe(t, keys):
        hd.check(hd.L.rg_step(hd.h, keys.ctypes.data, 0))
        hd.check(hd.L.rg_obs_gray(hd.h, 0, 0, ptr(out)))
        same(exp, lane, "gray image", t, out.cpu().numpy(), exp.gray(t))
    play(exp, lane, hd, observe)


def lane_obs_symbol(exp, lane):
    import torch

    hd = lane_handle(exp)
    out = dev_empty(hd, (exp.n, exp.symbols + 10, exp.H, exp.W), torch.float32)

    def observe(t, keys):
        hd.check(hd.L.rg_step(hd.h, keys.ctypes.data, 0))
        hd.check(hd.L.rg_obs_symbol(hd.h, FULL, 1, ptr(out)))
        same(exp, lane, "one-hot image with status and history planes", t, out.cpu().numpy(), exp.symbol_planes(t), skip=exp.raises[t])
        drain(exp, hd, t, True)
    play(exp, lane, hd, observe, one_hot=True)


def lane_step_obs_gray(exp, lane):
    import torch

    hd = lane_handle(exp)
    out = dev_empty(hd, (exp.n, 1, exp.H, exp.W), torch.float32)
    if exp.shape == "32x16":   # the pre-streamed encode: helper blocks in the step launch (k_step_w32<ENC>), k_obs_resid behind it
        assert not os.environ.get("ROGUE_GYM_HIP_NO_TAIL_ENCODE") and not os.environ.get("ROGUE_GYM_HIP_LIB")
        helpers = hd.L.rgk_step_enc_helpers(exp.n, 0)
        assert helpers > 0
        print("%s lane %s: the ENC instance runs with %d helper blocks for %d envs" % (exp.shape, lane, helpers, exp.n))

    def observe(t, keys):
        hd.check(hd.L.rg_step_obs_gray(hd.h, keys.ctypes.data, 0, 0, 0, ptr(out)))
        same(exp, lane, "gray image", t, out.cpu().numpy(), exp.gray(t))
    play(exp, lane, hd, observe)


def lane_step_obs_typed(exp, lane, kind, dtype):
    import torch

    hd = lane_handle(exp)
    ids = dtype == tu.RG_OBS_U8
    out = dev_empty(hd, (exp.n, 1, exp.H, exp.W), torch.uint8 if ids else torch.int16)
    if (exp.H * exp.W) % (16 if ids else 8):   # no typed kernels for such a grid: the call is refused and does not step
        keys = np.ascontiguousarray(exp.keys[0])
        assert hd.L.rg_step_obs_typed(hd.h, keys.ctypes.data, 0, kind, dtype, 0, 0, ptr(out)) != 0
        print("%s lane %s: refused, H * W = %d" % (exp.shape, lane, exp.H * exp.W))
        hd.close()
        return

    def observe(t, keys):
        hd.check(hd.L.rg_step_obs_typed(hd.h, keys.ctypes.data, 0, kind, dtype, 0, 0, ptr(out)))
        got = out.cpu().numpy()
        if ids:
            same(exp, lane, "symbol ids", t, got, tu.symbol_ids(exp.screen[t])[:, None])
        else:
            same(exp, lane, "f16 gray image", t, got.view(np.uint16), tu.f16_bits(exp.gray(t)))
    play(exp, lane, hd, observe, one_hot=ids)


def lane_crop(exp, lane, ids):
    import torch

    hd = lane_handle(exp)
    ry, rx = min(47, exp.H), min(159, exp.W)   # beyond the grid on every side from any cell (160x48: the largest window there is)
    out = dev_empty(hd, (exp.n, 1, 2 * ry + 1, 2 * rx + 1), torch.uint8 if ids else torch.float32)
    cen = dev_empty(hd, (exp.n, 2), torch.int32)

    def observe(t, keys):
        hd.check(hd.L.rg_step_obs_crop_typed(hd.h, keys.ctypes.data, 0, 2 if ids else 0, tu.RG_OBS_U8 if ids else tu.RG_OBS_F32, ry, rx, 0, 0, ptr(out), ptr(cen)))
        same(exp, lane, "window centres (cy, cx)", t, cen.cpu().numpy().astype(np.int64), exp.pos[t])
        if ids:
            want = tu.symbol_ids(pu.window_glyphs(exp.screen[t], exp.pos[t], ry, rx))[:, None]
        else:
            g = exp.gray(t)
            want = np.stack([crop_window(g[i], int(exp.pos[t, i, 0]), int(exp.pos[t, i, 1]), ry, rx, 0, 1, False) for i in range(exp.n)])
        same(exp, lane, "window", t, out.cpu().numpy(), want)
    play(exp, lane, hd, observe, one_hot=ids)


def lane_bound(exp, lane):
    import torch

    hd = lane_handle(exp)
    out = dev_empty(hd, (exp.n, 1, exp.H, exp.W), torch.float32)
    hd.check(hd.L.rg_obs_bind(hd.h, 0, 0, 0, ptr(out)))

    def observe(t, keys):
        hd.check(hd.L.rg_step(hd.h, keys.ctypes.data, 0))
        hd.check(hd.L.rg_obs_gray(hd.h, 0, 0, ptr(out)))
        same(exp, lane, "bound gray tensor", t, out.cpu().numpy(), exp.gray(t))
    play(exp, lane, hd, observe)


def lane_pixels(exp, lane, channels):
    import torch

    hd = lane_handle(exp)
    font, pal = pu.default_tileset(hd.L)
    th = font.shape[1]
    out = dev_empty(hd, (exp.n, channels, exp.H * th, exp.W * 8), torch.uint8)
    want = np.zeros(out.shape, np.uint8)
    last = np.zeros((exp.n, exp.H, exp.W), np.uint8)

    def observe(t, keys):
        hd.check(hd.L.rg_step_obs_pixels(hd.h, keys.ctypes.data, 0, channels, ptr(out)))
        changed = [i for i in range(exp.n) if not np.array_equal(last[i], exp.screen[t, i])]   # (pixel_util.full_images of the screens that changed; the others' stand)
        if changed:
            want[changed] = pu.full_images(font, pal, exp.screen[t][changed], channels)
            last[changed] = exp.screen[t][changed]
        same(exp, lane, "pixels", t, out.cpu().numpy(), want)
    play(exp, lane, hd, observe)


LANES = (
    ("1 fetch", lambda e, name: lane_fetch(e, name)),
    ("2 fetch, no mirror update", lambda e, name: lane_fetch(e, name, "ROGUE_GYM_HIP_NO_MIRROR_UPDATE")),
    ("3 obs_gray", lane_obs_gray),
    ("4 obs_symbol FULL + hist", lane_obs_symbol),
    ("5 step_obs_gray", lane_step_obs_gray),
    ("6 step_obs_typed u8 ids", lambda e, name: lane_step_obs_typed(e, name, 2, tu.RG_OBS_U8)),
    ("6 step_obs_typed f16 gray", lambda e, name: lane_step_obs_typed(e, name, 0, tu.RG_OBS_F16)),
    ("7 step_obs_crop_typed f32 gray", lambda e, name: lane_crop(e, name, False)),
    ("7 step_obs_crop_typed u8 ids", lambda e, name: lane_crop(e, name, True)),
    ("8 bound tensor", lane_bound),
    ("9 step_obs_pixels gray", lambda e, name: lane_pixels(e, name, 1)),
    ("9 step_obs_pixels RGB", lambda e, name: lane_pixels(e, name, 3)),
)


@pytest.mark.parametrize("shape", list(su.SHAPES))
def test_mirrors_and_observations_on_constructed_states_equal_the_shadow(shape):
    t0 = time.time()
    exp = Expected(shape)
    assert len(exp.died) == (0 if shape == "160x48" else 2), exp.died
    assert not (exp.screen == ord("Z")).any()
    t_shadow = time.time() - t0
    times = []
    for name, lane in LANES:
        t1 = time.time()
        lane(exp, name)
        times.append("%s %.1f" % (name.split()[0], time.time() - t1))
    print("%s: %d envs (%d of them died), %d keys, %d env-keys compared per lane, %d lanes with 0 differences; frames with a stale screen %d, a stale status %d; "
          "the Shadow %.1f s, lanes [%s] s, %.1f s in all" % (shape, exp.n, len(exp.died), exp.T, int(exp.alive.sum()), len(LANES), exp.stale[0], exp.stale[1], t_shadow,
                                                              ", ".join(times), time.time() - t0))
