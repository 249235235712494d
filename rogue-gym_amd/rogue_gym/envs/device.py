"""HipVecRogueEnv: the HBM-resident fast path.  Same engine and semantics as ParallelRogueEnv
(keys in, auto-reset on terminal, reward = max(0, gold delta)), but actions, observations, rewards
and done flags are PyTorch-ROCm tensors that never leave the GPU, and nothing synchronises with
the host.  With torch.distributed initialised (backend "nccl" = RCCL), envs are sharded across
ranks in contiguous index blocks and `all_gather_obs()` assembles the whole-job batch.
"""
import ctypes as C
import json
import operator
from typing import Iterable, Optional

import numpy as np

from rogue_gym_python import _rogue_gym as inner

from .rogue_env import DungeonType, ImageSetting, RogueEnv, StatusFlag


MONSTER_COLS = inner.MONSTER_COLS  # the int16 columns of a row of HipVecRogueEnv.monsters
OBJECT_COLS = inner.OBJECT_COLS    # the int16 columns of a row of HipVecRogueEnv.objects
Tileset = inner.Tileset


class _DevArray:
    """Zero-copy view of a device buffer owned by the C library (via __cuda_array_interface__)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


class CropView:
    """A player-centred window kept beside an env's main observation (HipVecRogueEnv.add_crop): `obs` [N, C, 2ry+1, 2rx+1] in the view's element
    type and `center` i32 [N, 2], the (y, x) of each window's centre.  Both are rewritten in place whenever the env refreshes its own `obs`."""

    def __init__(self, crop, image_setting, call, obs, center):
        self.crop, self.image_setting, self.obs, self.center = crop, image_setting, obs, center
        self._call = call  # (kind, RG_OBS_* dtype) of rg_obs_crop_typed


class HipVecRogueEnv:
    ACTIONS = RogueEnv.ACTIONS
    MONSTER_COLS = MONSTER_COLS
    OBJECT_COLS = OBJECT_COLS

    def __init__(self, config_dicts: Iterable[dict], max_steps: int = 1000,
                 image_setting: ImageSetting = ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), device: Optional[int] = None,
                 persistent_obs: bool = False, crop=None, obs_dtype=None, symbol_ids: bool = False, action_mask: bool = False, guide=None, guide_secrets: bool = False,
                 episodes: bool = False, scout: bool = False, episode_log: int = 0, monsters=None, monster_cap: int = 4,
                 objects=None, object_kinds: str = "stairs+gold+door", object_cap: int = 8, object_secrets: bool = False,
                 pixels=None, pixel_crop=None, tileset=None,
                 novelty=None, novelty_scope: str = "episode", novelty_crop=None, novelty_slots: int = 1024, novelty_global_slots: int = 1 << 22,
                 archive=None, archive_auto: bool = True):
        """persistent_obs (opt-in; image settings without status planes and history plane): `self.obs` is BOUND to the stepper (rg_obs_bind) -- every step
        keeps it current in place, rewriting only the envs whose screen changed; its contents are bit-identical to the unbound encode's.  The caller
        must not write to `self.obs`.

        crop (None, r or (ry, rx)): `self.obs` is the player-centred window f32 [N, C, 2ry+1, 2rx+1] of the image instead of the whole screen, padded
        with blank cells past the screen edge (rg_obs_crop), and `self.crop_center` i32 [N, 2] holds each window's centre (y, x), rewritten with every
        observation.  The window has one size for every env, so a batch whose envs differ in screen size can be built too.  Not with persistent_obs.

        obs_dtype (None, torch.float32, torch.float16 or torch.bfloat16): the element type of `self.obs`.  The 16-bit images are written by the encode pass
        itself (rg_obs_typed) and are bit-identical to the f32 image's `.to(obs_dtype)`; None / float32 is the f32 path.

        symbol_ids (needs DungeonType.SYMBOL, StatusFlag.EMPTY and obs_dtype None): `self.obs` is uint8 [N, 1 + hist, H, W] -- plane 0 holds each cell's symbol
        id (the one-hot image's argmax(1); ' ' is 0), what an embedding layer indexes with -- instead of the one-hot image.

        Neither with crop or persistent_obs (those are f32 only); a typed window BESIDE `obs` is a crop view: add_crop().

        action_mask (opt-in): `self.action_mask` is a bool tensor [N, len(ACTIONS)] on the device -- entry [i, a] says whether ACTIONS[a] would do anything
        for env i now (rg_action_mask: the engine's own move test; False = "can't move", "no downstairs") -- rewritten in place by everything that
        refreshes `obs`.  One small launch more per step, no host trip; it works on every env this class builds.  False: `self.action_mask` is None and
        nothing is added to any call.  legal_mask() and sample_keys() work either way.

        guide (opt-in; "stairs", "gold" or "stairs+gold"): `self.guide_keys` is a uint8 tensor [N] on the device -- for each env the key that takes it one
        move closer to the nearest goal cell, ready for step_keys: '>' on the stairs, 's' where no goal can be reached, '.' on a gold goal's own cell
        or in the Grave modal -- and `self.guide_dist` an int32 tensor [N], the number of moves to that cell, -1 = unreachable (rg_path: the engine's own
        move test, shortest paths from the goal cells).  Both are rewritten in place by everything that refreshes `obs`: one launch more per step, no
        host trip.  The guide is PRIVILEGED: it sees stairs, gold and passages the player has not discovered -- a teacher, a shaping potential or a
        critic input, not an observation.  None: both attributes are None and nothing is added to any call.  path() works either way.

        guide_secrets (with a guide): the guide plans THROUGH hidden and locked cells and answers 's' when the next cell of the route is one (rg_route with
        RG_ROUTE_SECRETS in place of rg_path), so an env whose stairs lie behind a secret searches in the right place instead of where it stands.  False:
        the guide is rg_path's, byte for byte and launch for launch.

        guide="explore" is the explorer that is NOT privileged: it plans on the player's own map only (the cells that are drawn or in view), towards the
        stairs once they are on it, else towards the nearest known cell beside an unknown one, and searches when it stands on such a cell -- a hidden
        passage cell is what stays unknown beside it (rg_route: goals stairs, fallback frontier, mode known).  `self.guide_tier` is a uint8
        tensor [N]: 0 = the stairs answered, 1 = the frontier, 255 = neither (the key is 's' then); None for every other guide.

        episodes (opt-in): episode accounting on the device (rg_episode_update, one small launch behind every step, no host trip).  The stepper rebuilds a
        finished env inside the step, so `done` and `reward` are all that is left of the old game; with episodes=True these device tensors [N] say the rest:
        `ep_return` f32, `ep_length` and `ep_depth` i32 of the running episode; `died` and `time_limit` bool, why an env whose `done` is set ended (a death
        on the very last allowed step is reported as a time limit); `last_return`, `last_length`, `last_depth` and `last_cause` uint8 (1 died, 2 time limit,
        3 cut by reset() / reset_envs()) of each env's last finished episode.  scout=True (implies episodes): `scout` f32 [N] is the number of map cells the
        step made known for the first time on the env's level -- NLE's "scout" reward, 0 in the step that starts a new game -- and `seen_bits` uint8 [N, SB]
        the bitmap behind it (bit b of byte j: cell 8 j + b).  episode_log (> 0, implies episodes): that many finished episodes are kept on the device
        between two pop_episodes() calls.  Without any of the three every one of these attributes is None and nothing is added to any call.  Not for
        batches with config groups.

        monsters (opt-in; "shown" or "all"): `self.monsters` is an int16 tensor [N, monster_cap, 8] on the device -- for each env the nearest monster_cap
        (1 .. 16) monsters as rows of MONSTER_COLS (tile, dx, dy, cheb, shown, active, hp, slot; a row whose tile is 0 is empty), nearest first -- and
        `self.threat` an int32 tensor [N, 4]: shown monsters next to the player, the distance of the nearest shown one (-1 = none), a bit per move key of
        ACTIONS[1:9] whose target cell holds a shown monster (positional only: AND it with `action_mask` for legality), and the number of monsters that
        qualify (rg_monsters).  Both are rewritten in place by everything that refreshes `obs`: one small launch more per step, no host trip.  "shown"
        lists what a redraw of the screen would show now -- read off the game state, so between two redraws it is more current than the image.  "all"
        lists every living monster of the level with its hit points and is PRIVILEGED, as the guide is.  It works on every env this class builds, config
        groups and mixed sizes included.  None: both attributes are None and nothing is added to any call.  monster_table() works either way.

        objects (opt-in; "known" or "all"): `self.objects` is an int16 tensor [N, object_cap, 8] on the device -- for each env the stairs, gold and doors of
        its level (object_kinds: names joined with '+'; "frontier", the known cells beside an unknown one, with "known" only) as rows of OBJECT_COLS (kind
        bits 1 stairs | 2 gold | 4 door | 8 frontier, dx, dy, walk, x, y, cheb, 0; a row whose kind is 0 is empty), ordered by `walk`, the number of moves
        it takes to walk there (then y, x), the first object_cap (1 .. 32) of them -- and `self.object_count` an int32 tensor [N, 4], the cells of each
        kind on the level, listed or not (rg_objects: one search from the player over rg_route's graph; an object that cannot be reached is counted and
        not listed).  Both are rewritten in place by everything that refreshes `obs`: one launch more per step, no host trip.  "known" reads the player's
        own map only (the cells that are drawn or in view): nothing is privileged.  "all" reads the level itself and is PRIVILEGED, as the guide is.
        object_secrets: the walk goes THROUGH hidden and locked cells, as guide_secrets' routes do.  A row's (y, x) is what route(goal=None, cells=...)
        takes.  It works on every env this class builds, config groups and mixed sizes included.  None: both attributes are None and nothing is added to
        any call.  object_table() works either way.

        pixels (opt-in; "gray" or "rgb"): `self.pixels` is a uint8 tensor [N, C, hp, wp] on the device, C = 1 or 3 -- every env's screen drawn through
        `tileset` (a Tileset: a bitmap font of 8-pixel-wide glyphs and a palette; None = the built-in 8 x 8 one), planar, hp = H * th and wp = W * 8
        (rg_obs_pixels).  pixel_crop (None, r or (ry, rx)): the player-centred window instead, hp = (2ry+1) * th and wp = (2rx+1) * 8, cells past the
        screen edge drawn as ' ' through the tileset, and `self.pixel_center` i32 [N, 2] holds each window's centre (rg_obs_pixels_crop) -- an 11 x 11
        window of 8 x 8 tiles is 88 x 88 pixels, 7.7 KB per env in gray, the form to train on; the whole-screen RGB image of an 80 x 24 env is 368 KB.
        With a crop it works on every env this class builds; the whole screen not on batches with config groups or mixed sizes.  Rewritten in place by
        everything that refreshes `obs`: one launch more per step, no host trip.  A learner does `.float() / 255` itself.  None: both attributes are None
        and nothing is added to any call.  render_pixels() and frame() work either way.

        novelty (None, "pos", "screen" or "crop"): count-based novelty on the device (rg_novelty_update, a small pass behind every step, no host trip) -- visit
        counts of hashed states, the signal of RIDE's episodic count, of the `count == 1` gate of NovelD / BeBold and of lifetime count bonuses.  What is
        hashed: "pos" the player's cell, "screen" the rows of the screen that show tiles, "crop" their player-centred window of novelty_crop = r or (ry, rx);
        the dungeon level is hashed in.  `novelty_hash` int64 [N] is the hash (the u64 bit pattern), kept current with `obs`.  novelty_scope "episode":
        `visit_count` int32 [N], how often the env has shown this state in its running episode, this step included, from a table of novelty_slots slots per
        env (a power of two, 64 .. 65 536; 16 B x slots x N of device memory -- 1 GB at 1 024 slots and 65 536 envs); "global": `visit_count_global` int32 [N],
        the count over every env and episode of this object since it was built or novelty_clear() was called, from one table of novelty_global_slots
        slots (a power of two, 1 024 .. 2^28), as it stands after the whole step; "both": both.  A visit that finds its table full counts 0 and is
        reported by novelty_stats().  step*, reset, reset_envs, load_state and clone_state keep all three current.  The bonus is one tensor op of the
        learner's: visit_count.float().rsqrt(), or visit_count == 1.  None: the three attributes are None and nothing is added to any call.  Not for
        batches with config groups.

        archive (None or cells, a power of two, 1 024 .. 2^24): the cell archive on the device (rg_archive_update) -- per hashed state the best state record
        any env has offered, Go-Explore's archive, and archive_restore() the way back into it.  An offer is (key, score, steps): a larger score beats a
        smaller, at equal scores fewer steps of the running episode beat more, at equal both the lowest env of the call wins and a later call replaces
        nothing.  `self.archive` carries the table as tensors, per slot `key` int64 [cells] (0 = empty), `score`, `steps`, `seen` (the offers the key
        ever got), `chosen` (the restores from it), `when` (the update call that last wrote it, from 1) int32 [cells], `records` uint8 [cells, state_bytes],
        and per env `slot` int32 [N] (-1: the offer was dropped, the table is full there), `stored` bool [N] (this env's record was written by the last
        update), `score_in`, `steps_in` int32 [N].  cells x state_bytes of device memory: 192 MB at 2^14 cells of the mini config.  With archive_auto
        (which needs novelty=) every step* offers each env's state behind the novelty pass under its novelty hash with its gold as the score; without,
        archive_update() is the explicit call.  None: `self.archive` is None and nothing is added to any call.  Not for batches with config groups."""
        import torch

        self.torch = torch
        self._views = []       # the crop views (add_crop): what _refresh_views encodes first, in this order
        self._refresh = []     # ... and then calls: the refresh call of each optional feature, registered by its _setup_* in the order they run below
        self._after_step = []  # what _step_keys calls behind the step's observation: the episode, novelty and archive updates, registered the same way
        self._scratch = {}
        self._draw = 0  # sample_keys: the draw counter of calls that give none
        cfgs = [d if isinstance(d, str) else json.dumps(d) for d in config_dicts]
        self._h = inner._Handle(cfgs, max_steps, auto_reset=True, device=device)
        self.device = torch.device("cuda", self._h.device)
        self.num_envs = self._h.n
        self.image_setting = image_setting
        self.symbols = self._h.symbols
        self.height, self.width = self._h.height, self._h.width
        L, h, n = self._h.L, self._h.h, self.num_envs
        with torch.cuda.device(self.device):
            self._h.check(L.rg_set_stream(h, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            self._action_keys = torch.tensor([ord(a) for a in self.ACTIONS], dtype=torch.uint8, device=self.device)
        self._setup_obs(crop, obs_dtype, symbol_ids, persistent_obs)
        p = C.c_void_p()
        for name, get, shape, typestr in (("reward", L.rg_reward, (n,), "<f4"), ("done", L.rg_done, (n,), "|b1"), ("flags", L.rg_flags, (n,), "<i4"), ("status", L.rg_status, (n, 10), "<i4")):
            self._h.check(get(h, C.byref(p)))
            setattr(self, name, self._dev_view(p.value, shape, typestr))
        self._screen = None
        if self.crop is None:  # (with a crop the batch may mix screen sizes: no screen tensor then, `screen` raises)
            self._screen_view()
        self._setup_pixels(pixels, pixel_crop, tileset)
        self._setup_action_mask(action_mask)
        self._setup_guide(guide, guide_secrets)
        self._setup_monsters(monsters, monster_cap)
        self._setup_objects(objects, object_kinds, object_secrets, object_cap)
        self._setup_episodes(bool(episodes) or bool(scout) or int(episode_log) > 0, bool(scout), int(episode_log))
        if self.persistent_obs:
            self._h.check(L.rg_obs_bind(h, int(self._sym), image_setting.status.value, int(image_setting.includes_hist), C.c_void_p(self.obs.data_ptr())))
        self._encode()
        self._setup_novelty(novelty, novelty_scope, novelty_crop, novelty_slots, novelty_global_slots)  # (behind the first encode: the mirrors are drawn)
        self._setup_archive(archive, archive_auto)

    # ---- what the argument checks share ----
    def _dev_view(self, ptr, shape, typestr):
        """A tensor over a device array that the library owns (zero-copy); None for a null pointer: the handle has no such array."""
        if not ptr:
            return None
        with self.torch.cuda.device(self.device):
            return self.torch.as_tensor(_DevArray(ptr, shape, typestr), device=self.device)

    def _dev_arg(self, call, name, t, dtypes, shape, contiguous=False):
        """The argument `name` of `call`, checked: a tensor of one of `dtypes` and of `shape` on this env's device.  contiguous=True (a tensor to write into)
        demands a contiguous one; otherwise the contiguous form of `t` is returned."""
        torch = self.torch
        if (not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.device != self.device or tuple(t.shape) != tuple(shape)
                or (contiguous and not t.is_contiguous())):
            raise ValueError("%s: %s must be a %s%s tensor %s on %s, got %s" % (
                call, name, "contiguous " if contiguous else "", " / ".join(str(d).replace("torch.", "") for d in dtypes), list(shape), self.device,
                "%s %s on %s" % (list(t.shape), t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t).__name__))
        return t if contiguous else t.contiguous()

    def _obs_call(self, st, obs_dtype, symbol_ids):
        """((kind, RG_OBS_* dtype) of the typed observation calls -- dtype 0 is f32 --, channels, torch dtype) of an image of setting `st` with the obs_dtype and
        symbol_ids of the constructor or of add_crop."""
        torch = self.torch
        if obs_dtype not in (None, torch.float32, torch.float16, torch.bfloat16):
            raise ValueError("obs_dtype must be None, torch.float32, torch.float16 or torch.bfloat16, got %r" % (obs_dtype,))
        sym = st.dungeon == DungeonType.SYMBOL
        if symbol_ids:
            if not sym or st.status.value != 0 or obs_dtype is not None:
                raise ValueError("symbol_ids=True needs DungeonType.SYMBOL, StatusFlag.EMPTY and obs_dtype=None (the ids are uint8), got %s, status %r, obs_dtype %r"
                                 % (st.dungeon, st.status, obs_dtype))
            return (2, 3), 1 + int(st.includes_hist), torch.uint8
        call = (int(sym), 1 if obs_dtype == torch.float16 else 2 if obs_dtype == torch.bfloat16 else 0)
        channels = self._h.L.rg_obs_channels(self._h.h, int(sym), st.status.value, int(st.includes_hist))
        return call, channels, torch.float32 if obs_dtype is None else obs_dtype

    # ---- the optional features: each checks its arguments, makes its tensors and registers its refresh call in one place ----
    def _setup_obs(self, crop, obs_dtype, symbol_ids, persistent_obs):
        """`obs` and `crop_center`; _encode_obs and _step_keys keep them current."""
        torch, st = self.torch, self.image_setting
        self._sym = st.dungeon == DungeonType.SYMBOL
        call, self.channels, dtype = self._obs_call(st, obs_dtype, symbol_ids)
        if call[1] and (crop is not None or persistent_obs):
            raise ValueError("%s cannot be combined with %s: the crop and the bound observation tensor are float32 only"
                             % ("symbol_ids=True" if symbol_ids else "obs_dtype=%s" % (obs_dtype,), "crop" if crop is not None else "persistent_obs=True"))
        if crop is not None and persistent_obs:
            raise ValueError("crop and persistent_obs cannot be combined: the bound observation tensor is the whole screen")
        self.crop = None if crop is None else self._crop_radii(crop)
        self.persistent_obs = bool(persistent_obs)
        self._typed = call if call[1] else None  # (kind, RG_OBS_* dtype) of rg_obs_typed, or None: the f32 calls
        oh, ow = (self.height, self.width) if self.crop is None else (2 * self.crop[0] + 1, 2 * self.crop[1] + 1)
        with torch.cuda.device(self.device):
            self.obs = torch.empty((self.num_envs, self.channels, oh, ow), dtype=dtype, device=self.device)
            self.crop_center = None if self.crop is None else torch.zeros((self.num_envs, 2), dtype=torch.int32, device=self.device)

    def _setup_pixels(self, pixels, pixel_crop, tileset):
        torch = self.torch
        if pixels not in (None, "gray", "rgb"):
            raise ValueError("pixels must be None, 'gray' or 'rgb', got %r" % (pixels,))
        if pixels is None and pixel_crop is not None:
            raise ValueError("pixel_crop needs pixels='gray' or 'rgb'")
        self.tileset = None
        self.pixels = self.pixel_center = None
        if tileset is not None or pixels is not None:
            self.set_tileset(tileset)
        if pixels is None:
            return
        crop = None if pixel_crop is None else self._crop_radii(pixel_crop)
        channels = 3 if pixels == "rgb" else 1
        self.pixels = self._pixel_tensor(self.num_envs, channels, crop)
        if crop is not None:
            with torch.cuda.device(self.device):
                self.pixel_center = torch.zeros((self.num_envs, 2), dtype=torch.int32, device=self.device)
        self._refresh.append(lambda: self._pixel_call(channels, crop, self.pixels, self.pixel_center))

    def _setup_action_mask(self, on):
        torch, hd = self.torch, self._h
        self._mask_u8 = torch.zeros((self.num_envs, len(self.ACTIONS)), dtype=torch.uint8, device=self.device) if on else None  # (sample_keys writes it too)
        self.action_mask = None if self._mask_u8 is None else self._mask_u8.view(torch.bool)
        if on:
            self._refresh.append(lambda: hd.check(hd.L.rg_action_mask(hd.h, None, 0, C.c_void_p(self._mask_u8.data_ptr()), None, 0, 0)))

    def _setup_guide(self, guide, secrets):
        torch, hd = self.torch, self._h
        if guide is not None and (not isinstance(guide, str) or (guide not in inner.PATH_GOALS and guide != "explore")):
            raise ValueError("guide must be None or one of %s, 'explore', got %r" % (", ".join(repr(g) for g in inner.PATH_GOALS), guide))
        if secrets and guide is None:
            raise ValueError("guide_secrets=True needs a guide")
        self.guide, self.guide_secrets = guide, bool(secrets)
        self.guide_keys = self.guide_dist = self.guide_tier = None
        if guide is None:
            return
        self.guide_keys = torch.zeros((self.num_envs,), dtype=torch.uint8, device=self.device)
        self.guide_dist = torch.zeros((self.num_envs,), dtype=torch.int32, device=self.device)
        if guide == "explore" or secrets:  # rg_route in place of rg_path
            goals, fb, mode = inner._route_args(*inner.EXPLORE) if guide == "explore" else inner._route_args(guide, None, True, False)
            if guide == "explore":
                self.guide_tier = torch.zeros((self.num_envs,), dtype=torch.uint8, device=self.device)
            self._refresh.append(lambda: hd.check(hd.L.rg_route(hd.h, goals, fb, mode, None, C.c_void_p(self.guide_dist.data_ptr()), C.c_void_p(self.guide_keys.data_ptr()),
                                                                None if self.guide_tier is None else C.c_void_p(self.guide_tier.data_ptr()))))
        else:
            goals = inner.PATH_GOALS[guide]
            self._refresh.append(lambda: hd.check(hd.L.rg_path(hd.h, goals, None, None, C.c_void_p(self.guide_dist.data_ptr()), C.c_void_p(self.guide_keys.data_ptr()))))

    def _setup_monsters(self, monsters, cap):
        torch, hd = self.torch, self._h
        self.monsters = self.threat = None
        if monsters is None:
            return
        mode, cap = inner._monster_args(monsters, cap)
        with torch.cuda.device(self.device):
            self.monsters = torch.zeros((self.num_envs, cap, len(self.MONSTER_COLS)), dtype=torch.int16, device=self.device)
            self.threat = torch.zeros((self.num_envs, 4), dtype=torch.int32, device=self.device)
        self._refresh.append(lambda: hd.check(hd.L.rg_monsters(hd.h, mode, cap, C.c_void_p(self.monsters.data_ptr()), C.c_void_p(self.threat.data_ptr()))))

    def _setup_objects(self, objects, kinds, secrets, cap):
        torch, hd = self.torch, self._h
        self.objects = self.object_count = None
        if objects is None:
            return
        if not isinstance(objects, str) or objects not in ("known", "all"):
            raise ValueError("objects must be None, 'known' or 'all', got %r" % (objects,))
        kw, mode, cap = inner._object_args(kinds, objects == "known", bool(secrets), cap)
        with torch.cuda.device(self.device):
            self.objects = torch.zeros((self.num_envs, cap, len(self.OBJECT_COLS)), dtype=torch.int16, device=self.device)
            self.object_count = torch.zeros((self.num_envs, 4), dtype=torch.int32, device=self.device)
        self._refresh.append(lambda: hd.check(hd.L.rg_objects(hd.h, kw, mode, cap, C.c_void_p(self.objects.data_ptr()), C.c_void_p(self.object_count.data_ptr()))))

    def _setup_novelty(self, what, scope, crop, slots, gslots):
        hd, n = self._h, self.num_envs
        self.novelty, self.novelty_hash, self.visit_count, self.visit_count_global = what, None, None, None
        self._nov_args = None  # the arguments of rg_novelty_enable, None = no novelty
        if what is None:
            if crop is not None:
                raise ValueError("novelty_crop needs novelty='crop'")
            return
        if not isinstance(what, str) or what not in inner.NOVELTY_WHAT:
            raise ValueError("novelty must be None, 'pos', 'screen' or 'crop', got %r" % (what,))
        if not isinstance(scope, str) or scope not in inner.NOVELTY_SCOPE:
            raise ValueError("novelty_scope must be 'episode', 'global' or 'both', got %r" % (scope,))
        if (what == "crop") != (crop is not None):
            raise ValueError("novelty_crop goes with novelty='crop' and only with it, got novelty=%r, novelty_crop=%r" % (what, crop))
        ry, rx = (0, 0) if crop is None else self._crop_radii(crop)
        args = (inner.NOVELTY_WHAT[what], inner.NOVELTY_SCOPE[scope], ry, rx, operator.index(slots), operator.index(gslots))
        hd.check(hd.L.rg_novelty_enable(hd.h, *args))
        self._nov_args = args
        a = inner.RgNoveltyArrays()
        hd.check(hd.L.rg_novelty_arrays(hd.h, C.byref(a)))
        self.novelty_hash, self.visit_count, self.visit_count_global = (self._dev_view(ptr, (n,), t) for ptr, t in ((a.hash, "<i8"), (a.count, "<i4"), (a.gcount, "<i4")))
        self._after_step.append(lambda: hd.check(hd.L.rg_novelty_update(hd.h)))  # the visit of the state a step left, behind its observation: the mirrors are drawn

    def _novelty_cut(self, ptr=None, k=0, on_dev=0, mask=None):
        """The envs a reset or a load replaced (a list, a mask, or every env) start a new episode and count the state they show now."""
        if self._nov_args is not None:
            self._h.check(self._h.L.rg_novelty_cut(self._h.h, ptr, k, on_dev, None if mask is None else C.c_void_p(mask.data_ptr())))

    def novelty_stats(self):
        """dict of occupied_global (slots of the global table in use), dropped_global, dropped_episode (visits that found their table full) and calls.  It
        waits for the stream.  Needs novelty."""
        if self._nov_args is None:
            raise ValueError("novelty_stats needs novelty")
        out = (C.c_uint64 * 4)()
        self._h.check(self._h.L.rg_novelty_stats(self._h.h, out))
        return dict(zip(inner.NOVELTY_STATS, (int(v) for v in out)))

    def novelty_table(self):
        """(hashes numpy uint64 [K], counts numpy uint32 [K]): the occupied slots of the global table sorted by hash -- a visitation histogram.  It waits for
        the stream.  Needs novelty with scope 'global' or 'both'."""
        if self._nov_args is None or not self._nov_args[1] & inner.RG_NOV_GLOBAL:
            raise ValueError("novelty_table needs novelty with novelty_scope 'global' or 'both'")
        L, h, n = self._h.L, self._h.h, C.c_int(0)
        self._h.check(L.rg_novelty_table_read(h, None, None, 0, C.byref(n)))
        hashes, counts = np.zeros(max(n.value, 1), np.uint64), np.zeros(max(n.value, 1), np.uint32)
        self._h.check(L.rg_novelty_table_read(h, hashes.ctypes.data, counts.ctypes.data, hashes.size, C.byref(n)))
        return hashes[:n.value], counts[:n.value]

    def novelty_clear(self):
        """Empty the global table and zero the counters of novelty_stats(); the episodic tables stay.  Needs novelty."""
        if self._nov_args is None:
            raise ValueError("novelty_clear needs novelty")
        self._h.check(self._h.L.rg_novelty_clear(self._h.h))

    # ---- the cell archive (rg_archive_*; the rule: csrc/rg_archive.h) ----
    class Archive:
        """The archive's tensors (HipVecRogueEnv.archive): views of the library's device arrays, rewritten in place by every update."""
        __slots__ = ("cells", "key", "score", "steps", "seen", "chosen", "when", "records", "slot", "stored", "score_in", "steps_in")

    def _setup_archive(self, cells, auto):
        hd, n, view = self._h, self.num_envs, self._dev_view
        self.archive = None
        if cells is None:
            return
        cells = operator.index(cells)
        if auto and self._nov_args is None:
            raise ValueError("archive_auto=True needs novelty= (the keys are the novelty hashes); pass archive_auto=False and call archive_update(keys=...)")
        hd.check(hd.L.rg_archive_enable(hd.h, cells))
        a = inner.RgArchiveArrays()
        hd.check(hd.L.rg_archive_arrays(hd.h, C.byref(a)))
        A = self.Archive()
        A.cells = cells
        A.key = view(a.key, (cells,), "<i8")
        for k in ("score", "steps", "seen", "chosen", "when"):
            setattr(A, k, view(getattr(a, k), (cells,), "<i4"))
        A.records = view(a.records, (cells, self.state_bytes), "|u1")
        A.slot, A.stored = view(a.slot, (n,), "<i4"), view(a.stored, (n,), "|b1")
        A.score_in, A.steps_in = view(a.score_in, (n,), "<i4"), view(a.steps_in, (n,), "<i4")
        self.archive = A
        if auto:  # every step offers the state it left to its cell, under the hash the novelty update just made
            self._after_step.append(lambda: hd.check(hd.L.rg_archive_update(hd.h, None, None, None)))

    def _archive_need(self, what):
        if self.archive is None:
            raise ValueError("%s needs archive=" % what)

    def archive_update(self, keys=None, score=None, mask=None):
        """Offer every env's present state to the archive (rg_archive_update; asynchronous, no host trip).  keys: int64 device tensor [N], the cells -- None
        takes `novelty_hash` (needs novelty=); a learner's own keys can be the hash xor a per-seed salt, which keeps the cells of different dungeons apart.
        score: int32 device tensor [N], larger is better -- None takes the env's gold.  mask: bool / uint8 device tensor [N], the envs that offer -- None:
        all.  Afterwards archive.slot / archive.stored say where each env's key lives and whose record was written."""
        torch = self.torch
        self._archive_need("archive_update")
        if keys is None and self._nov_args is None:
            raise ValueError("archive_update: keys=None takes the novelty hash, which needs novelty=")
        args = [None if t is None else self._dev_arg("archive_update", name, t, dtypes, (self.num_envs,))
                for t, name, dtypes in ((keys, "keys", (torch.int64,)), (score, "score", (torch.int32,)), (mask, "mask", (torch.bool, torch.uint8)))]
        self._h.check(self._h.L.rg_archive_update(self._h.h, *(None if t is None else C.c_void_p(t.data_ptr()) for t in args)))

    def archive_sample(self, k, weights="seen", generator=None):
        """int32 [k] on the device: k occupied slots drawn with replacement -- weights "seen": Go-Explore's 1 / sqrt(seen + 1), "uniform", or a float tensor
        [cells] of the caller's (empty slots never drawn).  Plain torch ops (one multinomial over the table), not a kernel of the library; it is meant for the
        few hundred draws between exploration phases, not for every step."""
        torch = self.torch
        self._archive_need("archive_sample")
        A = self.archive
        occupied = A.key != 0
        if isinstance(weights, torch.Tensor):
            if tuple(weights.shape) != (A.cells,) or weights.device != self.device:
                raise ValueError("archive_sample: a weight tensor must be [%d] on %s" % (A.cells, self.device))
            w = weights.to(torch.float32)
        elif weights == "seen":
            w = (A.seen.to(torch.float32) + 1.0).rsqrt()
        elif weights == "uniform":
            w = torch.ones((A.cells,), dtype=torch.float32, device=self.device)
        else:
            raise ValueError("archive_sample: weights must be 'seen', 'uniform' or a tensor, got %r" % (weights,))
        w = torch.where(occupied, w, torch.zeros_like(w))
        return torch.multinomial(w, operator.index(k), replacement=True, generator=generator).to(torch.int32)

    def archive_restore(self, slots, env_ids=None):
        """Restore envs env_ids (default: envs 0 .. len(slots)-1 when that is every env) from the records of archive slots `slots` (int32 device tensor, a
        list or a numpy array; env_ids of the same kind) -- rg_archive_restore: the records go through load_state's own path, `chosen` of each slot taken
        grows by 1, and an empty slot leaves its env unchanged and makes check_errors() raise.  Then what follows a load: the restored envs start a new
        episode of visit counts and, with episodes=True, of the accounting (the running one ends with cause 3), and the observations are re-encoded.
        Returns the observation batch."""
        torch = self.torch
        self._archive_need("archive_restore")
        on_dev = isinstance(slots, torch.Tensor) and slots.device.type == "cuda"
        if env_ids is not None and (isinstance(env_ids, torch.Tensor) and env_ids.device.type == "cuda") != on_dev:
            raise ValueError("archive_restore: slots and env_ids must both be device tensors or both be host lists")
        if on_dev:
            st = slots.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
            sp, ks = C.c_void_p(st.data_ptr()), int(st.numel())
        else:
            st = np.ascontiguousarray(np.asarray(slots.numpy() if isinstance(slots, torch.Tensor) else slots, dtype=np.int64).reshape(-1).astype(np.int32))
            sp, ks = C.c_void_p(st.ctypes.data), int(st.size)
        ptr, k, dev_ids, _keep = self._state_ids(env_ids, unique=True)
        if k != ks:
            raise ValueError("archive_restore: %d slots for %d envs" % (ks, k))
        L, h = self._h.L, self._h.h
        if k:
            self._h.check(L.rg_archive_restore(h, sp, ptr, k, int(on_dev)))
            if self._episodes:
                self._h.check(L.rg_episode_cut(h, ptr, k, dev_ids, None, 1))
        obs = self._encode()
        if k:
            self._novelty_cut(ptr, k, dev_ids)
        return obs

    def archive_stats(self):
        """dict of occupied (slots in use), dropped (offers that found the table full), written (records written) and calls (updates).  It waits for the
        stream.  Needs archive=."""
        self._archive_need("archive_stats")
        out = (C.c_uint64 * 4)()
        self._h.check(self._h.L.rg_archive_stats(self._h.h, out))
        return dict(zip(inner.ARCHIVE_STATS, (int(v) for v in out)))

    def archive_clear(self):
        """Empty the archive: the table, the records and the counters of archive_stats().  Needs archive=."""
        self._archive_need("archive_clear")
        self._h.check(self._h.L.rg_archive_clear(self._h.h))

    _EP_NAMES = ("ep_return", "ep_length", "ep_depth", "died", "time_limit", "last_return", "last_length", "last_depth", "last_cause", "scout", "seen_bits")

    def _setup_episodes(self, on, scout, log_cap):
        hd, n, view = self._h, self.num_envs, self._dev_view
        self._episodes, self._ep_log_cap = on, log_cap
        for k in self._EP_NAMES:
            setattr(self, k, None)
        if not on:
            return
        if log_cap < 0:
            raise ValueError("episode_log must be >= 0, got %d" % log_cap)
        hd.check(hd.L.rg_episode_enable(hd.h, inner.RG_EP_STATS | (inner.RG_EP_SCOUT if scout else 0), log_cap))
        a = inner.RgEpisodeArrays()
        hd.check(hd.L.rg_episode_arrays(hd.h, C.byref(a)))
        self.ep_return, self.ep_length, self.ep_depth = view(a.ret, (n,), "<f4"), view(a.len, (n,), "<i4"), view(a.depth, (n,), "<i4")
        self.died, self.time_limit = view(a.died, (n,), "|b1"), view(a.time_limit, (n,), "|b1")
        self.last_return, self.last_length, self.last_depth = view(a.last_return, (n,), "<f4"), view(a.last_length, (n,), "<i4"), view(a.last_depth, (n,), "<i4")
        self.last_cause = view(a.last_cause, (n,), "|u1")
        self.scout, self.seen_bits = view(a.scout, (n,), "<f4"), view(a.seen, (n, a.seen_bytes), "|u1")
        self._after_step.append(lambda: hd.check(hd.L.rg_episode_update(hd.h)))  # the accounting of a step, on the mirrors and cells as it left them

    def cut_episodes(self, env_ids=None, mask=None, record=False):
        """Tell the episode accounting that the caller overwrote envs (load_state / clone_state, which leave it alone): the lanes of env_ids (a list, a numpy
        array or a device tensor, without duplicates), of mask (a bool / uint8 device tensor [num_envs]) or -- both None -- of every env start anew from the
        game that stands in them now, `ep_length` from that game's own step counter.  record=True first finishes the running episode of each (if it has
        played a step) with cause 3, as reset() and reset_envs() do.  Needs episodes=True."""
        if not self._episodes:
            raise ValueError("cut_episodes needs episodes=True")
        ptr, k, on_dev, mask, _keep = self._ids_or_mask("cut_episodes", env_ids, mask, one=False)
        if env_ids is not None and k == 0:
            return
        self._h.check(self._h.L.rg_episode_cut(self._h.h, ptr, k, on_dev, None if mask is None else C.c_void_p(mask.data_ptr()), int(bool(record))))

    def pop_episodes(self):
        """The episodes finished since the last call, as a dict of numpy arrays in (serial, env) order -- serial (the ordinal of the step, reset or cut since
        the env was built, from 1), env, ret, length, depth, cause, scout (the episode's scout sum) -- plus `dropped`, the number that found the log full.
        The only host trip of the accounting: it waits for the stream.  Needs episode_log > 0."""
        if not self._episodes or self._ep_log_cap <= 0:
            raise ValueError("pop_episodes needs episode_log > 0")
        buf = np.zeros(self._ep_log_cap, dtype=np.dtype(inner.EPISODE_REC))
        n, dropped = C.c_int(0), C.c_uint64(0)
        self._h.check(self._h.L.rg_episode_log_read(self._h.h, buf.ctypes.data, self._ep_log_cap, C.byref(n), C.byref(dropped)))
        out = {k: buf[k][:n.value].copy() for k in ("serial", "env", "ret", "length", "depth", "cause", "scout")}
        out["dropped"] = int(dropped.value)
        return out

    def set_tileset(self, tileset=None):
        """Give the handle another tileset (rg_tileset_set; None = the built-in): the next pixel pass draws with it.  Waits for the stream.  The tile height
        decides the shape of `self.pixels`, so an env built with pixels= takes a tileset of the same height only."""
        ts = Tileset.default() if tileset is None else tileset
        if not isinstance(ts, Tileset):
            raise ValueError("tileset must be a Tileset or None, got %r" % (tileset,))
        if getattr(self, "pixels", None) is not None and ts.th != self.tileset.th:
            raise ValueError("set_tileset: `pixels` was built for tiles %d rows high, got %d" % (self.tileset.th, ts.th))
        self._h.check(self._h.L.rg_tileset_set(self._h.h, ts.th, ts.font.ctypes.data, ts.palette.ctypes.data))
        self.tileset = ts

    def _pixel_tensor(self, n, channels, crop):
        th = self.tileset.th
        hc, wc = (self.height, self.width) if crop is None else (2 * crop[0] + 1, 2 * crop[1] + 1)
        with self.torch.cuda.device(self.device):
            return self.torch.empty((n, channels, hc * th, wc * 8), dtype=self.torch.uint8, device=self.device)

    def _pixel_call(self, channels, crop, out, center):
        L, h = self._h.L, self._h.h
        if crop is None:
            self._h.check(L.rg_obs_pixels(h, channels, C.c_void_p(out.data_ptr())))
        else:
            self._h.check(L.rg_obs_pixels_crop(h, channels, crop[0], crop[1], C.c_void_p(out.data_ptr()), None if center is None else C.c_void_p(center.data_ptr())))

    def render_pixels(self, rgb=True, crop=None, tileset=None, out=None):
        """uint8 [N, C, hp, wp] on the device, C = 3 (rgb) or 1 (gray): every env's screen -- or with crop (r or (ry, rx)) its player-centred window -- drawn
        through the env's tileset (rg_obs_pixels / rg_obs_pixels_crop).  tileset (optional): a Tileset that replaces the env's from this call on
        (set_tileset).  out (optional): a contiguous uint8 tensor of that shape on this env's device to write into.  No host trip."""
        if tileset is not None or self.tileset is None:
            self.set_tileset(tileset)
        crop = None if crop is None else self._crop_radii(crop)
        channels = 3 if rgb else 1
        if out is None:
            out = self._pixel_tensor(self.num_envs, channels, crop)
        else:
            hc, wc = (self.height, self.width) if crop is None else (2 * crop[0] + 1, 2 * crop[1] + 1)
            self._dev_arg("render_pixels", "out", out, (self.torch.uint8,), (self.num_envs, channels, hc * self.tileset.th, wc * 8), contiguous=True)
        self._pixel_call(channels, crop, out, None)
        return out

    def frame(self, env_ids, cols=None):
        """One HWC uint8 mosaic [rows * H*th, cols * W*8, 3] on the device of the chosen envs' screens, row-major in the order given, for a video writer
        (`frame(...).cpu().numpy()`).  cols defaults to ceil(sqrt(k)); cells past the last env are black.  Built in torch from render_pixels."""
        torch = self.torch
        ids = torch.as_tensor(np.asarray(env_ids, dtype=np.int64).reshape(-1), device=self.device) if not isinstance(env_ids, torch.Tensor) else env_ids.reshape(-1).to(self.device, torch.int64)
        k = int(ids.numel())
        if k == 0:
            raise ValueError("frame: no envs")
        cols = int(np.ceil(np.sqrt(k))) if cols is None else operator.index(cols)
        if cols < 1:
            raise ValueError("frame: cols must be >= 1, got %r" % (cols,))
        rows = (k + cols - 1) // cols
        img = self.render_pixels(rgb=True)[ids]                      # [k, 3, hp, wp]
        hp, wp = int(img.shape[2]), int(img.shape[3])
        grid = torch.zeros((rows * cols, 3, hp, wp), dtype=torch.uint8, device=self.device)
        grid[:k] = img
        return grid.view(rows, cols, 3, hp, wp).permute(0, 3, 1, 4, 2).reshape(rows * hp, cols * wp, 3).contiguous()

    @staticmethod
    def _crop_radii(crop):
        try:
            ry, rx = (crop, crop) if not isinstance(crop, (tuple, list)) else crop
            ry, rx = operator.index(ry), operator.index(rx)
        except (TypeError, ValueError):
            ry = rx = -1
        if ry < 0 or rx < 0:
            raise ValueError("crop must be None, an int >= 0 or a pair (ry, rx) of ints >= 0, got %r" % (crop,))
        return ry, rx

    def add_crop(self, crop, image_setting: Optional[ImageSetting] = None, obs_dtype=None, symbol_ids: bool = False):
        """Add a crop VIEW: a player-centred window (r or (ry, rx), as the constructor's `crop`) kept beside `self.obs`, for models that read the full map
        and an egocentric crop in the same step.  Returns an object with `.obs` [N, C, 2ry+1, 2rx+1] and `.center` i32 [N, 2]; `self.crops` is the
        tuple of the views added so far.  image_setting defaults to the env's.  obs_dtype (None, torch.float32, torch.float16 or torch.bfloat16) is the
        view's element type; symbol_ids=True (needs DungeonType.SYMBOL, StatusFlag.EMPTY and obs_dtype None, as in the constructor) makes it the uint8
        window of symbol ids [N, 1 + hist, 2ry+1, 2rx+1] -- NLE's `chars_crop`, 121 bytes per env at 11 x 11 (rg_obs_crop_typed).  The view is encoded
        now, and again after `obs` by everything that refreshes `obs`: reset, reset_envs, step_keys / step, load_state and clone_state.  It works on
        every env this class builds -- typed, bound (persistent_obs), cropped, config groups, mixed sizes -- and leaves `obs` as it is without views.
        A learner that wants only the small window: HipVecRogueEnv(cfgs, crop=0) plus add_crop(4, ImageSetting(DungeonType.SYMBOL, ...), symbol_ids=True)."""
        torch = self.torch
        if crop is None:
            raise ValueError("crop must be an int >= 0 or a pair (ry, rx) of ints >= 0, got None")
        ry, rx = self._crop_radii(crop)
        st = self.image_setting if image_setting is None else image_setting
        if not isinstance(st, ImageSetting):
            raise ValueError("image_setting must be an ImageSetting or None, got %r" % (image_setting,))
        call, channels, dtype = self._obs_call(st, obs_dtype, symbol_ids)
        with torch.cuda.device(self.device):
            view = CropView((ry, rx), st, call, torch.empty((self.num_envs, channels, 2 * ry + 1, 2 * rx + 1), dtype=dtype, device=self.device),
                            torch.zeros((self.num_envs, 2), dtype=torch.int32, device=self.device))
        self._encode_view(view)  # (a refused setting -- a config group with more symbols than env 0's under the one-hot kind -- raises here, before the view is kept)
        self._views.append(view)
        return view

    @property
    def crops(self):
        """The crop views added so far (add_crop), in order."""
        return tuple(self._views)

    def _encode_view(self, v):
        st = v.image_setting
        self._h.check(self._h.L.rg_obs_crop_typed(self._h.h, v._call[0], v._call[1], v.crop[0], v.crop[1], st.status.value, int(st.includes_hist),
                                                  C.c_void_p(v.obs.data_ptr()), C.c_void_p(v.center.data_ptr())))

    def _refresh_views(self):
        """After `obs` was refreshed: nothing is pending then, so the crop passes only read the mirrors (and a bound `obs` stays valid)."""
        for v in self._views:
            self._encode_view(v)
        for call in self._refresh:  # pixels, action mask, guide, monsters, objects: those the env was built with
            call()

    def object_table(self, kinds="stairs+gold+door", known=False, secrets=False, cap=8):
        """(table, count) on the device (rg_objects): table int16 [N, cap, 8], the first `cap` (1 .. 32) objects of every env as rows of OBJECT_COLS in
        ascending order of (walk, y, x), empty rows zero; count int32 [N, 4], the cells of each kind (stairs, gold, door, frontier), listed or not.  kinds:
        "stairs", "gold", "door" and -- with known=True only -- "frontier", joined with '+'.  known=True reads the player's own map only; without it the
        answer is PRIVILEGED.  secrets=True walks through hidden and locked cells.  No host trip; the states, mirrors and `obs` are left as they are."""
        torch = self.torch
        kw, mode, cap = inner._object_args(kinds, known, secrets, cap)
        with torch.cuda.device(self.device):
            table = torch.empty((self.num_envs, cap, len(self.OBJECT_COLS)), dtype=torch.int16, device=self.device)
            count = torch.empty((self.num_envs, 4), dtype=torch.int32, device=self.device)
        self._h.check(self._h.L.rg_objects(self._h.h, kw, mode, cap, C.c_void_p(table.data_ptr()), C.c_void_p(count.data_ptr())))
        return table, count

    def monster_table(self, mode="shown", cap=4):
        """(table, threat) on the device (rg_monsters): table int16 [N, cap, 8], the nearest `cap` (1 .. 16) monsters of every env as rows of MONSTER_COLS, nearest
        first, empty rows zero; threat int32 [N, 4], always about the shown monsters: how many stand next to the player, the distance of the nearest (-1 =
        none), the positional attack mask over ACTIONS[1:9], and the number of monsters that qualify in `mode`.  mode "shown": what a redraw would show now.
        mode "all": every living monster of the level, with active, hp and slot filled in -- PRIVILEGED.  No host trip; the states, mirrors and `obs` are left
        as they are."""
        torch = self.torch
        m, cap = inner._monster_args(mode, cap)
        with torch.cuda.device(self.device):
            table = torch.empty((self.num_envs, cap, len(self.MONSTER_COLS)), dtype=torch.int16, device=self.device)
            threat = torch.empty((self.num_envs, 4), dtype=torch.int32, device=self.device)
        self._h.check(self._h.L.rg_monsters(self._h.h, m, cap, C.c_void_p(table.data_ptr()), C.c_void_p(threat.data_ptr())))
        return table, threat

    def route(self, goal="stairs", fallback=None, secrets=False, known=False, cells=None):
        """(keys, dist, tier) on the device (rg_route): path() with two switches and a fallback goal, without a field.  secrets=True plans THROUGH hidden and
        locked cells and answers 's' when the next cell of the route is one.  known=True plans on the player's own map only (the cells that are drawn or
        in view): nothing is privileged then.  goal / fallback: "stairs", "gold", "stairs+gold", or "frontier" with known=True (the known cells beside an
        unknown one); goal None with `cells` = the caller's cells alone.  An env that `goal` does not reach is answered from `fallback`; tier uint8 [N]
        says which answered: 0, 1, or 255 = neither (dist -1, key 's').  cells as path()'s; they join `goal`.  No host trip; the states, mirrors and
        `obs` are left as they are."""
        torch = self.torch
        goals, fb, mode = inner._route_args(goal, fallback, secrets, known, cells is not None)
        if cells is not None:
            cells = self._dev_arg("route", "cells", cells, (torch.int32,), (self.num_envs, 2))
        with torch.cuda.device(self.device):
            keys = torch.empty((self.num_envs,), dtype=torch.uint8, device=self.device)
            dist = torch.empty((self.num_envs,), dtype=torch.int32, device=self.device)
            tier = torch.empty((self.num_envs,), dtype=torch.uint8, device=self.device)
        self._h.check(self._h.L.rg_route(self._h.h, goals, fb, mode, None if cells is None else C.c_void_p(cells.data_ptr()), C.c_void_p(dist.data_ptr()),
                                         C.c_void_p(keys.data_ptr()), C.c_void_p(tier.data_ptr())))
        return keys, dist, tier

    def path(self, goal="stairs", cells=None, field=False):
        """(keys, dist, field) on the device (rg_path): keys uint8 [N], the teacher key of every env towards its nearest goal cell, for step_keys; dist int32 [N],
        the number of moves to it, -1 = unreachable; field uint16 [N, H, W], the number of moves from every cell (0xFFFF = unreachable), or None unless
        field=True (not for batches that mix sizes or configs).  goal: "stairs", "gold", "stairs+gold", or None with `cells`.  cells (optional): an int32
        tensor [N, 2] on this env's device, one cell (y, x) per env that is a goal too; a cell outside the grid adds nothing.  The answers are PRIVILEGED:
        they see stairs, gold and passages the player has not discovered.  No host trip; the states, mirrors and `obs` are left as they are."""
        torch = self.torch
        goals = inner._path_goals(goal, cells is not None)
        if cells is not None:
            cells = self._dev_arg("path", "cells", cells, (torch.int32,), (self.num_envs, 2))
        with torch.cuda.device(self.device):
            keys = torch.empty((self.num_envs,), dtype=torch.uint8, device=self.device)
            dist = torch.empty((self.num_envs,), dtype=torch.int32, device=self.device)
            fld = torch.empty((self.num_envs, self.height, self.width), dtype=torch.uint16, device=self.device) if field else None
        self._h.check(self._h.L.rg_path(self._h.h, goals, None if cells is None else C.c_void_p(cells.data_ptr()), None if fld is None else C.c_void_p(fld.data_ptr()),
                                        C.c_void_p(dist.data_ptr()), C.c_void_p(keys.data_ptr())))
        return keys, dist, fld

    def _mask_call(self, keys, mask, sample, seed, draw):
        kb, nk = inner._mask_keys(keys)
        self._h.check(self._h.L.rg_action_mask(self._h.h, kb, nk, None if mask is None else C.c_void_p(mask.data_ptr()),
                                               None if sample is None else C.c_void_p(sample.data_ptr()), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFFFFFFFFFF))

    def legal_mask(self, keys=None, out=None):
        """bool [N, n_keys] on the device: entry [i, k] says whether keys[k] would do anything for env i now (rg_action_mask).  keys: bytes / str of keys of
        KeyMap::ai, run keys included, checked by the library; None = ACTIONS in index order.  out (optional): a contiguous uint8 / bool tensor
        [N, n_keys] on this env's device to write into.  No host trip; the states, mirrors and `obs` are left as they are."""
        torch = self.torch
        nk = inner._mask_keys(keys)[1]
        if out is None:
            with torch.cuda.device(self.device):
                out = torch.empty((self.num_envs, nk), dtype=torch.uint8, device=self.device)
        else:
            self._dev_arg("legal_mask", "out", out, (torch.uint8, torch.bool), (self.num_envs, nk), contiguous=True)
        self._mask_call(keys, out, None, 0, 0)
        return out if out.dtype == torch.bool else out.view(torch.bool)

    def sample_keys(self, seed=0, draw=None, keys=None):
        """uint8 [N] on the device: for each env one key byte of `keys` (None = ACTIONS) drawn uniformly among the keys that would do anything for it now --
        what step_keys takes -- from the launch that computes the mask.  The draw is a stateless function of (seed, env index, draw) (rg_sample_index):
        draw=None uses a counter kept by this env that advances by one per call; the same (seed, draw) on the same states gives the same keys.  With
        action_mask=True and keys=None the call also rewrites `self.action_mask`, which it equals anyway."""
        torch = self.torch
        if draw is None:
            draw, self._draw = self._draw, self._draw + 1
        with torch.cuda.device(self.device):
            out = torch.empty((self.num_envs,), dtype=torch.uint8, device=self.device)
        self._mask_call(keys, self._mask_u8 if keys is None else None, out, seed, draw)
        return out

    def act(self, logits, greedy=False, temperature=1.0, epsilon=0.0, teacher=None, beta=0.0, given=None, seed=0, draw=None, keys=None):
        """One masked categorical action per env from policy logits, in one launch (rg_act) -> ActResult(keys, actions, logp, entropy, source) of device
        tensors [N]: `keys` uint8 is what step_keys takes, `actions` int32 the index into `keys=` (None = ACTIONS), `logp` float32 the natural log of
        pi(action), `entropy` float32 of pi in nats, `source` uint8 0 policy / 1 uniform / 2 teacher / 3 none (inner.ACT_SOURCES).
        logits: [N, n_keys] float32, float16 or bfloat16 on this env's device.  pi is the softmax of logits / temperature over the keys that are LEGAL now
        (`action_mask`'s rule); an illegal key has probability 0 whatever its logit.  greedy=True takes the legal argmax (ties: the lowest index).
        epsilon: the probability of a uniform draw among the legal keys; teacher (uint8 [N] key bytes, e.g. `self.guide_keys`) with beta: the probability of
        playing the teacher's key where it is listed and legal -- DAgger's mixing; epsilon + beta <= 1.  given (int32 [N] action indices): no draw, the
        log-probability of those actions (-inf for an illegal one), `keys` their key bytes.
        `logp` is ALWAYS under the pure masked softmax, also when epsilon or the teacher chose: it is the BEHAVIOUR log-probability for the rollout buffer
        and carries no autograd -- the learner's update recomputes log pi from its own logits and the stored `action_mask` with `rogue_gym.masked_logp`
        (or `self.evaluate`), which answers these very bits for unchanged logits and has a backward pass.
        The draw is a stateless function of (seed, env index, draw); draw=None uses the counter sample_keys uses, which advances by one per call.  With
        action_mask=True and keys=None the call also rewrites `self.action_mask`.  No host trip; states, mirrors and `obs` are left as they are."""
        torch = self.torch
        kb, nk = inner._mask_keys(keys)
        logits = self._dev_arg("act", "logits", logits, (torch.float32, torch.float16, torch.bfloat16), (self.num_envs, nk)).detach()
        if teacher is not None:
            teacher = self._dev_arg("act", "teacher", teacher, (torch.uint8,), (self.num_envs,))
        if given is not None:
            given = self._dev_arg("act", "given", given, (torch.int32,), (self.num_envs,))
        if draw is None:
            draw, self._draw = self._draw, self._draw + 1
        opts = inner._act_opts(greedy, temperature, epsilon, beta, given is not None, seed, draw)
        with torch.cuda.device(self.device):
            out = inner.ActResult(torch.empty((self.num_envs,), dtype=torch.uint8, device=self.device), torch.empty((self.num_envs,), dtype=torch.int32, device=self.device),
                                  torch.empty((self.num_envs,), dtype=torch.float32, device=self.device), torch.empty((self.num_envs,), dtype=torch.float32, device=self.device),
                                  torch.empty((self.num_envs,), dtype=torch.uint8, device=self.device))
        mask = self._mask_u8 if keys is None else None
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        self._h.check(self._h.L.rg_act(self._h.h, kb, nk, ptr(logits), inner.ACT_DTYPES[str(logits.dtype).replace("torch.", "")], C.byref(opts), ptr(teacher), ptr(given),
                                       ptr(out.keys), ptr(out.actions), ptr(out.logp), ptr(out.entropy), ptr(out.source), ptr(mask)))
        return out

    def evaluate(self, logits, actions, mask=None, temperature=1.0):
        """rogue_gym.masked_logp(logits, actions, mask, temperature) -> (logp, entropy) with autograd, `mask` defaulting to `self.action_mask` as it stands now
        (the envs must not have stepped since the actions were chosen; a rollout buffer passes the masks it stored)."""
        from ..learn import masked_logp
        if mask is None:
            if self.action_mask is None:
                raise ValueError("evaluate: no mask given and the env was made without action_mask=True")
            mask = self.action_mask
        return masked_logp(logits, actions, mask, temperature)

    def step_logits(self, logits, **opts):
        """act(logits, **opts) followed by step_keys of the keys it chose -> (obs, reward, done, act_result)."""
        res = self.act(logits, **opts)
        obs, reward, done = self.step_keys(res.keys)
        return obs, reward, done, res

    @property
    def screen(self):
        """u8 [num_envs, H, W] glyph mirror (PlayerState.map of every env).  Reading it flushes the pending render (a batch with several
        config groups assembles the groups' screens first); the tensor itself is the same device buffer every time."""
        return self._screen_view()

    def _screen_view(self):
        p = C.c_void_p()
        self._h.check(self._h.L.rg_screen(self._h.h, C.byref(p)))
        if self._screen is None:
            self._screen = self._dev_view(p.value, (self.num_envs, self.height, self.width), "|u1")
        return self._screen

    def _encode(self):
        """Re-encode `obs`, then the crop views."""
        obs = self._encode_obs()
        self._refresh_views()
        return obs

    def _encode_obs(self):
        L, h = self._h.L, self._h.h
        if self.crop is not None:
            self._h.check(L.rg_obs_crop(h, int(self._sym), self.crop[0], self.crop[1], self.image_setting.status.value, int(self.image_setting.includes_hist),
                                        C.c_void_p(self.obs.data_ptr()), C.c_void_p(self.crop_center.data_ptr())))
            return self.obs
        if self._typed is not None:
            self._h.check(L.rg_obs_typed(h, self._typed[0], self._typed[1], self.image_setting.status.value, int(self.image_setting.includes_hist),
                                         C.c_void_p(self.obs.data_ptr())))
            return self.obs
        fn = L.rg_obs_symbol if self._sym else L.rg_obs_gray
        self._h.check(fn(h, self.image_setting.status.value, int(self.image_setting.includes_hist), C.c_void_p(self.obs.data_ptr())))
        return self.obs

    def reset(self):
        self._h.check(self._h.L.rg_reset(self._h.h))
        if self._episodes:  # the running episodes end here, cause 3
            self._h.check(self._h.L.rg_episode_cut(self._h.h, None, 0, 0, None, 1))
        obs = self._encode()
        self._novelty_cut()
        return obs

    def reset_envs(self, env_ids=None, mask=None, seeds=None):
        """Rebuild the chosen envs as reset() rebuilds every env (rg_reset_envs / rg_reset_mask) and return the observation batch, re-encoded; every
        other env keeps its state.  Exactly one of env_ids (a list, a numpy array or a device tensor of env indices, without duplicates) and mask (a
        bool / uint8 device tensor [num_envs], True = rebuild; it never reaches the host) is given.  seeds (optional, with host env_ids only): one
        int of up to 128 bits per id, given to those envs first (rg_seed_envs) -- they restart on it now and at every later reset."""
        ptr, k, on_dev, mask, _keep = self._ids_or_mask("reset_envs", env_ids, mask, one=True)
        L, h = self._h.L, self._h.h
        if mask is not None:
            if seeds is not None:
                raise ValueError("reset_envs: seeds go with host env_ids, not with a mask")
            self._h.check(L.rg_reset_mask(h, C.c_void_p(mask.data_ptr())))  # (a bool tensor is one byte per element, 0 / 1)
            if self._episodes:
                self._h.check(L.rg_episode_cut(h, None, 0, 0, C.c_void_p(mask.data_ptr()), 1))
            obs = self._encode()
            self._novelty_cut(mask=mask)
            return obs
        if seeds is not None:
            if on_dev:
                raise ValueError("reset_envs: seeds go with host env_ids, not with a device tensor")
            seeds = [int(s) for s in seeds]
            if len(seeds) != k or any(s < 0 or s >> 128 for s in seeds):
                raise ValueError("reset_envs: seeds must be %d ints in [0, 2**128), one per env id" % k)
            lo = (C.c_uint64 * k)(*[s & 0xFFFFFFFFFFFFFFFF for s in seeds])
            hi = (C.c_uint64 * k)(*[s >> 64 for s in seeds])
            self._h.check(L.rg_seed_envs(h, ptr, lo, hi, k))
        if k == 0:  # (an empty device tensor has no address, and a NULL list means every env)
            _keep = np.zeros(1, np.int32)
            ptr, on_dev = C.c_void_p(_keep.ctypes.data), 0
        self._h.check(L.rg_reset_envs(h, ptr, k, on_dev))
        if self._episodes and k:
            self._h.check(L.rg_episode_cut(h, ptr, k, on_dev, None, 1))
        obs = self._encode()
        if k:
            self._novelty_cut(ptr, k, on_dev)
        return obs

    def seed(self, seeds):
        seeds = [int(s) for s in seeds]
        n = len(seeds)
        lo = (C.c_uint64 * n)(*[s & 0xFFFFFFFFFFFFFFFF for s in seeds])
        hi = (C.c_uint64 * n)(*[(s >> 64) & 0xFFFFFFFFFFFFFFFF for s in seeds])
        self._h.check(self._h.L.rg_seed(self._h.h, lo, hi, n))

    def step_keys(self, keys):
        """keys: uint8 CUDA tensor [num_envs] of key bytes (KeyMap::ai), contiguous, on this env's device."""
        out = self._step_keys(keys)
        self._refresh_views()
        return out

    def _step_keys(self, keys):
        """The step and the refresh of `obs`, without the crop views."""
        if keys.dtype != self.torch.uint8 or keys.device != self.device or not keys.is_contiguous() or keys.numel() != self.num_envs:
            raise ValueError("step_keys needs a contiguous uint8 tensor of %d keys on %s, got %s %s on %s"
                             % (self.num_envs, self.device, tuple(keys.shape), keys.dtype, keys.device))
        if self._typed is not None:  # the step and the typed observation as one call (rg_step_obs_typed)
            self._h.check(self._h.L.rg_step_obs_typed(self._h.h, C.c_void_p(keys.data_ptr()), 1, self._typed[0], self._typed[1], self.image_setting.status.value,
                                                       int(self.image_setting.includes_hist), C.c_void_p(self.obs.data_ptr())))
            obs = self.obs
        elif self._sym or self.crop is not None:
            self._h.check(self._h.L.rg_step(self._h.h, C.c_void_p(keys.data_ptr()), 1))
            obs = self._encode_obs()
        else:  # the step and the gray observation as one call: fused into one kernel where the config allows it (rg_step_obs_gray)
            self._h.check(self._h.L.rg_step_obs_gray(self._h.h, C.c_void_p(keys.data_ptr()), 1, self.image_setting.status.value, int(self.image_setting.includes_hist),
                                                      C.c_void_p(self.obs.data_ptr())))
            obs = self.obs
        for call in self._after_step:  # the episode, novelty and archive updates: those the env was built with
            call()
        return obs, self.reward, self.done

    def step(self, actions):
        """actions: integer CUDA tensor [num_envs] of indices into ACTIONS."""
        return self.step_keys(self._action_keys[actions.long()])

    def check_errors(self):
        """Synchronise and raise like the reference's PyRuntimeError if any env saw an invalid key."""
        self._h.check(self._h.L.rg_sync(self._h.h))

    def packed_records(self, with_hist: bool = False):
        """u8 [num_envs, record]: the compact observation record of every env of this rank (rg_pack_compact)."""
        L, h = self._h.L, self._h.h
        rec = L.rg_compact_record_bytes(h, int(with_hist))
        buf = self._scratch_tensor(("packed", bool(with_hist)), (self.num_envs, rec))
        self._h.check(L.rg_pack_compact(h, int(with_hist), C.c_void_p(buf.data_ptr())))
        return buf

    def _scratch_tensor(self, key, shape):
        """The uint8 device tensor kept under `key` from one call to the next (made by the first)."""
        buf = self._scratch.get(key)
        if buf is None:
            buf = self._scratch[key] = self.torch.empty(shape, dtype=self.torch.uint8, device=self.device)
        return buf

    def expand_records(self, packed, image_setting: Optional[ImageSetting] = None, packed_has_hist: bool = False, out=None):
        """f32 [N, C, H, W] from N compact records (of any rank) under `image_setting`: the HIP encode kernels on the consumer GPU."""
        st = self.image_setting if image_setting is None else image_setting
        sym = st.dungeon == DungeonType.SYMBOL
        L, h = self._h.L, self._h.h
        n = int(packed.shape[0])
        c = L.rg_obs_channels(h, int(sym), st.status.value, int(st.includes_hist))
        if out is None:
            out = self.torch.empty((n, c, self.height, self.width), dtype=self.torch.float32, device=self.device)
        if packed.dtype != self.torch.uint8 or not packed.is_contiguous() or packed.device != self.device:
            raise ValueError("expand_records needs a contiguous uint8 tensor on %s" % (self.device,))
        self._h.check(L.rg_expand_compact(h, C.c_void_p(packed.data_ptr()), n, int(packed_has_hist), int(sym), st.status.value, int(st.includes_hist),
                                          C.c_void_p(out.data_ptr())))
        return out

    def init_comm(self, rank: Optional[int] = None, world: Optional[int] = None, unique_id: Optional[bytes] = None):
        """Give the handle its own RCCL communicator (rg_comm_init), so that the one collective of the sharded path runs behind the C-ABI
        (rg_allgather_compact: pack into this rank's slice, ncclAllGather in place on the handle's stream) -- the path a non-Python host
        binds.  Without arguments the rank / world come from torch.distributed and rank 0's ncclUniqueId is broadcast through it; a host
        without torch passes all three (the id from `HipVecRogueEnv.comm_unique_id()` on one rank)."""
        import torch.distributed as dist

        if rank is None or world is None:
            rank, world = dist.get_rank(), dist.get_world_size()
        if unique_id is None:
            box = [self.comm_unique_id() if rank == 0 else None]
            if world > 1:
                dist.broadcast_object_list(box, src=0)
            unique_id = box[0]
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._h.check(self._h.L.rg_comm_init(self._h.h, buf, int(rank), int(world)))
        self._comm = (int(rank), int(world))

    def comm_count(self):
        """(ranks, this rank) as the RCCL communicator itself reports them (rg_comm_count = ncclCommCount / ncclCommUserRank)."""
        c, r = C.c_int(), C.c_int()
        self._h.check(self._h.L.rg_comm_count(self._h.h, C.byref(c), C.byref(r)))
        return c.value, r.value

    @staticmethod
    def comm_unique_id() -> bytes:
        L = inner.load_library()
        buf = (C.c_uint8 * 128)()
        if L.rg_comm_unique_id(buf):
            raise RuntimeError("Error in rogue-gym: " + L.rg_last_error(None).decode())
        return bytes(buf)

    def all_gather_records(self, with_hist: bool = False):
        """u8 [world * num_envs, record] on every rank through the handle's own communicator (init_comm): rg_allgather_compact."""
        rank, world = self._comm
        L, h = self._h.L, self._h.h
        rec = L.rg_compact_record_bytes(h, int(with_hist))
        buf = self._scratch_tensor(("gathered", bool(with_hist)), (world * self.num_envs, rec))
        self._h.check(L.rg_allgather_compact(h, int(with_hist), C.c_void_p(buf.data_ptr())))
        return buf

    def all_gather_obs(self, compact: bool = True):
        """Whole-job observation batch f32 [world * num_envs, C, H, W] on every rank, env order = rank order -- the same type whatever the
        world size (world 1: this rank's own `obs`).  compact=True (default): ONE RCCL all-gather over xGMI of the packed records
        (560 B per mini env instead of 2 KB .. 330 KB of f32), expanded on the consumer GPU by the HIP encode kernels -- through the
        handle's own communicator when init_comm() was called (the C-ABI path), else through torch.distributed;
        compact=False gathers the f32 observation itself (xGMI-bound for the one-hot image)."""
        import torch.distributed as dist

        torch = self.torch
        if compact and getattr(self, "_comm", None) is not None:
            with_hist = bool(self.image_setting.includes_hist)
            return self.expand_records(self.all_gather_records(with_hist), packed_has_hist=with_hist)
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return self.obs
        group = getattr(self, "process_group", None)  # None = the default group; a host whose default group is a CPU one sets its RCCL group here
        ws = dist.get_world_size(group)
        if not compact:
            out = torch.empty((ws * self.num_envs,) + tuple(self.obs.shape[1:]), dtype=self.obs.dtype, device=self.device)
            dist.all_gather_into_tensor(out, self.obs, group=group)
            return out
        from .sharding import all_gather_packed

        with_hist = bool(self.image_setting.includes_hist)
        gathered = all_gather_packed(self.packed_records(with_hist), group=group)
        return self.expand_records(gathered, packed_has_hist=with_hist)

    def all_gather_step(self):
        """(obs, reward, done, flags) of the WHOLE job on every rank from the ONE collective of the step: obs f32 [world * num_envs, C, H, W],
        reward f32 [N], done bool [N], flags i32 [N] (public RG_FLAG_* bits), env order = rank order.  ThreadConductor::step returns state and
        terminal flag of every env in one reply (python/src/thread_impls.rs:61-81) and parallel.py:59-64 derives reward and done from it; here the
        compact record carries them next to the screen, so a learner that wants the all-gathered batch needs no second collective."""
        import torch.distributed as dist
        from .sharding import all_gather_packed, unpack_step

        with_hist = bool(self.image_setting.includes_hist)
        if getattr(self, "_comm", None) is not None:
            packed = self.all_gather_records(with_hist)
        else:
            packed = self.packed_records(with_hist)
            if dist.is_available() and dist.is_initialized() and dist.get_world_size(getattr(self, "process_group", None)) > 1:
                packed = all_gather_packed(packed, group=getattr(self, "process_group", None))
        reward, done, flags = unpack_step(packed, self.height, self.width, with_hist)
        return self.expand_records(packed, packed_has_hist=with_hist), reward, done, flags

    def all_gather_compact(self, with_hist: bool = False):
        """The gathered records themselves, as views: (screen u8 [N,H,W], status i32 [N,10], hist u8 [N,H,W] or None)."""
        import torch.distributed as dist
        from .sharding import all_gather_packed, unpack_records

        packed = self.packed_records(with_hist)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            packed = all_gather_packed(packed, group=getattr(self, "process_group", None))
        return unpack_records(packed, self.height, self.width, with_hist)

    def status_vec(self, flag=None):
        """i32 [num_envs, popcount(flag)] device tensor: PlayerState::status_vec of every env (flags.rs:67-87)."""
        flag = self.image_setting.status.value if flag is None else int(getattr(flag, "value", flag))
        cols = [c for b, c in enumerate((0, 2, 3, 4, 5, 6, 7, 8, 9)) if flag & (1 << b)]
        return self.status[:, cols]

    def counters(self, reset: bool = False):
        """Workload counters since the last reset of the counters (rg_counters)."""
        out = (C.c_uint64 * 9)()
        self._h.check(self._h.L.rg_counters_ex(self._h.h, out, 9, int(reset)))
        names = ("resets", "descents", "dist_maps", "inline_generations", "spares_taken", "redraws", "keys", "partial_maps_continued", "next_level_structures_used")
        return dict(zip(names, (int(v) for v in out)))

    # ---- batched save / restore of game states (rg_state_save / rg_state_load; record layout: include/rogue_gym_hip.h) ----
    @property
    def state_bytes(self) -> int:
        """R: bytes of one state record of this env batch (geometry, room grid and key-log capacity decide it)."""
        return self._h.state_bytes()

    def _state_ids(self, env_ids, unique):
        """(pointer, count, on_device, keep-alive) of env_ids: None = every env in order; a list / numpy array (range-checked by the library) or a
        device tensor (checked here)."""
        torch = self.torch
        if env_ids is None:
            return None, self.num_envs, 0, None
        if isinstance(env_ids, torch.Tensor) and env_ids.device.type == "cuda":
            t = env_ids.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= self.num_envs):
                raise ValueError("env ids out of range [0, %d)" % self.num_envs)
            if unique and torch.unique(t).numel() != t.numel():
                raise ValueError("load_state: duplicate env ids")
            return C.c_void_p(t.data_ptr()), int(t.numel()), 1, t
        if isinstance(env_ids, torch.Tensor):
            env_ids = env_ids.numpy()
        a = np.ascontiguousarray(np.asarray(env_ids, dtype=np.int64).reshape(-1))
        if unique and np.unique(a).size != a.size:
            raise ValueError("load_state: duplicate env ids")
        a = a.astype(np.int32)
        return C.c_void_p(a.ctypes.data), int(a.size), 0, a

    def _ids_or_mask(self, call, env_ids, mask, one):
        """(pointer, count, on_device, mask, keep-alive) of the envs that `call` names by env_ids (_state_ids' forms, duplicates among device ids refused here) or
        by mask (a bool / uint8 device tensor [num_envs]: pointer None, count 0).  one: exactly one of the two must be given; else both None = every env."""
        if (env_ids is not None and mask is not None) or (one and env_ids is None and mask is None):
            raise ValueError("%s takes %s env_ids and mask" % (call, "exactly one of" if one else "at most one of"))
        if mask is not None:
            return None, 0, 0, self._dev_arg(call, "mask", mask, (self.torch.bool, self.torch.uint8), (self.num_envs,)), None
        ptr, k, on_dev, keep = self._state_ids(env_ids, unique=False)
        if on_dev and self.torch.unique(keep).numel() != k:
            raise ValueError("%s: duplicate env_ids" % call)
        return ptr, k, on_dev, None, keep

    def save_state(self, env_ids=None):
        """u8 [k, state_bytes] on this env's device: the state records of env_ids (default: every env, in order), asynchronously on the stream.
        A record holds the env's whole running game -- grids, mirrors, dist cache, monsters, RNG streams, the episode's key log -- and not what
        decides its future episodes (seed, spares): those belong to whichever slot it is loaded into."""
        ptr, k, on_dev, _keep = self._state_ids(env_ids, unique=False)
        out = self.torch.empty((k, self.state_bytes), dtype=self.torch.uint8, device=self.device)
        if k:
            self._h.check(self._h.L.rg_state_save(self._h.h, ptr, k, on_dev, C.c_void_p(out.data_ptr())))
        return out

    def load_state(self, records, env_ids=None):
        """Restore envs env_ids (default: every env, in order) from state records u8 [k, R] (save_state of this or another batch of the same config,
        seed aside, or RogueEnv.save_state).  A restored env plays out the saved episode; when that ends it resets from its OWN seed.  A record that
        does not fit leaves its env unchanged and makes check_errors() raise.  Returns the observation batch, re-encoded.  The episode accounting
        (episodes=True) is left alone -- the lanes go on counting as if nothing had happened; cut_episodes() rebases them on the loaded games."""
        torch = self.torch
        if not isinstance(records, torch.Tensor) or records.dtype != torch.uint8 or records.dim() != 2 or records.device != self.device:
            raise ValueError("load_state needs a uint8 tensor [k, record bytes] on %s" % (self.device,))
        records = records.contiguous()
        ptr, k, on_dev, _keep = self._state_ids(env_ids, unique=True)
        if k != records.shape[0]:
            raise ValueError("load_state: %d records for %d envs" % (records.shape[0], k))
        if k:
            self._h.check(self._h.L.rg_state_load(self._h.h, C.c_void_p(records.data_ptr()), int(records.shape[1]), ptr, k, on_dev))
        obs = self._encode()
        if k:  # (the visit tables are not part of a record: the loaded envs start a new episode of counts)
            self._novelty_cut(ptr, k, on_dev)
        return obs

    def clone_state(self, src_ids, dst_ids):
        """Copy the states of src_ids into dst_ids (through a scratch record batch, so overlapping id sets are well defined): e.g. one
        interesting env branched into many lanes, clone_state([17] * 4096, range(4096)).  As load_state, it leaves the episode accounting alone
        (cut_episodes())."""
        return self.load_state(self.save_state(src_ids), dst_ids)

    def enable_history(self, cap_per_env: int):
        self._h.check(self._h.L.rg_history_enable(self._h.h, int(cap_per_env)))

    def dump_history(self, env: int, previous: bool = False) -> str:
        """GameState::dump_history (python/src/lib.rs:245-250) of env `env`: the InputCode JSON of its running (or previous) episode."""
        return self._h.dump_history(int(env), previous)

    def history_keys(self, env: int, previous: bool = False) -> bytes:
        return self._h.history_keys(int(env), previous)

    def close(self):
        self._h.close()


class HipVecStairReward(HipVecRogueEnv):
    """StairRewardParallel (python/rogue_gym/envs/wrappers.py:45-64) on device tensors.  The rule -- `stair_reward` whenever an env reports a deeper
    level than one step earlier, the comparison level following the auto-reset back to 1 -- runs inside the step kernel (rg_set_stair_reward): `reward`
    is the same device tensor as without the wrapper, no extra launch, and the all-gathered records carry the bonus too."""

    def __init__(self, *args, stair_reward: float = 50.0, **kwargs):
        super().__init__(*args, **kwargs)
        self.stair_reward = float(stair_reward)
        self._h.check(self._h.L.rg_set_stair_reward(self._h.h, self.stair_reward))


class HipVecFirstFloor(HipVecStairReward):
    """FirstFloorEnv (python/rogue_gym/envs/wrappers.py:35-43) on device tensors, with the auto-reset convention of ThreadConductor::step: an env that reports
    dungeon level 2 after a step has finished its episode -- it is rebuilt at once (rg_reset_mask; the mask is computed on the device, nothing synchronises)
    and the step returns its post-reset observation with `done` true and the step's reward, stair bonus included.  The bonus rule lives in the step kernel and
    pays only in a step that descends, so a rebuilt env (level 1 again) is not paid twice.  `reward` and `done` are new tensors here: the handle's own are
    rewritten by the rebuild (reward 0, done 0)."""

    def step_keys(self, keys):
        _, reward, done = self._step_keys(keys)  # (the crop views are encoded once, after the rebuild)
        reached = (self.status[:, 0] >= 2) & ~done
        reward = reward.clone()
        done = done | reached
        obs = self.reset_envs(mask=reached)
        return obs, reward, done
