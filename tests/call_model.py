"""The model of the interleaved call programs (tests/call_programs.py): what every C-ABI call of a program must produce, from the CPU oracle alone.

The model is a dict env -> (Lane, lineage); a Lane is an OracleEnv and the bookkeeping of forced descents (class Lane).  A lineage is the seed the running episode was built from and the keys it has received since, a forced
descent recorded as the marker DESCEND; a terminal step empties it and puts the env's own current seed in it.  A state record is a copy of a lineage (and
of the one bit a replay does not bring back: the is_terminal that an auto-reset forces on the new game it reports, thread_impls.rs:69-79):
rg_state_load is modelled by replaying it into a fresh OracleEnv and giving that clone the destination's seed (include/rogue_gym_hip.h: a record carries
the running episode, what decides the env's future episodes belongs to the destination).  tests/test_call_programs_host.py proves the replay.

CallModel.apply(op) plays one program entry and returns that call's own outputs as a dict name -> numpy array, the names being those the GPU harness
(tests/test_gpu_call_programs.py) fills from the library.  Expected values come from the helpers the suite trusts already: encode_image (the oracle's
encoders), typed_util, parity_util.crop_window and pixel_util.

What the model leaves out, and why:
  * `done` of an env that rg_step_prefix gave no key: the header defines reward 0 and an unchanged state for it, not its done byte.
  * the reward / done mirrors after anything but a step (a load brings the record's, a reset zeroes them): no call of a program reads them there.
  * the one-hot image of an env whose screen shows a glyph PlayerState::symbol_image refuses ('Z' with 26 monster kinds): the oracle raises, the library
    reports it at the next rg_sync -- apply() marks the env in `skip`, and the program puts that rg_sync right behind the call.

`wrong` selects one of six deliberate misreadings of the header (WRONG); the CPU proof shows that each changes an output the GPU test compares."""
import numpy as np

import pixel_util
import shadow_turn as shadow
import typed_util as tu
from oracle.pyoracle import OracleEnv, encode_image, lib as oracle_lib  # noqa: F401
from parity_util import crop_window

DESCEND = "D"
S_STAIR = 4  # rg_state.h: the surface code of the stairs (bits 0-2 of a cell word; orc_grid's surface plane)
WRONG = ("load_seed",          # a loaded env later resets from the record's seed
         "seed_ignored",       # rg_seed_envs is ignored by the next auto-reset (a stale spare is taken)
         "reset_keeps_steps",  # a partial reset keeps the step counter
         "load_keeps_steps",   # a load keeps the destination's step counter
         "prefix_dot",         # a prefix step plays '.' for the envs without a key
         "load_keeps_status")  # a load keeps the destination's status mirror

_TILESET = []


def tileset():
    """The built-in tileset of the pixel passes (rg_tileset_default: stateless, needs no device)."""
    if not _TILESET:
        from rogue_gym_python import _rogue_gym as inner

        _TILESET.append(pixel_util.default_tileset(inner.load_library()))
    return _TILESET[0]


def popcount(x):
    return bin(x & 0x1FF).count("1")


def same_state(a, b, terminal=True):
    """None if two lanes (or OracleEnvs) are in the same state -- mirrors, flags, grid, monsters, scalars, RNG words -- else the name of the first part that differs.
    terminal=False leaves is_terminal out: the state an auto-reset reports is a new game's with is_terminal forced (thread_impls.rs:69-79), and the model
    keeps that bit beside the lineage (CallModel.shown_terminal)."""
    for name, f in (("screen", lambda o: o.screen()), ("hist", lambda o: o.hist()), ("status", lambda o: o.status_arr()), ("rng", lambda o: o.rng()[0])):
        if not np.array_equal(f(a), f(b)):
            return name
    for name, f in (("flags", lambda o: dict(o.flags(), is_terminal=terminal and o.flags()["is_terminal"])), ("scalars", lambda o: o.scalars()), ("monsters", lambda o: o.monsters()), ("rng counters", lambda o: o.rng()[1])):
        if f(a) != f(b):
            return name
    for k, (x, y) in enumerate(zip(a.grid(), b.grid())):
        if not np.array_equal(x, y):
            return "grid plane %d" % k
    return None


class Lane:
    """One env of the model: an OracleEnv, and what rg_debug_descend does to the mirrors.  The oracle's hook (orc_debug_descend) is actions::new_level alone and
    leaves its PlayerState mirror to the next reactions; the library's (include/rogue_gym_hip.h, k_debug_descend) also rewrites the status, clears the message
    bits and marks the screen and the history of the NEW level for redrawing at the next read.  So behind a forced descent the lane shows the second
    restatement's drawing of the oracle's state (tests/shadow_turn.py Shadow.draw_screen / history_map / status, pinned to the oracle by
    tests/test_oracle_shadow.py), and follows the mirror's own rules from there until the oracle's mirror has caught up:
      * the status stays the drawn one until a key updates the oracle's status (both are then the same fresh words);
      * a Redraw -- seen as a change of the oracle's screen or history -- shows the oracle's screen and the visited map of the level the status mirror names:
        the current one, or on a real descent the floor just left (PlayerState::draw_map with the status of before the key, python/src/lib.rs:59-68);
      * after the status has caught up, the next Redraw is the oracle's own in every byte, and the lane is an OracleEnv again.
    Everything else is the oracle's."""

    def __init__(self, cfg, max_steps, seed):
        self.o = OracleEnv(cfg, max_steps=max_steps, seed=int(seed))
        self.cfg, self.forced = cfg, None

    def __getattr__(self, name):   # (scalars, grid, monsters, rooms, rng, set_seed, h, w, symbols ...: the oracle's)
        return getattr(self.o, name)

    def visited(self):
        return ((self.o.grid()[1] & shadow.VISITED) != 0).astype(np.uint8)

    def reset(self):
        self.o.reset()
        self.forced = None

    def debug_descend(self):
        o, d = self.o, self.cfg.get("dungeon", {})
        o.debug_descend()
        sh = shadow.Shadow(o.w, o.h, self.cfg.get("player", {}).get("hunger_time", 1300), d.get("passage_unlock_rate_inv", 3), d.get("door_unlock_rate_inv", 5))
        sh.new_game(o)
        self.forced = dict(screen=sh.draw_screen().reshape(o.h, o.w), hist=sh.history_map().reshape(o.h, o.w), status=np.array(sh.status(), np.int64).astype(np.uint32),
                           message=0, caught=False)

    def step_autoreset(self, key):
        o, f = self.o, self.forced
        if f is None:
            return o.step_autoreset(key)
        before = (o.screen(), o.hist(), o.status_arr(), o.scalars()["level"], self.visited())
        o.step_autoreset(key)
        if o.flags()["is_terminal"]:
            self.forced = None
            return
        f["message"] = None
        redraw = not (np.array_equal(before[0], o.screen()) and np.array_equal(before[1], o.hist()))
        if redraw and f["caught"]:
            self.forced = None
            return
        if redraw:
            f["screen"], f["hist"] = None, before[4] if o.scalars()["level"] > before[3] else self.visited()
        if not np.array_equal(before[2], o.status_arr()):
            f["status"], f["caught"] = None, True

    def _shown(self, name, own):
        return own() if self.forced is None or self.forced[name] is None else self.forced[name]

    def screen(self):
        return self._shown("screen", self.o.screen)

    def hist(self):
        return self._shown("hist", self.o.hist)

    def status_arr(self):
        return self._shown("status", self.o.status_arr)

    def flags(self):
        f = self.o.flags()
        return f if self.forced is None or self.forced["message"] is None else dict(f, message=0)


class CallModel:
    def __init__(self, cfg, seeds, max_steps, wrong=None):
        assert wrong is None or wrong in WRONG
        self.cfg, self.max_steps, self.wrong = dict(cfg), int(max_steps), wrong
        self.n = len(seeds)
        self.seed = [int(s) for s in seeds]   # what the header says each env's next reset of any kind uses
        self.cur = list(self.seed)            # what the OracleEnv's next reset uses (differs from `seed` only under a misreading)
        self.env = [self.fresh(s) for s in self.seed]
        self.lin = [[s] for s in self.seed]
        self.h, self.w, self.symbols = self.env[0].h, self.env[0].w, self.env[0].symbols
        self.hw = self.h * self.w
        self.bonus = 0.0
        self.bound, self.tail = None, True     # rg_obs_bind's kind or None; rg_tail_encode
        self.slots = {}                        # slot -> list of lineages: the records of one rg_state_save
        self.tile_pending = False              # an InvalidTile the next rg_sync reports
        self.stats = dict(calls=0, steps=0, resets=0, descents=0, loads=0, loads_on_stairs=0, forced_descents=0)
        self.odd, self.force_term, self.status_over = set(), set(), {}   # (misreadings only)

    # ---- the oracle side ----
    def fresh(self, seed, max_steps=None):
        return Lane(self.cfg, self.max_steps if max_steps is None else max_steps, seed)

    def replay(self, lineage, max_steps=None):
        """A fresh OracleEnv played through a lineage: the clone a state record stands for."""
        o = self.fresh(lineage[0], max_steps)
        for k in lineage[1:]:
            if k == DESCEND:
                o.debug_descend()
            else:
                o.step_autoreset(int(k))
        return o

    def on_stairs(self, e):
        o = self.env[e]
        sc = o.scalars()
        return int(o.grid()[0][sc["py"], sc["px"]]) == S_STAIR

    def _touch(self, e):
        self.force_term.discard(e)

    def shown_terminal(self, e):
        return bool(self.env[e].flags()["is_terminal"]) or e in self.force_term

    def _rebuild(self, e):
        """reset() of one env: from its seed, an empty lineage."""
        self._touch(e)
        self.status_over.pop(e, None)
        o = self.env[e]
        if self.cur[e] != self.seed[e]:
            self.cur[e] = self.seed[e]
            o.set_seed(self.seed[e])
        if e in self.odd:
            self.odd.discard(e)
            o = self.env[e] = self.fresh(self.cur[e])
        else:
            o.reset()
        self.lin[e] = [self.cur[e]]

    def _play(self, e, key):
        """step_autoreset of one env -> (reward, done)."""
        self._touch(e)
        o = self.env[e]
        level0, status0 = o.scalars()["level"], o.status_arr()
        gold0 = int(status0[1])
        o.step_autoreset(int(key))
        term = bool(o.flags()["is_terminal"])
        if term or not np.array_equal(status0, o.status_arr()):   # (load_keeps_status: the mirror is rewritten when the status changes)
            self.status_over.pop(e, None)
        reward = float(max(0, int(o.status_arr()[1]) - gold0))
        if term:
            self.stats["resets"] += 1
            self.lin[e] = [self.cur[e]]
            if self.cur[e] != self.seed[e]:   # (seed_ignored: the seed arrives one episode late)
                self.cur[e] = self.seed[e]
                o.set_seed(self.seed[e])
            if e in self.odd:                 # (a misreading's env with another step budget: the next episode is an ordinary one)
                self.odd.discard(e)
                self.env[e] = self.fresh(self.lin[e][0])
                if self.cur[e] != self.lin[e][0]:
                    self.env[e].set_seed(self.cur[e])
                self.force_term.add(e)
        else:
            self.lin[e].append(int(key))
            if o.scalars()["level"] > level0:  # StairRewardParallel: the reported level rose and the episode goes on
                self.stats["descents"] += 1
                reward += self.bonus
        return reward, term

    # ---- what the library shows ----
    def status(self, e):
        return self.status_over[e] if e in self.status_over else self.env[e].status_arr()

    def mirrors(self):
        n = self.n
        scr, hist = np.empty((n, self.h, self.w), np.uint8), np.empty((n, self.h, self.w), np.uint8)
        st, term, dead, msg = np.empty((n, 10), np.uint32), np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, np.uint32)
        for e, o in enumerate(self.env):
            scr[e], hist[e], st[e] = o.screen(), o.hist(), self.status(e)
            f = o.flags()
            term[e], dead[e], msg[e] = self.shown_terminal(e), f["dead"], f["message"]
        return dict(screen=scr, hist=hist, status=st, terminal=term, dead=dead, message=msg)

    def images(self, kind, flag, with_hist):
        """(f32 [n, C, H, W], skip bool [n]): skip marks the envs whose one-hot image the reference refuses."""
        c = (self.symbols if kind else 1) + popcount(flag) + int(bool(with_hist))
        out, skip = np.zeros((self.n, c, self.h, self.w), np.float32), np.zeros(self.n, bool)
        for e, o in enumerate(self.env):
            try:
                out[e] = encode_image(kind, o.screen(), self.status(e), self.symbols, flag & 0x1FF, o.hist() if with_hist else None)
            except RuntimeError:
                skip[e] = True
        if skip.any():
            self.tile_pending = True
        return out, skip

    def centers(self):
        return np.array([[o.scalars()["py"], o.scalars()["px"]] for o in self.env], np.int32)

    def id_planes(self, with_hist):
        planes = [np.stack([tu.symbol_ids(o.screen()) for o in self.env])]
        if with_hist:
            planes.append(np.stack([o.hist() for o in self.env]))
        return np.stack(planes, 1).astype(np.uint8)

    def refused(self, spec):
        """The observation calls this grid has no kernel for (include/rogue_gym_hip.h: refused before anything is launched or stepped)."""
        t = spec["type"]
        if t == "typed":
            return spec["dtype"] != tu.RG_OBS_F32 and self.hw % (16 if spec["dtype"] == tu.RG_OBS_U8 else 8) != 0
        return t in ("compact", "fetch") and self.hw % 4 != 0

    def observe(self, spec):
        t = spec["type"]
        if t in ("gray", "symbol", "host", "compact"):
            kind = spec.get("kind", 1 if t == "symbol" else 0)
            img, skip = self.images(kind, spec["flag"], spec["hist"])
            out = dict(img=img, skip=skip)
            if t == "compact":
                out["status"] = np.stack([self.status(e) for e in range(self.n)]).astype(np.uint32)
            return out
        if t == "typed":
            if spec["kind"] == 2:
                ids = self.id_planes(spec["hist"])
                if (ids[:, 0] >= self.symbols - 1).any():
                    self.tile_pending = True
                return dict(ids=ids)
            img, skip = self.images(spec["kind"], spec["flag"], spec["hist"])
            return dict(bits=tu.bits16(img, spec["dtype"]), skip=skip)
        if t == "crop":
            ry, rx, cen = spec["ry"], spec["rx"], self.centers()
            if spec["kind"] == 2:
                ids = self.id_planes(spec["hist"]).astype(np.float32)
                win = np.stack([crop_window(ids[e], int(cen[e, 0]), int(cen[e, 1]), ry, rx, 0, 1, spec["hist"]) for e in range(self.n)]).astype(np.uint8)
                if (win[:, 0] >= self.symbols - 1).any():
                    self.tile_pending = True
                return dict(ids=win, center=cen)
            img, _ = self.images(0, spec["flag"], spec["hist"])
            win = np.stack([crop_window(img[e], int(cen[e, 0]), int(cen[e, 1]), ry, rx, 0, 1, spec["hist"]) for e in range(self.n)])
            return dict(center=cen, **({"img": win, "skip": np.zeros(self.n, bool)} if spec["dtype"] == tu.RG_OBS_F32 else {"bits": tu.bits16(win, spec["dtype"])}))
        if t == "pixels":
            font, pal = tileset()
            return dict(pixels=pixel_util.full_images(font, pal, np.stack([o.screen() for o in self.env]), spec["channels"]))
        if t == "fetch":
            return self.mirrors()
        if t == "status_vec":
            k, out = popcount(spec["flag"]), np.zeros((self.n, 9), np.int32)
            for e in range(self.n):
                st = np.ascontiguousarray(np.asarray(self.status(e), np.uint32))
                assert oracle_lib().orc_status_vec(st.ctypes.data, spec["flag"], out[e].ctypes.data) == k
            return dict(status_vec=out[:, :k].copy())
        raise ValueError(t)

    # ---- one program entry ----
    def apply(self, op):
        call, a = op
        self.stats["calls"] += 1
        return getattr(self, "_" + call)(a)

    def _step(self, a):
        keys, n_keys = a["keys"], len(a["keys"])
        self.stats["steps"] += 1
        reward, done = np.zeros(self.n, np.float32), np.zeros(n_keys, bool)
        for e in range(n_keys):
            reward[e], done[e] = self._play(e, keys[e])
        if self.wrong == "prefix_dot":
            for e in range(n_keys, self.n):
                self._play(e, ord("."))
        return dict(reward=reward, done=done)

    def _step_obs(self, a):
        if self.refused(a["obs"]):
            return dict(refused=np.ones(1, bool))
        out = self._step(a)
        out.update(self.observe(a["obs"]))
        return out

    def _obs(self, a):
        return dict(refused=np.ones(1, bool)) if self.refused(a["obs"]) else self.observe(a["obs"])

    def _mirror(self, a):
        return self.mirrors()

    def _reader(self, a):
        # (the library's answer is held against its own host twin on the device's cells; the model adds where the sampled players stand)
        sc = [self.env[e].scalars() for e in a["envs"]]
        return dict(player=np.array([[s["px"], s["py"], s["level"]] for s in sc], np.int32))

    def _reset(self, a):
        for e in range(self.n):
            self._rebuild(e)
        return {}

    def _reset_envs(self, a):
        if a["seeds"] is not None:
            self._seed(dict(ids=a["ids"], seeds=a["seeds"]))
        for e in a["ids"]:
            if self.wrong == "reset_keeps_steps":
                steps = self.env[e].flags()["steps"]
                self._rebuild(e)
                if steps:
                    self.env[e] = self.fresh(self.cur[e], self.max_steps - steps)
                    self.odd.add(e)
            else:
                self._rebuild(e)
        return {}

    def _seed(self, a):
        ids = range(len(a["seeds"])) if a["ids"] is None else a["ids"]
        for e, s in zip(ids, a["seeds"]):
            self.seed[e] = int(s)
            if self.wrong != "seed_ignored":
                self.cur[e] = int(s)
                self.env[e].set_seed(int(s))
        return {}

    def _descend(self, a):
        self.stats["forced_descents"] += 1
        for e, o in enumerate(self.env):   # (the oracle keeps is_terminal through it: so does a forced one)
            self.status_over.pop(e, None)
            o.debug_descend()
            self.lin[e].append(DESCEND)
        return {}

    def _save(self, a):
        # a record: the lineage, and whether the env shows the forced is_terminal of an auto-reset (a record carries the flag word)
        self.slots[a["slot"]] = [(list(self.lin[e]), self.shown_terminal(e)) for e in (range(self.n) if a["ids"] is None else a["ids"])]
        return {}

    def _load(self, a):
        rec = self.slots[a["slot"]]
        for row, d in a["pairs"]:
            (lin, shown), old = rec[row], self.env[d]
            old_steps, old_status = old.flags()["steps"], np.array(self.status(d))
            self._touch(d)
            self.status_over.pop(d, None)
            self.odd.discard(d)
            o = self.replay(lin)
            if shown and not o.flags()["is_terminal"]:
                self.force_term.add(d)
            if self.wrong == "load_keeps_steps" and old_steps != o.flags()["steps"]:
                o = self.replay(lin, self.max_steps - (old_steps - o.flags()["steps"]))
                self.odd.add(d)
            if self.wrong == "load_seed":
                self.seed[d] = self.cur[d] = lin[0]
            else:
                self.cur[d] = self.seed[d]
                o.set_seed(self.seed[d])
            if self.wrong == "load_keeps_status":
                self.status_over[d] = old_status
            self.env[d], self.lin[d] = o, list(lin)
            self.stats["loads"] += 1
            self.stats["loads_on_stairs"] += int(self.on_stairs(d))
        return {}

    def _switch(self, a):
        what = a["what"]
        if what == "tail":
            self.tail = bool(a["on"])
        elif what == "bind":
            self.bound = a["kind"]
        elif what == "stair":
            self.bonus = float(a["bonus"])
        else:  # rg_sync: non-zero exactly when an InvalidTile is pending
            rc, self.tile_pending = self.tile_pending, False
            return dict(sync=np.array([int(rc)]))
        return {}


def run(cfg, seeds, max_steps, ops, wrong=None):
    """The model's outputs for a whole program, and the model."""
    m = CallModel(cfg, seeds, max_steps, wrong)
    return [m.apply(op) for op in ops], m


def differences(exp, got):
    """Names of the outputs of one call that differ (tolerance 0), each with the first envs that do.  `skip` masks envs out of `img` / `bits`."""
    out = []
    assert set(exp) == set(got), (sorted(exp), sorted(got))
    skip = exp.get("skip")
    for name in sorted(exp):
        if name == "skip":
            continue
        x, y = np.ascontiguousarray(exp[name]), np.ascontiguousarray(got[name])
        if x.shape != y.shape or x.dtype != y.dtype:
            out.append((name, "%s %s vs %s %s" % (x.dtype, x.shape, y.dtype, y.shape)))
            continue
        if name in ("img", "bits") and skip is not None and skip.any():
            x, y = x[~skip], y[~skip]
        if x.dtype == np.float32:   # bit patterns: -0.0 and NaN payloads count
            x, y = x.view(np.uint32), y.view(np.uint32)
        if not np.array_equal(x, y):
            rows = np.flatnonzero((x != y).reshape(len(x), -1).any(1)) if x.ndim and len(x) == len(y) and len(x) else []
            out.append((name, [int(r) for r in rows[:8]]))
    return out


def compared(op, out):
    """What of one call's model outputs the GPU harness holds against the library: `skip` is a mask, not an output, and rg_step_fetch without screens
    delivers no screen and no history."""
    out = {k: v for k, v in out.items() if k != "skip"}
    if op[0] == "step_obs" and op[1]["obs"]["type"] == "fetch" and not op[1]["obs"]["screens"]:
        out.pop("screen", None), out.pop("hist", None)
    return out


class VecModel(CallModel):
    """The model of a program over HipVecRogueEnv's public methods (call_programs.vec_program), built with episodes, novelty, the legal-action mask, an
    archive and one added crop view.  After EVERY call the env refreshes obs, the crop view and the mask (device.py _refresh / _after_step), so every call's
    outputs are: obs, the crop view and its centres, the mask, ep_return and ep_length -- and reward and done behind a step.
    Episode accounting (include/rogue_gym_hip.h): a step adds the reward as one f32 add and 1 to the length, a done zeroes both; reset, reset_envs and
    archive_restore cut with a record, cut_episodes as asked -- return 0, length the game's own step counter; load_state and clone_state leave it alone.
    The archive (csrc/rg_archive.h): per key the best offer by (score = pack gold, fewer steps, lower env); a later equal offer replaces nothing."""
    CROP = dict(type="crop", kind=0, dtype=tu.RG_OBS_F16, ry=3, rx=5, flag=0x1FF, hist=1)

    def __init__(self, cfg, seeds, max_steps):
        super().__init__(cfg, seeds, max_steps)
        self.ep_ret, self.ep_len, self.arc = np.zeros(self.n, np.float32), np.zeros(self.n, np.int32), {}

    def shown(self):
        import mask_util

        crop = self.observe(self.CROP)
        return dict(obs=self.observe(dict(type="gray", flag=0, hist=0))["img"], crop=crop["bits"], center=crop["center"],
                    mask=np.stack([mask_util.oracle_row(o) for o in self.env]).astype(bool), ep_return=self.ep_ret.copy(), ep_length=self.ep_len.copy())

    def cut(self, ids):
        for e in ids:
            self.ep_ret[e], self.ep_len[e] = 0.0, self.env[e].flags()["steps"]

    def apply(self, op):
        self.stats["calls"] += 1
        out = getattr(self, "_v_" + op[0])(op[1]) or {}
        out.update(self.shown())
        return out

    def _v_step(self, a):
        out = self._step(a)
        self.ep_ret = (self.ep_ret + out["reward"]).astype(np.float32)
        self.ep_len += 1
        self.ep_ret[out["done"]], self.ep_len[out["done"]] = 0.0, 0
        return out

    def _v_reset(self, a):
        self._reset(a)
        self.cut(range(self.n))

    def _v_reset_envs(self, a):
        self._reset_envs(a)
        self.cut(a["ids"])

    def _v_seed(self, a):
        self._seed(dict(ids=None, seeds=a["seeds"]))

    def _v_save(self, a):
        self._save(a)

    def _v_load(self, a):
        self._load(a)

    def _v_clone(self, a):
        self._save(dict(slot="clone", ids=a["src"]))
        self._load(dict(slot="clone", pairs=list(enumerate(a["dst"]))))

    def _v_archive_update(self, a):
        best = {}
        for e, key in enumerate(a["keys"]):
            if a["mask"] is None or a["mask"][e]:
                offer = (self.env[e].scalars()["gold"], -self.env[e].flags()["steps"], -e)
                if key not in best or offer > best[key]:
                    best[key] = offer
        for key, (score, nsteps, ne) in best.items():
            if key not in self.arc or (score, nsteps) > self.arc[key][:2]:
                self.arc[key] = (score, nsteps, (list(self.lin[-ne]), self.shown_terminal(-ne)))

    def _v_archive_restore(self, a):
        self.slots["archive"] = [self.arc[k][2] for k in a["keys"]]
        self._load(dict(slot="archive", pairs=list(enumerate(a["ids"]))))
        self.cut(a["ids"])

    def _v_cut(self, a):
        self.cut(range(self.n) if a["ids"] is None else a["ids"])
