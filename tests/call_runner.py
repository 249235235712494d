"""The GPU side of the interleaved call programs (tests/call_programs.py): one _Handle driven through ctypes, entry by entry, each call's own outputs
held against the model (tests/call_model.py) with tolerance 0.

The harness makes no library call that the entry does not stand for: a stray rg_fetch_states would consume Redraw flags and change the path under test.
What it adds is inert: rg_dev_read (a copy on the handle's stream and a wait for it), rg_reward / rg_done (two pointers), and for a reader entry
rg_debug_fetch, whose cells feed the reader's host twin.  Output buffers are filled with 0xA5 before a call -- an env nobody serves shows -- except the
tensor that is bound at the time, which the caller must not write."""
import ctypes as C
import json
import time
import types

import numpy as np

import call_model as cm
import call_programs as cp
import typed_util as tu
from parity_util import compare_internal

SENTINEL = 0xA5
NP16 = np.uint16


def vp(x):
    return C.c_void_p(x)


class Runner:
    def __init__(self, profile, seed):
        import torch
        from rogue_gym_python import _rogue_gym as inner

        self.torch, self.profile, self.seed = torch, profile, seed
        cfg = cp.config(profile)
        self.hd = inner._Handle([json.dumps(dict(cfg, seed=s)) for s in cp.env_seeds(seed)], cp.MAX_STEPS, auto_reset=True)
        self.L, self.h = self.hd.L, self.hd.h
        self.n, self.H, self.W, self.symbols = self.hd.n, self.hd.height, self.hd.width, self.hd.symbols
        self.hw = self.H * self.W
        self.dev = torch.device("cuda", self.hd.device)
        self.R = self.hd.state_bytes()
        self.bufs, self.pinned, self.bound = {}, {}, None
        self.rooms = (cfg.get("dungeon", {}).get("room_num_x", 3), cfg.get("dungeon", {}).get("room_num_y", 3))

    def close(self):
        for p in self.pinned.values():
            self.L.rg_host_free(vp(p))
        self.pinned = {}
        self.hd.close()

    # ---- memory ----
    def check(self, rc, what=""):
        if rc:
            raise AssertionError("%s refused: %s" % (what, self.L.rg_last_error(self.h).decode()))

    def buf(self, name, nbytes, fill=True):
        """A device buffer of at least nbytes kept under `name` (16-byte aligned: torch's allocations are)."""
        t = self.bufs.get(name)
        if t is None or t.numel() < nbytes:
            assert name not in ("T0", "TS") or t is None, "a tensor that may be bound never moves"
            t = self.bufs[name] = self.torch.empty(max(nbytes, 16), dtype=self.torch.uint8, device=self.dev)
        if fill:
            t.fill_(SENTINEL)
        self.torch.cuda.synchronize(self.dev)
        assert t.data_ptr() % 16 == 0
        return t

    def read(self, ptr, dtype, shape):
        out = np.empty(shape, dtype)
        self.check(self.L.rg_dev_read(self.h, vp(ptr), out.ctypes.data, out.nbytes), "rg_dev_read")
        return out

    def pin(self, name, nbytes):
        if name not in self.pinned:
            p = C.c_void_p()
            assert self.L.rg_host_alloc(nbytes, C.byref(p)) == 0
            self.pinned[name] = p.value
        C.memset(self.pinned[name], SENTINEL, nbytes)
        return self.pinned[name]

    def keys_arg(self, keys, dev):
        arr = np.frombuffer(keys, np.uint8).copy()
        if not dev:
            return arr, vp(arr.ctypes.data), 0
        t = self.torch.from_numpy(arr).to(self.dev)
        self.torch.cuda.synchronize(self.dev)
        return t, vp(t.data_ptr()), 1

    def ids_arg(self, ids, dev):
        arr = np.asarray(ids, np.int32).copy()
        if not dev:
            return arr, vp(arr.ctypes.data), 0
        t = self.torch.from_numpy(arr).to(self.dev)
        self.torch.cuda.synchronize(self.dev)
        return t, vp(t.data_ptr()), 1

    def reward_done(self, n_keys):
        rp, dp = C.c_void_p(), C.c_void_p()
        self.check(self.L.rg_reward(self.h, C.byref(rp)) or self.L.rg_done(self.h, C.byref(dp)))
        return dict(reward=self.read(rp.value, np.float32, self.n), done=self.read(dp.value, np.uint8, self.n)[:n_keys].astype(bool))

    @staticmethod
    def flag_parts(flags):
        flags = flags.astype(np.uint32)
        return dict(terminal=(flags & 1) != 0, dead=(flags & 2) != 0, message=(flags >> 8) & 0x7F)

    # ---- observations: `step` is None or the (pointer, on-device) pair of a fused step's keys; returns None where the library refuses ----
    def observe(self, spec, step=None, n_keys=None):
        L, h, n, H, W, t = self.L, self.h, self.n, self.H, self.W, spec["type"]
        flag, hist = spec.get("flag", 0), spec.get("hist", 0)
        planes = cm.popcount(flag) + hist
        if t in ("gray", "symbol"):
            kind = int(t == "symbol")
            shape = (n, (self.symbols if kind else 1) + planes, H, W)
            is_bound = self.bound is not None and spec["buf"] == ("T0", "TS")[self.bound]
            out = self.buf(spec["buf"], 4 * int(np.prod(shape)), fill=not is_bound)
            if step:
                assert kind == 0
                self.check(L.rg_step_obs_gray(h, step[0], step[1], flag, hist, vp(out.data_ptr())), "rg_step_obs_gray")
            else:
                self.check((L.rg_obs_symbol if kind else L.rg_obs_gray)(h, flag, hist, vp(out.data_ptr())), "rg_obs_%s" % t)
            return dict(img=self.read(out.data_ptr(), np.float32, shape))
        if t == "typed":
            kind, dtype = spec["kind"], spec["dtype"]
            shape = (n, 1 + hist, H, W) if kind == 2 else (n, 1 + planes, H, W)
            out = self.buf("typed", (1 if kind == 2 else 2) * int(np.prod(shape)))
            rc = (L.rg_step_obs_typed(h, step[0], step[1], kind, dtype, flag, hist, vp(out.data_ptr())) if step else
                  L.rg_obs_typed(h, kind, dtype, flag, hist, vp(out.data_ptr())))
            if rc:
                assert "multiple of" in L.rg_last_error(h).decode(), L.rg_last_error(h).decode()
                return None
            return dict(ids=self.read(out.data_ptr(), np.uint8, shape)) if kind == 2 else dict(bits=self.read(out.data_ptr(), NP16, shape))
        if t == "crop":
            kind, dtype, ry, rx = spec["kind"], spec["dtype"], spec["ry"], spec["rx"]
            shape = (n, 1 + hist if kind == 2 else 1 + planes, 2 * ry + 1, 2 * rx + 1)
            size = tu_bytes(dtype)
            out, cen = self.buf("crop", size * int(np.prod(shape))), self.buf("centers", 8 * n)
            if step:
                self.check(L.rg_step_obs_crop_typed(h, step[0], step[1], kind, dtype, ry, rx, flag, hist, vp(out.data_ptr()), vp(cen.data_ptr())), "rg_step_obs_crop_typed")
            else:
                self.check(L.rg_obs_crop_typed(h, kind, dtype, ry, rx, flag, hist, vp(out.data_ptr()), vp(cen.data_ptr())), "rg_obs_crop_typed")
            got = dict(center=self.read(cen.data_ptr(), np.int32, (n, 2)))
            got["ids" if kind == 2 else "img" if dtype == tu.RG_OBS_F32 else "bits"] = self.read(out.data_ptr(), {1: np.uint8, 2: NP16, 4: np.float32}[size], shape)
            return got
        if t == "pixels":
            ch = spec["channels"]
            shape = (n, ch, H * 8, W * 8)   # the built-in tileset: 8 x 8 tiles
            out = self.buf("pixels", int(np.prod(shape)))
            self.check(L.rg_step_obs_pixels(h, step[0], step[1], ch, vp(out.data_ptr())) if step else L.rg_obs_pixels(h, ch, vp(out.data_ptr())), "rg_obs_pixels")
            return dict(pixels=self.read(out.data_ptr(), np.uint8, shape))
        if t == "fetch":
            st, fl = self.pin("status", 40 * n), self.pin("flags", 4 * n)
            scr, hi = (self.pin("screen", n * self.hw), self.pin("hist", n * self.hw)) if spec["screens"] else (None, None)
            rc = L.rg_step_fetch(h, step[0], n_keys, vp(scr), vp(hi), vp(st), vp(fl))
            if rc:
                assert "divisible by 4" in L.rg_last_error(h).decode(), L.rg_last_error(h).decode()
                return None
            got = dict(status=np.ctypeslib.as_array(C.cast(st, C.POINTER(C.c_uint32)), (n, 10)).copy())
            got.update(self.flag_parts(np.ctypeslib.as_array(C.cast(fl, C.POINTER(C.c_uint32)), (n,)).copy()))
            if scr:
                got["screen"] = np.ctypeslib.as_array(C.cast(scr, C.POINTER(C.c_uint8)), (n, H, W)).copy()
                got["hist"] = np.ctypeslib.as_array(C.cast(hi, C.POINTER(C.c_uint8)), (n, H, W)).copy()
            return got
        if t == "host":
            out = np.full((n, (self.symbols if spec["kind"] else 1) + planes, H, W), np.nan, np.float32)
            self.check(L.rg_obs_host(h, spec["kind"], flag, hist, out.ctypes.data), "rg_obs_host")
            return dict(img=out)
        if t == "compact":
            ph = spec["packed_hist"]
            if self.hw % 4:
                packed = self.buf("packed", n * (2 * self.hw + 48))
                assert L.rg_pack_compact(h, ph, vp(packed.data_ptr())) != 0, "rg_pack_compact on a grid with H*W % 4 != 0"
                return None
            rec = L.rg_compact_record_bytes(h, ph)
            assert rec == self.hw + 48 + (self.hw if ph else 0)
            shape = (n, (self.symbols if spec["kind"] else 1) + planes, H, W)
            packed, out = self.buf("packed", n * rec), self.buf("expanded", 4 * int(np.prod(shape)))
            self.check(L.rg_pack_compact(h, ph, vp(packed.data_ptr())), "rg_pack_compact")
            self.check(L.rg_expand_compact(h, vp(packed.data_ptr()), n, ph, spec["kind"], flag, hist, vp(out.data_ptr())), "rg_expand_compact")
            raw = self.read(packed.data_ptr(), np.uint8, (n, rec))
            return dict(img=self.read(out.data_ptr(), np.float32, shape), status=raw[:, self.hw:self.hw + 40].copy().view(np.uint32))
        assert t == "status_vec"
        k = cm.popcount(flag)
        out = np.full((n, k), -7, np.int32)
        self.check(L.rg_status_vec(h, flag, out.ctypes.data), "rg_status_vec")
        return dict(status_vec=out)

    # ---- one entry ----
    def apply(self, op):
        return getattr(self, "_" + op[0])(op[1])

    def _step(self, a):
        hold, p, on = self.keys_arg(a["keys"], a["dev"])
        self.check(self.L.rg_step_prefix(self.h, p, len(a["keys"]), on) if a["prefix"] else self.L.rg_step(self.h, p, on), "rg_step")
        return self.reward_done(len(a["keys"]))

    def _step_obs(self, a):
        hold, p, on = self.keys_arg(a["keys"], a["dev"])
        got = self.observe(a["obs"], (p, on), len(a["keys"]))
        if got is None:
            return dict(refused=np.ones(1, bool))
        got.update(self.reward_done(len(a["keys"])))
        return got

    def _obs(self, a):
        got = self.observe(a["obs"])
        return dict(refused=np.ones(1, bool)) if got is None else got

    def _mirror(self, a):
        n, H, W = self.n, self.H, self.W
        if a["how"] == "fetch":
            scr, hist, status, flags = self.hd.fetch()
        else:
            p = [C.c_void_p() for _ in range(4)]
            for f, q in zip((self.L.rg_screen, self.L.rg_hist, self.L.rg_status, self.L.rg_flags), p):
                self.check(f(self.h, C.byref(q)), "mirror pointer")
            scr, hist = self.read(p[0].value, np.uint8, (n, H, W)), self.read(p[1].value, np.uint8, (n, H, W))
            status, flags = self.read(p[2].value, np.int32, (n, 10)), self.read(p[3].value, np.uint32, n)
        return dict(screen=scr, hist=hist, status=status.view(np.uint32) if status.dtype == np.int32 else status, **self.flag_parts(flags))

    def _reader(self, a):
        L, h, n, H, W, which = self.L, self.h, self.n, self.H, self.W, a["which"]
        glob = lambda: L.rg_last_error(None).decode()  # noqa: E731
        if which == "action_mask":
            out = self.buf("reader", 16 * n)
            self.check(L.rg_action_mask(h, None, 0, vp(out.data_ptr()), vp(out.data_ptr() + 11 * n + (-11 * n) % 16), a["seed"], a["draw"]), "rg_action_mask")
            mask, sample = self.read(out.data_ptr(), np.uint8, (n, 11)), self.read(out.data_ptr() + 11 * n + (-11 * n) % 16, np.uint8, n)
        elif which == "path":
            out = self.buf("reader", 2 * n * self.hw + 16 * n)
            base, o_dist = out.data_ptr(), 2 * n * self.hw
            self.check(L.rg_path(h, a["goals"], None, vp(base) if a["field"] else None, vp(base + o_dist), vp(base + o_dist + 4 * n)), "rg_path")
            field = self.read(base, np.uint16, (n, H, W)) if a["field"] else None
            dist, key = self.read(base + o_dist, np.int32, n), self.read(base + o_dist + 4 * n, np.uint8, n)
        elif which == "route":
            out = self.buf("reader", 16 * n)
            base = out.data_ptr()
            self.check(L.rg_route(h, a["goals"], a["fallback"], a["mode"], None, vp(base), vp(base + 4 * n), vp(base + 5 * n)), "rg_route")
            dist, key, tier = self.read(base, np.int32, n), self.read(base + 4 * n, np.uint8, n), self.read(base + 5 * n, np.uint8, n)
        else:
            cap = a["cap"]
            out = self.buf("reader", n * cap * 16 + 16 * n)
            base = out.data_ptr()
            if which == "monsters":
                self.check(L.rg_monsters(h, a["mode"], cap, vp(base), vp(base + n * cap * 16)), "rg_monsters")
            else:
                self.check(L.rg_objects(h, a["kinds"], a["mode"], cap, vp(base), vp(base + n * cap * 16)), "rg_objects")
            table, words = self.read(base, np.int16, (n, cap, 8)), self.read(base + n * cap * 16, np.int32, (n, 4))
        player = []
        for e in a["envs"]:   # the host twin on the device's own cells
            d, cells = self.hd.debug_state(e)
            player.append([d.px, d.py, d.dungeon_level])
            where = "%s %s env %d" % (which, {k: v for k, v in a.items() if k != "envs"}, e)
            if which == "action_mask":
                row = np.full(11, 0xAA, np.uint8)
                assert L.rg_action_mask_host(cells.ctypes.data, H, W, d.px, d.py, 0, None, 0, row.ctypes.data) == 0, glob()
                assert np.array_equal(mask[e], row), (where, mask[e], row)
                legal = np.flatnonzero(row)
                want = cp.ACTION_KEYS[legal[L.rg_sample_index(a["seed"], e, a["draw"], len(legal))]] if len(legal) else cp.ACTION_KEYS[0]
                assert int(sample[e]) == want, (where, sample[e], want)
            elif which == "path":
                f, dd, kk = np.full((H, W), 0xAAAA, np.uint16), np.full(1, -7, np.int32), np.full(1, 0xAA, np.uint8)
                assert L.rg_path_host(cells.ctypes.data, H, W, d.px, d.py, 0, a["goals"], 0, 0, f.ctypes.data, dd.ctypes.data, kk.ctypes.data) == 0, glob()
                assert (int(dist[e]), int(key[e])) == (int(dd[0]), int(kk[0])), (where, dist[e], key[e], dd, kk)
                assert field is None or np.array_equal(field[e], f), where
            elif which == "route":
                dd, kk, tt = np.full(1, -7, np.int32), np.full(1, 0xAA, np.uint8), np.full(1, 0xAA, np.uint8)
                assert L.rg_route_host(cells.ctypes.data, H, W, d.px, d.py, 0, a["goals"], a["fallback"], a["mode"], 0, 0, None, dd.ctypes.data, kk.ctypes.data,
                                       tt.ctypes.data) == 0, glob()
                assert (int(dist[e]), int(key[e]), int(tier[e])) == (int(dd[0]), int(kk[0]), int(tt[0])), (where, dist[e], key[e], tier[e], dd, kk, tt)
            else:
                t_out, w_out = np.full((a["cap"], 8), -77, np.int16), np.full(4, -77, np.int32)
                if which == "monsters":
                    m = d.n_monsters
                    arr = [np.array(list(x[:m]) or [0], np.int32) for x in (d.mon_x, d.mon_y, d.mon_type, d.mon_active, d.mon_hp)]
                    rect, meta = np.array(d.room_rect[:d.n_rooms], np.uint32), np.array(d.room_meta[:d.n_rooms], np.int32)
                    rc = L.rg_monsters_host(cells.ctypes.data, H, W, d.px, d.py, 0, m, *(x.ctypes.data for x in arr), None, self.rooms[0], self.rooms[1], rect.ctypes.data,
                                            meta.ctypes.data, a["mode"], a["cap"], t_out.ctypes.data, w_out.ctypes.data)
                else:
                    rc = L.rg_objects_host(cells.ctypes.data, H, W, d.px, d.py, 0, a["kinds"], a["mode"], a["cap"], t_out.ctypes.data, w_out.ctypes.data)
                assert rc == 0, glob()
                if which == "monsters" and a["mode"] == 1:   # (column 7 is the monster's slot in the arrays given: the device's table, the debug copy's order)
                    table[e][:, 7] = t_out[:, 7]
                assert np.array_equal(table[e], t_out) and np.array_equal(words[e], w_out), (where, table[e], t_out, words[e], w_out)
        return dict(player=np.array(player, np.int32))

    def _reset(self, a):
        self.check(self.L.rg_reset(self.h), "rg_reset")
        return {}

    def seed_words(self, seeds):
        k = len(seeds)
        return (C.c_uint64 * k)(*[s & (1 << 64) - 1 for s in seeds]), (C.c_uint64 * k)(*[s >> 64 for s in seeds])

    def _reset_envs(self, a):
        if a["seeds"] is not None:
            self._seed(dict(ids=a["ids"], seeds=a["seeds"]))
        if a["how"] == "mask":
            mask = np.zeros(self.n, np.uint8)
            mask[a["ids"]] = 1
            hold, p, _ = self.keys_arg(mask.tobytes(), True)
            self.check(self.L.rg_reset_mask(self.h, p), "rg_reset_mask")
        else:
            hold, p, on = self.ids_arg(a["ids"], a["how"] == "dev")
            self.check(self.L.rg_reset_envs(self.h, p, len(a["ids"]), on), "rg_reset_envs")
        return {}

    def _seed(self, a):
        lo, hi = self.seed_words(a["seeds"])
        if a["ids"] is None:
            self.check(self.L.rg_seed(self.h, lo, hi, len(a["seeds"])), "rg_seed")
        else:
            ids = np.asarray(a["ids"], np.int32)
            self.check(self.L.rg_seed_envs(self.h, ids.ctypes.data, lo, hi, len(ids)), "rg_seed_envs")
        return {}

    def _descend(self, a):
        self.check(self.L.rg_debug_descend(self.h), "rg_debug_descend")
        return {}

    def _save(self, a):
        rec = self.buf("slot%d" % a["slot"], self.n * self.R)
        if a["ids"] is None:
            self.check(self.L.rg_state_save(self.h, None, 0, 0, vp(rec.data_ptr())), "rg_state_save")
        else:
            hold, p, on = self.ids_arg(a["ids"], a["dev"])
            self.check(self.L.rg_state_save(self.h, p, len(a["ids"]), on, vp(rec.data_ptr())), "rg_state_save")
        return {}

    def _load(self, a):
        rec = self.bufs["slot%d" % a["slot"]]
        runs = []   # maximal runs of consecutive record rows: one rg_state_load each
        for row, d in a["pairs"]:
            if runs and runs[-1][0] + len(runs[-1][1]) == row:
                runs[-1][1].append(d)
            else:
                runs.append((row, [d]))
        for row, dst in runs:
            hold, p, on = self.ids_arg(dst, a["dev"])
            self.check(self.L.rg_state_load(self.h, vp(rec.data_ptr() + row * self.R), self.R, p, len(dst), on), "rg_state_load")
        return {}

    def _switch(self, a):
        L, h, what = self.L, self.h, a["what"]
        if what == "tail":
            self.check(L.rg_tail_encode(h, a["on"]), "rg_tail_encode")
        elif what == "bind":
            kind = a["kind"]
            if kind is None:
                self.check(L.rg_obs_bind(h, 0, 0, 0, None), "rg_obs_bind")
            else:
                out = self.buf(("T0", "TS")[kind], 4 * self.n * (self.symbols if kind else 1) * self.hw, fill=self.bound != kind)
                self.check(L.rg_obs_bind(h, kind, 0, 0, vp(out.data_ptr())), "rg_obs_bind")
            self.bound = kind
        elif what == "stair":
            self.check(L.rg_set_stair_reward(h, a["bonus"]), "rg_set_stair_reward")
        else:
            rc = L.rg_sync(h)
            assert not rc or "Invalid tile" in L.rg_last_error(h).decode(), L.rg_last_error(h).decode()
            return dict(sync=np.array([int(rc != 0)]))
        return {}


def tu_bytes(dtype):
    return {tu.RG_OBS_F32: 4, tu.RG_OBS_F16: 2, tu.RG_OBS_BF16: 2, tu.RG_OBS_U8: 1}[dtype]


def run_program(profile, seed):
    """Plays the program of (profile, seed) on a new handle and holds every call against the model; then the internals and the mirrors of every env, rg_sync
    and the workload counters.  Returns a dict of counts and the wall time."""
    prog = cp.program(profile, seed)   # (generated before the clock starts: it plays the model once by itself)
    t0 = time.time()
    run, model = Runner(profile, seed), cm.CallModel(cp.config(profile), cp.env_seeds(seed), cp.MAX_STEPS)
    try:
        for i, op in enumerate(prog["ops"]):
            out, got = model.apply(op), run.apply(op)
            exp = cm.compared(op, out)   # (what the CPU proof digests, name for name)
            if "skip" in out:            # the envs whose one-hot image the reference refuses: masked out of both sides
                exp["skip"] = got["skip"] = out["skip"]
            diff = cm.differences(exp, got)
            assert not diff, "%s seed %d, call %d %s %s (after %s): differs from the model in %s" % (
                profile, seed, i, op[0], {k: v for k, v in op[1].items() if k != "keys"}, [o[0] for o in prog["ops"][max(0, i - 3):i]], diff)
        batch = types.SimpleNamespace(fetch=run.hd.fetch, debug=run.hd.debug_state)
        compare_internal(batch, model.env, range(run.n), "%s seed %d, end" % (profile, seed))
        end = run.apply(("mirror", dict(how="fetch")))   # (the model's own mirrors, shown_terminal included: not the lanes' flags)
        assert not cm.differences(model.mirrors(), end), ("%s seed %d, end" % (profile, seed), cm.differences(model.mirrors(), end))
        rc = run.L.rg_sync(run.h)
        assert rc == 0, "rg_sync at the end reports: " + run.L.rg_last_error(run.h).decode()
        out = (C.c_uint64 * 9)()
        run.check(run.L.rg_counters_ex(run.h, out, 9, 0), "rg_counters_ex")
        counts = dict(calls=len(prog["ops"]), auto_resets=int(out[0]), descents=int(out[1]), spare_takes=int(out[4]), structure_loads=int(out[8]),
                      loads_on_stairs=model.stats["loads_on_stairs"], model_resets=model.stats["resets"], model_descents=model.stats["descents"])
        assert counts["auto_resets"] == counts["model_resets"], counts   # (rg_step counts the auto-resets of its keyed envs: so does the model)
        assert counts["auto_resets"] > 0 and counts["spare_takes"] > 0 and counts["structure_loads"] > 0 and counts["loads_on_stairs"] > 0, counts
    finally:
        run.close()
    counts["seconds"] = round(time.time() - t0, 2)
    return counts


def run_vec_program(seed):
    """Plays call_programs.vec_program(seed) on a HipVecRogueEnv built with episodes, novelty, the legal-action mask, an archive and one added crop view, and
    holds obs, the crop view, the mask, ep_return and ep_length after EVERY call (reward and done behind a step) against call_model.VecModel."""
    import torch
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv

    prog = cp.vec_program(seed)
    t0 = time.time()
    cfg = cp.config("mini_plain")
    env = HipVecRogueEnv([dict(cfg, seed=s) for s in cp.env_seeds(seed)], max_steps=cp.MAX_STEPS, episodes=True, novelty="screen", action_mask=True, archive=1024,
                         archive_auto=False)
    model = cm.VecModel(cfg, cp.env_seeds(seed), cp.MAX_STEPS)
    c = model.CROP
    view = env.add_crop((c["ry"], c["rx"]), ImageSetting(DungeonType.GRAY, StatusFlag.FULL, True), obs_dtype=torch.float16)
    n, dev, saved, slot_of = env.num_envs, env.device, {}, {}

    def ids_of(ids, how):
        if how == "mask":
            m = torch.zeros(n, dtype=torch.bool)
            m[list(ids)] = True
            return dict(mask=m.to(dev))
        return dict(env_ids=torch.tensor(list(ids), dtype=torch.int64, device=dev) if how == "dev" else list(ids))

    try:
        for i, (call, a) in enumerate(prog["ops"]):
            got = {}
            if call == "step":
                _, reward, done = env.step_keys(torch.as_tensor(np.frombuffer(a["keys"], np.uint8).copy(), device=dev))
                got = dict(reward=reward.cpu().numpy(), done=done.cpu().numpy().astype(bool))
            elif call == "reset":
                env.reset()
            elif call == "reset_envs":
                env.reset_envs(seeds=a["seeds"], **ids_of(a["ids"], a["how"]))
            elif call == "seed":
                env.seed(a["seeds"])
            elif call == "save":
                saved[a["slot"]] = env.save_state(a["ids"])
            elif call == "load":
                rows = torch.tensor([r for r, _ in a["pairs"]], dtype=torch.int64, device=dev)
                env.load_state(saved[a["slot"]][rows], [d for _, d in a["pairs"]])
            elif call == "clone":
                env.clone_state(a["src"], a["dst"])
            elif call == "archive_update":
                keys = torch.tensor(a["keys"], dtype=torch.int64, device=dev)
                env.archive_update(keys=keys, mask=None if a["mask"] is None else torch.tensor(a["mask"], dtype=torch.bool, device=dev))
                slots = env.archive.slot.cpu().numpy()
                for e, k in enumerate(a["keys"]):
                    if a["mask"] is None or a["mask"][e]:
                        assert slots[e] >= 0 and slot_of.setdefault(k, int(slots[e])) == int(slots[e]), (i, e, k, slots[e])
            elif call == "archive_restore":
                slots = [slot_of[k] for k in a["keys"]]
                if a["dev"]:
                    env.archive_restore(torch.tensor(slots, dtype=torch.int32, device=dev), torch.tensor(a["ids"], dtype=torch.int32, device=dev))
                else:
                    env.archive_restore(slots, a["ids"])
            else:
                env.cut_episodes(record=a["record"], **({} if a["how"] == "all" else ids_of(a["ids"], a["how"])))
            got.update(obs=env.obs.cpu().numpy(), crop=view.obs.view(torch.int16).cpu().numpy().view(NP16), center=view.center.cpu().numpy(),
                       mask=env.action_mask.cpu().numpy().astype(bool), ep_return=env.ep_return.cpu().numpy(), ep_length=env.ep_length.cpu().numpy())
            diff = cm.differences(model.apply((call, a)), got)
            assert not diff, "vec seed %d, call %d %s %s (after %s): differs from the model in %s" % (
                seed, i, call, {k: v for k, v in a.items() if k not in ("keys", "mask")}, [o[0] for o in prog["ops"][max(0, i - 3):i]], diff)
        env.check_errors()
        compare_internal(types.SimpleNamespace(fetch=env._h.fetch, debug=env._h.debug_state), model.env, range(n), "vec seed %d, end" % seed)
        counts = dict(calls=len(prog["ops"]), auto_resets=env.counters()["resets"], model_resets=model.stats["resets"], loads=model.stats["loads"],
                      archive=env.archive_stats(), novelty_calls=env.novelty_stats()["calls"])
        assert counts["auto_resets"] == counts["model_resets"] > 0 and counts["archive"]["written"] > 0, counts
    finally:
        env.close()
    counts["seconds"] = round(time.time() - t0, 2)
    return counts
