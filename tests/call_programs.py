"""Interleaved C-ABI call programs: a list of (call, arguments), a pure function of (profile, seed).

A program opens with an Eulerian circuit of the complete digraph over the thirteen call CLASSES, loops included, so every ordered pair of classes is adjacent
exactly once; a random tail follows, weighted towards steps (max_steps = 24: every env times out several times; the spare slots, the bulk refill and the
urgent builds get work), with the six named TRIPLES put into it, and a coda of max_steps + 1 uninterrupted steps that shows every env's step counter.  Arguments are drawn at random but never invalid: ids in range and unique where a call
refuses duplicates, records only from a save of the same program, keys of the eleven actions.  The generator plays the model (tests/call_model.py) along, so
that arguments can depend on the state -- an env that stands on the stairs, envs that have timed out -- and still be a function of (profile, seed) alone.

Entries (call, arguments):
  step        keys (bytes, one per keyed env), dev (keys on the device), prefix (rg_step_prefix; else rg_step)
  step_obs    keys, dev, obs -- a step fused with the observation `obs`
  obs         obs
  mirror      how: "fetch" (rg_fetch_states) | "dev" (rg_screen / rg_hist / rg_status / rg_flags + rg_dev_read)
  reader      which: action_mask | path | route | monsters | objects, its arguments, envs: the stride sample held against the host twin
  reset       rg_reset
  reset_envs  ids, how: host | dev | mask, seeds (None, or one per id: rg_seed_envs first)
  seed        ids (None: rg_seed on a prefix), seeds
  save        slot, ids (None: all), dev        load   slot, pairs [(record row, destination env)], dev
  descend     rg_debug_descend
  switch      what: tail (on) | bind (kind 0 / 1 / None) | stair (bonus) | sync
An observation `obs` is a dict: type gray | symbol (flag, hist, buf) | typed (kind, dtype, flag, hist) | crop (kind, dtype, ry, rx, flag, hist) |
pixels (channels) | fetch (screens) | host (kind, flag, hist) | compact (packed_hist, kind, flag, hist) | status_vec (flag)."""
import json
import os

import numpy as np

import typed_util as tu
from call_model import CallModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ENVS, MAX_STEPS, SEEDS, TAIL = 82, 24, (1, 2, 3), 130   # 82 = ten groups of 8 plus 2 = one 64-env wave and a short one
ACTION_KEYS = b".hjklnbuy>s"
CLASSES = ("step", "step_own", "step_other", "obs_own", "obs_other", "mirror", "reader", "reset", "reset_envs", "seed", "saveload", "descend", "switch")
STEP_CLASSES = ("step", "step_own", "step_other")
TRIPLES = ("step_load_bound", "step_reset_tail", "seed_timeout_obs", "save_reset_load", "load_on_stairs", "unbind_step_rebind")
PROFILES = {   # config of tests/golden/reference_goldens.json, another grid size, whether the standing tensor is bound (rg_obs_bind)
    "mini_plain": dict(config="mini", size=None, bound=False),
    "mini_bound": dict(config="mini", size=None, bound=True),
    "default": dict(config="default", size=None, bound=False),
    "odd33x17": dict(config="mini", size=(33, 17), bound=False),
}
OWN = dict(type="gray", flag=0, hist=0, buf="T0")   # every profile's own observation: the plain gray image in the standing tensor
SEEK_TABLE = b"yku" b"h>l" b"bjn"
SLOTS = 3


def config(profile):
    p = PROFILES[profile]
    with open(os.path.join(ROOT, "tests", "golden", "reference_goldens.json")) as f:
        cfg = dict(json.load(f)["configs"][p["config"]])
    if p["size"]:
        cfg["width"], cfg["height"] = p["size"]
    return cfg


def env_seeds(seed):
    return [1000 * seed + 17 * i for i in range(N_ENVS)]


def class_of(op):
    call, a = op
    if call == "step_obs":
        return "step_own" if a["obs"] == OWN else "step_other"
    if call == "obs":
        return "obs_own" if a["obs"] == OWN else "obs_other"
    return "saveload" if call in ("save", "load") else call


def euler_circuit(k, rng):
    """A closed walk over the complete digraph on k vertices, loops included, that uses each of the k * k edges once (Hierholzer): k * k + 1 vertices."""
    out = {v: [int(x) for x in rng.permutation(k)] for v in range(k)}
    stack, path = [int(rng.randint(k))], []
    while stack:
        if out[stack[-1]]:
            stack.append(out[stack[-1]].pop())
        else:
            path.append(stack.pop())
    return path[::-1]


def seeker_key(screen, rng):
    """The stair-seeking policy of tests/test_gpu_reset_envs.py: '>' where no stairs are in sight (the player may stand on them), else a greedy step."""
    st, at = np.argwhere(screen == ord("%")), np.argwhere(screen == ord("@"))
    if len(st) == 0 or len(at) == 0:
        return ord(">")
    dy, dx = int(np.sign(st[0][0] - at[0][0])), int(np.sign(st[0][1] - at[0][1]))
    return SEEK_TABLE[(dy + 1) * 3 + dx + 1]


class _Gen:
    def __init__(self, profile, seed):
        self.profile, self.p = profile, PROFILES[profile]
        self.rng = np.random.RandomState(100 * sorted(PROFILES).index(profile) + seed)
        self.m = CallModel(config(profile), env_seeds(seed), MAX_STEPS)
        self.n, self.ops, self.aux, self.saved = self.m.n, [], [], {}

    # ---- plumbing ----
    def emit(self, op, aux=False):
        self.ops.append(op)
        self.aux.append(aux)
        out = self.m.apply(op)
        if self.m.tile_pending and op != ("switch", dict(what="sync")):
            self.emit(("switch", dict(what="sync")), aux=True)   # the InvalidTile of this call is collected at once (call_model.py)
        return out

    def pick(self, *choices):
        return choices[self.rng.randint(len(choices))]

    def subset(self, lo, hi, among=None):
        among = list(range(self.n)) if among is None else list(among)
        k = min(len(among), int(self.rng.randint(lo, hi + 1)))
        return [int(among[i]) for i in self.rng.permutation(len(among))[:k]]

    def keys(self, n_keys=None, seek=0.5, force=None):
        n_keys = self.n if n_keys is None else n_keys
        out = bytearray(n_keys)
        for e in range(n_keys):
            out[e] = seeker_key(self.m.env[e].screen(), self.rng) if self.rng.rand() < seek else ACTION_KEYS[self.rng.randint(len(ACTION_KEYS))]
        for e, k in (force or {}).items():
            out[e] = k
        return bytes(out)

    def seeds(self, k):
        return [int(self.rng.randint(1, 1 << 30)) | (int(self.rng.randint(1, 1 << 30)) << 70 if self.rng.rand() < 0.3 else 0) for _ in range(k)]

    # ---- observations ----
    def other_obs(self, fused):
        r, h, w = self.rng, self.m.h, self.m.w
        flag, hist = self.pick(0, 0x1FF, int(r.randint(1, 0x200))), int(r.randint(2))
        kinds = ["gray_full", "typed_ids", "typed_f16", "crop", "pixels"] + (["fetch"] if fused else ["gray2", "symbol", "host", "compact", "status_vec"])
        if not fused and self.m.bound == 1:
            kinds += ["bound_symbol"] * 3
        t = self.pick(*kinds)
        if t == "gray_full":
            return dict(type="gray", flag=0x1FF, hist=1, buf="T1")
        if t == "gray2":
            return dict(type="gray", flag=0, hist=0, buf="T2")
        if t == "symbol":
            return dict(type="symbol", flag=0x1FF, hist=1, buf="TS1")
        if t == "bound_symbol":
            return dict(type="symbol", flag=0, hist=0, buf="TS")
        if t == "typed_ids":
            return dict(type="typed", kind=2, dtype=tu.RG_OBS_U8, flag=0, hist=hist)
        if t == "typed_f16":
            return dict(type="typed", kind=0, dtype=self.pick(tu.RG_OBS_F16, tu.RG_OBS_BF16), flag=flag, hist=hist)
        if t == "crop":   # radii of half the grid: the window hangs off the grid for every player cell
            ids = bool(r.randint(2))
            return dict(type="crop", kind=2 if ids else 0, dtype=tu.RG_OBS_U8 if ids else self.pick(tu.RG_OBS_F32, tu.RG_OBS_F16), ry=h // 2, rx=w // 2,
                        flag=0 if ids else flag, hist=hist)
        if t == "pixels":
            return dict(type="pixels", channels=self.pick(1, 3))
        if t == "fetch":
            return dict(type="fetch", screens=bool(r.randint(2)))
        if t == "host":
            return dict(type="host", kind=int(r.randint(2)), flag=flag, hist=hist)
        if t == "compact":
            return dict(type="compact", packed_hist=max(hist, int(r.randint(2))), kind=int(r.randint(2)), flag=flag, hist=hist)
        return dict(type="status_vec", flag=self.pick(0x1FF, int(r.randint(1, 0x200))))

    # ---- one entry of a class ----
    def plain_step(self, seek=0.5, full=False, force=None):
        v = int(self.rng.randint(2 if full else 4))
        n_keys = self.n if v < 2 else int(self.rng.randint(1, self.n))
        return ("step", dict(keys=self.keys(n_keys, seek, force), dev=bool(v & 1), prefix=v >= 2))

    def save_op(self, ids="draw"):
        if ids == "draw":
            ids = None if self.rng.rand() < 0.5 else self.subset(1, 24)
        slot = int(self.rng.randint(SLOTS))
        self.saved[slot] = list(range(self.n)) if ids is None else list(ids)
        return ("save", dict(slot=slot, ids=ids, dev=bool(ids is not None and self.rng.randint(2))))

    def load_op(self, slot=None, pattern=None):
        slot = self.pick(*sorted(self.saved)) if slot is None else slot
        src = self.saved[slot]
        pattern = pattern or self.pick("perm", "fan", "rewind")
        if pattern == "perm":     # a move: record i into the i-th env of a shuffle -- one call
            pairs = list(zip(range(len(src)), self.subset(len(src), len(src))))
        elif pattern == "fan":    # one source into many destinations
            row = int(self.rng.randint(len(src)))
            pairs = [(row, d) for d in self.subset(2, 9)]
        else:                     # a rewind: some of the records back into the envs they came from
            pairs = sorted((int(i), src[i]) for i in self.rng.permutation(len(src))[:max(1, len(src) // 2)])
        return ("load", dict(slot=slot, pairs=[(int(r), int(d)) for r, d in pairs], dev=bool(pattern == "perm" and self.rng.randint(2))))

    def make(self, cls):
        r = self.rng
        if cls == "step":
            return self.plain_step()
        if cls == "step_own":
            return ("step_obs", dict(keys=self.keys(), dev=bool(r.randint(2)), obs=dict(OWN)))
        if cls == "step_other":
            obs = self.other_obs(True)
            if obs["type"] == "fetch":   # rg_step_fetch: host keys, zipped with the envs
                return ("step_obs", dict(keys=self.keys(self.pick(self.n, int(r.randint(1, self.n)))), dev=False, obs=obs))
            return ("step_obs", dict(keys=self.keys(), dev=bool(r.randint(2)), obs=obs))
        if cls == "obs_own":
            return ("obs", dict(obs=dict(OWN)))
        if cls == "obs_other":
            return ("obs", dict(obs=self.other_obs(False)))
        if cls == "mirror":
            return ("mirror", dict(how=self.pick("fetch", "dev")))
        if cls == "reader":
            which = self.pick("action_mask", "path", "route", "monsters", "objects")
            a = dict(which=which, envs=list(range(int(r.randint(7)), self.n, 7)))
            if which == "action_mask":
                a.update(seed=int(r.randint(1 << 30)), draw=int(r.randint(1000)))
            elif which == "path":
                a.update(goals=self.pick(1, 2, 3), field=bool(r.randint(2)))
            elif which == "route":
                a.update(zip(("goals", "fallback", "mode"), self.pick((1, 0, 1), (1, 8, 3), (3, 0, 0), (8, 1, 2))))
            elif which == "monsters":
                a.update(mode=int(r.randint(2)), cap=self.pick(1, 4, 16))
            else:
                a.update(zip(("kinds", "mode"), self.pick((7, 0), (15, 2), (5, 1), (15, 3))), cap=self.pick(1, 8, 32))
            return ("reader", a)
        if cls == "reset":
            return ("reset", {})
        if cls == "reset_envs":
            ids = self.subset(1, self.n // 3)
            how = self.pick("host", "dev", "mask")
            return ("reset_envs", dict(ids=sorted(ids) if how == "mask" else ids, how=how, seeds=self.seeds(len(ids)) if r.rand() < 0.3 else None))
        if cls == "seed":
            if r.rand() < 0.3:
                return ("seed", dict(ids=None, seeds=self.seeds(int(r.randint(1, self.n + 1)))))
            ids = self.subset(1, 10)
            return ("seed", dict(ids=ids, seeds=self.seeds(len(ids))))
        if cls == "saveload":
            return self.save_op() if not self.saved or r.rand() < 0.4 else self.load_op()
        if cls == "descend":
            return ("descend", {})
        v = self.pick("tail", "bind", "stair", "sync", "profile")
        if v == "tail":
            return ("switch", dict(what="tail", on=int(r.randint(2))))
        if v == "bind":
            return ("switch", dict(what="bind", kind=self.pick(0, 1, None)))
        if v == "stair":
            return ("switch", dict(what="stair", bonus=self.pick(0.0, 50.0, 0.5)))
        if v == "sync":
            return ("switch", dict(what="sync"))
        return self.profile_state()[0]   # back to what the profile is about

    def profile_state(self):
        ops = []
        if self.m.bound != (0 if self.p["bound"] else None):
            ops.append(("switch", dict(what="bind", kind=0 if self.p["bound"] else None)))
        if not self.m.tail or not ops:
            ops.append(("switch", dict(what="tail", on=1)))
        return ops

    # ---- the named triples ----
    def triple(self, name):
        m = self.m
        if name == "step_load_bound":         # a plain step, then a load, then the bound observation
            if m.bound != 0:
                self.emit(("switch", dict(what="bind", kind=0)))
            if not self.saved:
                self.emit(self.save_op())
            at = len(self.ops)
            for op in (self.plain_step(), self.load_op(), ("obs", dict(obs=dict(OWN)))):
                self.emit(op)
        elif name == "step_reset_tail":       # a plain step, then a partial reset, then the fused tail-encode step
            if m.bound is not None:
                self.emit(("switch", dict(what="bind", kind=None)))
            if not m.tail:
                self.emit(("switch", dict(what="tail", on=1)))
            at = len(self.ops)
            for cls in ("step", "reset_envs", "step_own"):
                self.emit(self.make(cls))
        elif name == "seed_timeout_obs":      # rg_seed_envs, then steps until every one of those envs has timed out (or died), then an observation
            ids = self.subset(5, 5)
            at = len(self.ops)
            self.emit(("seed", dict(ids=ids, seeds=self.seeds(5))))
            left = set(ids)
            while left:
                done = self.emit(self.plain_step(seek=0.0, full=True))["done"]
                left -= {e for e in left if done[e]}
            self.emit(self.make(self.pick("obs_own", "obs_other")))
        elif name == "save_reset_load":       # a save, then a reset of the source, then a load of it elsewhere
            src = self.subset(4, 12)
            rest = [e for e in range(self.n) if e not in src]
            at = len(self.ops)
            self.emit(self.save_op(ids=src))
            self.emit(("reset_envs", dict(ids=list(src), how="host", seeds=None)))
            slot = self.ops[at][1]["slot"]
            self.emit(("load", dict(slot=slot, pairs=[(i, int(d)) for i, d in enumerate(self.subset(len(src), len(src), rest))], dev=False)))
        elif name == "load_on_stairs":        # a load onto a player standing on stairs, then '>' as the next key
            for _ in range(3 * MAX_STEPS):
                if sum(m.on_stairs(e) for e in range(self.n)) >= 2:
                    break
                self.emit(self.plain_step(seek=1.0, full=True, force={e: ord(".") for e in range(self.n) if m.on_stairs(e)}))
            src = [e for e in range(self.n) if m.on_stairs(e)][:4]
            assert src, "no env reached the stairs"
            dst = self.subset(2 * len(src), 2 * len(src), [e for e in range(self.n) if e not in src])
            at = len(self.ops)
            self.emit(self.save_op(ids=src))
            slot = self.ops[at][1]["slot"]
            self.emit(("load", dict(slot=slot, pairs=[(i % len(src), int(d)) for i, d in enumerate(dst)], dev=False)))
            self.emit(self.plain_step(full=True, force={e: ord(">") for e in src + dst}))
        else:                                 # unbind, then a step, then rebind
            if m.bound is None:
                self.emit(("switch", dict(what="bind", kind=0)))
            at = len(self.ops)
            self.emit(("switch", dict(what="bind", kind=None)))
            self.emit(self.make(self.pick(*STEP_CLASSES)))
            self.emit(("switch", dict(what="bind", kind=0)))
        return at

    def build(self):
        if self.p["bound"]:
            self.emit(("switch", dict(what="bind", kind=0)))
        start = len(self.ops)
        for v in euler_circuit(len(CLASSES), self.rng):
            self.emit(self.make(CLASSES[v]))
        end = len(self.ops)
        triples, due = {}, {10 + 22 * i: name for i, name in enumerate(TRIPLES)}
        others = [c for c in CLASSES if c not in STEP_CLASSES]
        for i in range(TAIL):
            if i in due:
                for op in self.profile_state() if due[i] != "step_load_bound" else []:
                    self.emit(op)
                triples[due[i]] = self.triple(due[i])
                continue
            x = self.rng.rand()   # about 60 % steps
            self.emit(self.make("step" if x < 0.3 else "step_own" if x < 0.5 else "step_other" if x < 0.6 else self.pick(*others)))
        # the coda: a partial reset and a load of envs in mid-episode, then max_steps + 1 steps of every env with nothing between them -- each env's step
        # counter shows in the step at which it times out
        for op in self.profile_state():
            self.emit(op)
        for _ in range(4):
            self.emit(self.plain_step(full=True))
        src = self.subset(10, 10)
        self.emit(self.save_op(ids=src))
        slot = self.ops[-1][1]["slot"]
        self.emit(("descend", {}))   # (every env a level below the records: a loaded status differs from the one it replaces)
        for _ in range(5):
            self.emit(self.plain_step(full=True))
        self.emit(("reset_envs", dict(ids=self.subset(12, 12), how="dev", seeds=None)))
        self.emit(self.load_op(slot=slot, pattern="fan"))
        self.emit(self.load_op(slot=slot, pattern="rewind"))
        self.emit(("mirror", dict(how="fetch")))
        for i in range(MAX_STEPS + 1):
            self.emit(self.make("step_own") if i % 2 else self.plain_step(full=True))
        return dict(profile=self.profile, ops=self.ops, aux=self.aux, circuit=(start, end), triples=triples, stats=dict(self.m.stats))


_CACHE = {}


def program(profile, seed):
    """The program of (profile, seed): dict(ops, aux -- entries put in to collect an InvalidTile, not part of the walk --, circuit = (first, past-last) entry
    of the Eulerian circuit, triples = name -> first entry, stats = the model's counts)."""
    if (profile, seed) not in _CACHE:
        _CACHE[(profile, seed)] = _Gen(profile, seed).build()
    return _CACHE[(profile, seed)]


# ---- the shorter program over HipVecRogueEnv's public methods (mini only) ----
VEC_CLASSES = ("step", "reset", "reset_envs", "seed", "save", "load", "clone", "archive_update", "archive_restore", "cut")
VEC_TAIL, VEC_KEYS = 60, 12   # archive keys 1 .. 12: a dozen cells, so that offers meet stored records


class _VecGen(_Gen):
    def __init__(self, seed):
        from call_model import VecModel

        self.profile, self.p = "mini_plain", PROFILES["mini_plain"]
        self.rng = np.random.RandomState(7000 + seed)
        self.m = VecModel(config("mini_plain"), env_seeds(seed), MAX_STEPS)
        self.n, self.ops, self.aux, self.saved = self.m.n, [], [], {}

    def make(self, cls):
        r = self.rng
        if cls == "step":
            return ("step", dict(keys=self.keys()))
        if cls == "reset":
            return ("reset", {})
        if cls == "reset_envs":
            ids, how = self.subset(1, self.n // 3), self.pick("host", "dev", "mask")
            return ("reset_envs", dict(ids=sorted(ids) if how == "mask" else ids, how=how, seeds=self.seeds(len(ids)) if how == "host" and r.rand() < 0.5 else None))
        if cls == "seed":
            return ("seed", dict(seeds=self.seeds(int(r.randint(1, self.n + 1)))))
        if cls == "save":
            op = self.save_op()
            return ("save", dict(slot=op[1]["slot"], ids=op[1]["ids"]))
        if cls == "load":
            op = self.load_op()
            return ("load", dict(slot=op[1]["slot"], pairs=op[1]["pairs"]))
        if cls == "clone":   # one interesting env branched into many lanes, or a shuffle of a few (overlapping id sets are well defined)
            if r.rand() < 0.5:
                dst = self.subset(2, 12)
                return ("clone", dict(src=[int(r.randint(self.n))] * len(dst), dst=dst))
            ids = self.subset(4, 10)
            return ("clone", dict(src=ids, dst=ids[1:] + ids[:1]))
        if cls == "archive_update":
            salt = int(r.randint(VEC_KEYS))
            return ("archive_update", dict(keys=[1 + (3 * e + salt) % VEC_KEYS for e in range(self.n)], mask=None if r.rand() < 0.5 else [bool(v) for v in r.randint(0, 2, self.n)]))
        if cls == "archive_restore":
            ids = self.subset(1, 16)
            have = sorted(self.m.arc)
            return ("archive_restore", dict(keys=[have[int(r.randint(len(have)))] for _ in ids], ids=ids, dev=bool(r.randint(2))))
        ids, how = self.subset(1, self.n // 2), self.pick("host", "dev", "mask", "all")
        return ("cut", dict(ids=None if how == "all" else sorted(ids), how=how, record=bool(r.randint(2))))

    def build(self):
        for cls in ("step", "step", "step", "save", "archive_update"):   # (so that every load and every restore of the walk has a record to take)
            self.emit(self.make(cls))
        start = len(self.ops)
        for v in euler_circuit(len(VEC_CLASSES), self.rng):
            self.emit(self.make(VEC_CLASSES[v]))
        end = len(self.ops)
        for _ in range(VEC_TAIL):
            self.emit(self.make("step" if self.rng.rand() < 0.6 else self.pick(*VEC_CLASSES[1:])))
        for _ in range(MAX_STEPS + 1):   # the coda: every env's step counter shows in the step at which it times out
            self.emit(self.make("step"))
        return dict(profile="vec", ops=self.ops, aux=self.aux, circuit=(start, end), triples={}, stats=dict(self.m.stats))


def vec_program(seed):
    if ("vec", seed) not in _CACHE:
        _CACHE[("vec", seed)] = _VecGen(seed).build()
    return _CACHE[("vec", seed)]
