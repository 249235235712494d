"""CPU proof of the interleaved call programs (tests/call_programs.py) and of their model (tests/call_model.py), for every profile and seed: the circuit's
pairs and the named triples are there, no argument is invalid, a lineage replayed into a fresh oracle equals the env it was taken from, the model is
deterministic, and each of six misreadings of the header changes an output the GPU test (tests/test_gpu_call_programs.py) compares."""
import hashlib

import numpy as np
import pytest

import call_model as cm
import call_programs as cp

CASES = [(p, s) for p in sorted(cp.PROFILES) for s in cp.SEEDS]


def digest(out):
    """One call's outputs as name -> (dtype, shape, sha1): equal outputs, equal digests; a whole run's arrays would be gigabytes."""
    return {k: (str(np.asarray(v).dtype), np.asarray(v).shape, hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest()) for k, v in out.items()}


@pytest.fixture(scope="module")
def runs():
    """Per case, from ONE pass of the true model over the program, computed once and left alone: the program, the digest of every call's outputs, and what the
    other tests need of that pass -- the `done` bytes of the steps, the lineage proof (at every save, every saved lineage replayed into a fresh lane is
    compared with the env it was taken from), and whether the destinations of the load_on_stairs triple stood on stairs behind their load."""
    cache = {}

    def get(profile, seed):
        if (profile, seed) not in cache:
            prog = cp.program(profile, seed)
            m, outs, done, saves, bad, on_stairs = cm.CallModel(cp.config(profile), cp.env_seeds(seed), cp.MAX_STEPS), [], {}, 0, [], None
            for i, op in enumerate(prog["ops"]):
                out = m.apply(op)
                outs.append(digest(cm.compared(op, out)))
                if "done" in out:
                    done[i] = out["done"]
                if i == prog["triples"]["load_on_stairs"] + 1:
                    on_stairs = op[0] == "load" and all(m.on_stairs(d) for _, d in op[1]["pairs"])
                if op[0] == "save":
                    saves += 1
                    for (lin, shown), e in zip(m.slots[op[1]["slot"]], range(m.n) if op[1]["ids"] is None else op[1]["ids"]):
                        clone = m.replay(lin)
                        what = cm.same_state(clone, m.env[e], terminal=False)
                        if what or shown != m.shown_terminal(e) or (clone.flags()["is_terminal"] and not shown):
                            bad.append((i, e, what, shown))
            cache[(profile, seed)] = (prog, outs, dict(done=done, saves=saves, bad=bad, on_stairs=on_stairs))
        return cache[(profile, seed)]

    return get


def walk(prog):
    """The entries that belong to the walk (the rg_sync entries put in behind an InvalidTile do not), with their positions."""
    return [(i, op) for i, (op, aux) in enumerate(zip(prog["ops"], prog["aux"])) if not aux]


@pytest.mark.parametrize("profile,seed", CASES)
def test_coverage(profile, seed, runs):
    prog, _, facts = runs(profile, seed)
    ops = walk(prog)
    first, last = prog["circuit"]
    classes = [cp.class_of(op) for i, op in ops if first <= i < last]
    k = len(cp.CLASSES)
    assert len(classes) == k * k + 1 and classes[0] == classes[-1]
    pairs = list(zip(classes, classes[1:]))
    assert len(set(pairs)) == k * k == len(pairs), "every ordered pair of classes, loops included, exactly once"
    assert set(pairs) == {(a, b) for a in cp.CLASSES for b in cp.CLASSES}
    # the named triples, found by a scan of the whole program that does not trust the generator's own positions
    seq = [(cp.class_of(op), op) for _, op in ops]

    bound, tail, state = None, True, []
    for c, op in seq:   # (the switches' state BEFORE each entry)
        state.append((bound, tail))
        if c == "switch" and op[1]["what"] == "bind":
            bound = op[1]["kind"]
        if c == "switch" and op[1]["what"] == "tail":
            tail = bool(op[1]["on"])
    found = {name: False for name in cp.TRIPLES}
    for i in range(len(seq) - 2):
        (c0, o0), (c1, o1), (c2, o2) = seq[i:i + 3]
        if c0 == "step" and o1[0] == "load" and c2 == "obs_own" and state[i + 2][0] == 0:
            found["step_load_bound"] = True
        if c0 == "step" and c1 == "reset_envs" and c2 == "step_own" and state[i + 2] == (None, True):
            found["step_reset_tail"] = True
        if o0[0] == "save" and c1 == "reset_envs" and o2[0] == "load" and o0[1]["ids"] is not None and set(o1[1]["ids"]) == set(o0[1]["ids"]) \
                and o2[1]["slot"] == o0[1]["slot"] and not set(d for _, d in o2[1]["pairs"]) & set(o0[1]["ids"]):
            found["save_reset_load"] = True
        if c0 == "switch" and o0[1] == dict(what="bind", kind=None) and c1 in cp.STEP_CLASSES and o2[1] == dict(what="bind", kind=0) and state[i][0] is not None:
            found["unbind_step_rebind"] = True
    at = prog["triples"]["seed_timeout_obs"]   # rg_seed_envs, steps until each of those envs has ended an episode, then an observation
    ids, j = set(prog["ops"][at][1]["ids"]), at + 1
    assert prog["ops"][at][0] == "seed"
    while prog["ops"][j][0] == "step":
        ids -= {e for e in ids if e < len(facts["done"][j]) and facts["done"][j][e]}
        j += 1
    found["seed_timeout_obs"] = not ids and prog["ops"][j][0] == "obs"
    at = prog["triples"]["load_on_stairs"]      # a load onto a player standing on stairs, then '>' as the next key
    step = prog["ops"][at + 2]
    found["load_on_stairs"] = bool(facts["on_stairs"]) and step[0] == "step" and all(step[1]["keys"][d] == ord(">") for _, d in prog["ops"][at + 1][1]["pairs"])
    assert all(found.values()), found
    # every env times out several times; descents, forced descents and loads onto the stairs happen
    st = prog["stats"]
    assert st["resets"] >= 2 * cp.N_ENVS and st["descents"] > 0 and st["forced_descents"] > 0 and st["loads_on_stairs"] > 0, st
    print(profile, seed, "calls %d (aux %d)" % (len(prog["ops"]), sum(prog["aux"])), st)


@pytest.mark.parametrize("profile,seed", CASES)
def test_arguments_are_valid(profile, seed):
    prog = cp.program(profile, seed)
    if seed == cp.SEEDS[0]:   # (generated anew: a program is a function of (profile, seed) and of nothing else)
        assert cp._Gen(profile, seed).build()["ops"] == prog["ops"]
    n, saved = cp.N_ENVS, {}

    def ids_ok(ids, unique=True):
        return all(isinstance(e, int) and 0 <= e < n for e in ids) and (not unique or len(set(ids)) == len(ids))

    for call, a in prog["ops"]:
        if call in ("step", "step_obs"):
            assert 1 <= len(a["keys"]) <= n and set(a["keys"]) <= set(cp.ACTION_KEYS)
            if call == "step":
                assert a["prefix"] == (len(a["keys"]) < n)
            elif a["obs"]["type"] != "fetch":
                assert len(a["keys"]) == n
        if call in ("obs", "step_obs"):
            o = a["obs"]
            assert 0 <= o.get("flag", 0) <= 0x1FF
            if o["type"] == "crop":
                assert 0 <= o["ry"] <= 47 and 0 <= o["rx"] <= 159
            if o["type"] in ("typed", "crop"):
                assert (o["kind"] == 2) == (o["dtype"] == 3) and (o["kind"] != 2 or o["flag"] == 0)
            if o["type"] == "compact":
                assert o["hist"] <= o["packed_hist"]
        if call == "reset_envs":
            assert ids_ok(a["ids"]) and (a["seeds"] is None or len(a["seeds"]) == len(a["ids"]))
        if call == "seed":
            assert len(a["seeds"]) <= n if a["ids"] is None else (ids_ok(a["ids"], False) and len(a["seeds"]) == len(a["ids"]))
            assert all(0 <= s < 1 << 128 for s in a["seeds"])
        if call == "save":
            assert 0 <= a["slot"] < cp.SLOTS and (a["ids"] is None or (ids_ok(a["ids"], False) and a["ids"]))
            saved[a["slot"]] = n if a["ids"] is None else len(a["ids"])
        if call == "load":   # records come only from a save of this program; a load refuses duplicate destinations
            assert a["slot"] in saved and a["pairs"] and all(0 <= r < saved[a["slot"]] for r, _ in a["pairs"]) and ids_ok([d for _, d in a["pairs"]])
        if call == "reader":
            assert ids_ok(a["envs"]) and 1 <= a.get("cap", 1) <= (16 if a["which"] == "monsters" else 32)
        if call == "switch" and a["what"] == "stair":
            assert a["bonus"] >= 0


def test_replay_equals_direct_stepping():
    """40 seeds of the mini config, max_steps 40, 160 keys each with forced descents: after every key a fresh oracle played through the lineage equals the
    one that was stepped directly, and after set_seed(other) its next terminal step shows the first screen and status of a new game of `other`."""
    cfg, clones = cp.config("mini_plain"), 0
    for seed in range(40):
        m = cm.CallModel(cfg, [seed], 40)
        rng = np.random.RandomState(seed)
        for t in range(160):
            if rng.randint(25) == 0:
                m.apply(("descend", {}))
            m.apply(("step", dict(keys=bytes([cp.ACTION_KEYS[rng.randint(11)] if rng.randint(3) else cp.seeker_key(m.env[0].screen(), rng)]))))
            if t % 12 == 5:
                clone = m.replay(m.lin[0])
                # (straight after an auto-reset the env shows a new game with is_terminal forced: the model keeps that bit beside the lineage)
                assert cm.same_state(clone, m.env[0], terminal=len(m.lin[0]) > 1) is None, (seed, t, cm.same_state(clone, m.env[0]))
                clones += 1
                other = 5000 + seed
                clone.set_seed(other)
                while not clone.flags()["is_terminal"]:
                    clone.step_autoreset(ord("s"))
                new = m.fresh(other)
                assert np.array_equal(clone.screen(), new.screen()) and np.array_equal(clone.status_arr(), new.status_arr()), (seed, t)
    assert clones == 40 * 13


@pytest.mark.parametrize("profile,seed", CASES)
def test_lineages_at_every_save(profile, seed, runs):
    """At every save of a program, every saved lineage replayed equals the env it was taken from -- envs that were themselves loaded, rebuilt, reseeded,
    timed out and forced down a level before (the comparison is made in the `runs` fixture's one pass)."""
    facts = runs(profile, seed)[2]
    assert facts["saves"] >= 5 and not facts["bad"], (facts["saves"], facts["bad"][:5])

@pytest.mark.parametrize("profile,seed", CASES)
def test_determinism(profile, seed, runs):
    prog, first, _ = runs(profile, seed)
    m = cm.CallModel(cp.config(profile), cp.env_seeds(seed), cp.MAX_STEPS)
    assert len(first) == len(prog["ops"])
    for i, op in enumerate(prog["ops"]):
        assert digest(cm.compared(op, m.apply(op))) == first[i], (i, op[0])


@pytest.mark.parametrize("wrong", cm.WRONG)
@pytest.mark.parametrize("profile,seed", CASES)
def test_misreadings_show(profile, seed, wrong, runs):
    """A model that misreads the header differs from the true one in at least one output of at least one call: the GPU test, which holds every such output
    against the true model with tolerance 0, cannot pass a library that behaves like the misreading."""
    prog, true, _ = runs(profile, seed)
    m = cm.CallModel(cp.config(profile), cp.env_seeds(seed), cp.MAX_STEPS, wrong)
    for i, op in enumerate(prog["ops"]):
        if digest(cm.compared(op, m.apply(op))) != true[i]:   # (only what the GPU harness compares: call_model.compared)
            print("%s %d: '%s' shows at call %d (%s)" % (profile, seed, wrong, i, op[0]))
            return
    raise AssertionError("misreading '%s' changes no compared output" % wrong)


@pytest.mark.parametrize("seed", cp.SEEDS)
def test_vec_program_coverage_and_arguments(seed):
    """The program over HipVecRogueEnv's methods: every ordered pair of its ten classes once, valid arguments, a function of the seed, and a model that
    gives the same outputs twice."""
    prog = cp.vec_program(seed)
    first, last = prog["circuit"]
    classes = [op[0] for op in prog["ops"][first:last]]
    k = len(cp.VEC_CLASSES)
    pairs = list(zip(classes, classes[1:]))
    assert len(pairs) == k * k == len(set(pairs)) and set(pairs) == {(a, b) for a in cp.VEC_CLASSES for b in cp.VEC_CLASSES}
    assert cp._VecGen(seed).build()["ops"] == prog["ops"]
    n, saved, offered = cp.N_ENVS, {}, set()
    ok = lambda ids, unique=True: all(0 <= e < n for e in ids) and (not unique or len(set(ids)) == len(ids))  # noqa: E731
    for call, a in prog["ops"]:
        if call == "step":
            assert len(a["keys"]) == n and set(a["keys"]) <= set(cp.ACTION_KEYS)
        if call == "reset_envs":
            assert ok(a["ids"]) and (a["seeds"] is None or (a["how"] == "host" and len(a["seeds"]) == len(a["ids"])))
        if call == "save":
            saved[a["slot"]] = n if a["ids"] is None else len(a["ids"])
        if call == "load":
            assert all(0 <= r < saved[a["slot"]] for r, _ in a["pairs"]) and ok([d for _, d in a["pairs"]])
        if call == "clone":
            assert len(a["src"]) == len(a["dst"]) and ok(a["src"], False) and ok(a["dst"])
        if call == "archive_update":
            offered |= {key for e, key in enumerate(a["keys"]) if a["mask"] is None or a["mask"][e]}
        if call == "archive_restore":   # only slots that hold a record
            assert set(a["keys"]) <= offered and ok(a["ids"]) and len(a["keys"]) == len(a["ids"])
        if call == "cut":
            assert a["ids"] is None or ok(a["ids"])
    st = prog["stats"]
    assert st["resets"] >= cp.N_ENVS and st["loads"] > 0, st
    a, b = (cm.VecModel(cp.config("mini_plain"), cp.env_seeds(seed), cp.MAX_STEPS) for _ in range(2))
    for op in prog["ops"]:
        assert digest(a.apply(op)) == digest(b.apply(op))
    assert (a.ep_len > 0).any() and len(a.arc) > 3


def test_lane_behind_a_forced_descent_against_the_second_restatement():
    """The model's one part that is not the oracle's: what a lane shows behind a forced descent.  The second restatement (tests/shadow_turn.py) plays the same
    keys from the oracle's state with a Mirror that starts as rg_debug_descend leaves the library's -- status rewritten, screen and history of the new level
    drawn -- and follows GameStateImpl::react's rules through its OWN reaction lists, where the lane infers a Redraw from a change of the oracle's mirror:
    screen, history and status are equal after every key, real descents behind the forced one included."""
    from shadow_turn import Mirror, Shadow
    from test_oracle_shadow import M32, mixed_policy

    cfg = cp.config("mini_plain")
    d, keys_played, descents, lagged = cfg.get("dungeon", {}), 0, 0, 0
    for seed in range(60):
        rng = np.random.RandomState(900 + seed)
        m = cm.CallModel(cfg, [seed], 10 ** 6)
        lane, stuck, died = m.env[0], [0], False
        sh = Shadow(lane.w, lane.h, cfg.get("player", {}).get("hunger_time", 1300), d.get("passage_unlock_rate_inv", 3), d.get("door_unlock_rate_inv", 5))
        sh.new_game(lane.o)   # (from the episode's first key on: the Shadow's DistCache lives as long as the oracle's)

        def play(key):
            lineage = list(m.lin[0])

            def new_level():
                twin = m.replay(lineage)
                twin.debug_descend()
                sh.load_level(twin.o)

            dead = sh.process_action(key, new_level)
            m.apply(("step", dict(keys=bytes([ord(key)]))))
            return dead or lane.flags()["is_terminal"]

        for _ in range(int(rng.randint(0, 12))):
            died = died or play(mixed_policy(lane.o, rng, stuck))
        if died:
            continue
        m.apply(("descend", {}))   # actions::new_level alone, on both sides: the floor that is left joins the past floors
        sh.past_floors.append(sh.history_map())
        sh.load_level(lane.o)
        mirror = Mirror(sh)
        for t in range(60):
            key = mixed_policy(lane.o, rng, stuck)
            level0 = sh.level
            if play(key):
                break
            mirror.react(sh)
            keys_played, descents = keys_played + 1, descents + (sh.level > level0)
            lagged += int(lane.forced is not None)
            where = "seed %d key %d (%r), reactions %s, lane %s" % (seed, t, key, sh.reactions, None if lane.forced is None else {k: v is not None for k, v in lane.forced.items()})
            assert np.array_equal(lane.screen().reshape(-1), mirror.screen), where + ": screen"
            assert np.array_equal(lane.hist().reshape(-1), mirror.hist), where + ": history"
            assert [int(v) for v in lane.status_arr()] == [v & M32 for v in mirror.status], where + ": status"
    assert keys_played >= 2000 and descents >= 20 and lagged >= 200, (keys_played, descents, lagged)
