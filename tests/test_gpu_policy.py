"""rg_act on the GPU (rogue-gym_amd/csrc/rg_policy.hip k_act) against its host twin rg_act_host, byte for byte on every output -- floats as their bit
patterns: full and partial waves, dead envs, 80 x 24, every dtype, key lists of 1 to 32 keys, every mode, the mixing, the non-finite and underflowing rows;
config groups (the ext path); the mask output; no side effects; step_logits; the oracle in lock step under the keys act chose; the draw counter; the
refusals; the value API.  Shapes are the smallest that reach every path of the kernel."""
import ctypes as C
import json

import numpy as np
import pytest

import mask_util as mu
import policy_edge_rows as pe
import policy_util as pu
from parity_util import HipBatch, compare_internal, compare_mirrors, make_oracles
from policy_util import BF16, GIVEN, GREEDY, KEYS, LISTS, SAMPLE

pytestmark = pytest.mark.gpu
OUTS = ("key", "action", "logp", "entropy", "source")


def torch_mod():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def inner_mod():
    from rogue_gym_python import _rogue_gym as inner
    return inner


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def coded(x, dtype):
    """float32 rows as the host twin takes them for `dtype`: float32, float16, or the uint16 patterns of bfloat16."""
    if dtype == 0:
        return np.ascontiguousarray(x, np.float32)
    if dtype == 1:
        with np.errstate(over="ignore"):
            return x.astype(np.float16)
    return pu.to_bf16(x)


def to_device(torch, a, dev, dtype=None):
    """The device tensor of a host array; uint16 patterns become a bfloat16 tensor."""
    if dtype == BF16:
        return torch.from_numpy(a.view(np.int16).copy()).to(dev).view(torch.bfloat16)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def states_of(hd):
    """Per env what the host twin takes: (cells, height, width, px, py, dead)."""
    flags = np.empty(hd.n, np.uint32)
    hd.check(hd.L.rg_fetch_states(hd.h, None, None, None, flags.ctypes.data))
    out = []
    for e in range(hd.n):
        d, cells = hd.debug_state(e)
        out.append((cells, int(hd.env_heights[e]), int(hd.env_widths[e]), d.px, d.py, int(flags[e] >> 1) & 1))
    return out


def twin(hd, states, logits, dtype, keys, teacher=None, given=None, env_ids=None, **o):
    """rg_act_host over every env -> dict of arrays.  env_ids: the env index of each draw (default: the position in the handle)."""
    inner, L = inner_mod(), hd.L
    nk = len(KEYS) if keys is None else len(keys)
    out = dict(key=np.zeros(hd.n, np.uint8), action=np.zeros(hd.n, np.int32), logp=np.zeros(hd.n, np.float32), entropy=np.zeros(hd.n, np.float32), source=np.zeros(hd.n, np.uint8))
    opts = pu.opts_of(inner, **o)
    for e, (cells, h, w, px, py, dead) in enumerate(states):
        rc = L.rg_act_host(cells.ctypes.data, h, w, px, py, dead, keys, nk, logits[e].ctypes.data, dtype, C.byref(opts), e if env_ids is None else int(env_ids[e]), -1 if teacher is None else int(teacher[e]),
                           0 if given is None else int(given[e]), *[out[k][e:].ctypes.data for k in OUTS])
        assert rc == 0, L.rg_last_error(None).decode()
    return out


def device(hd, logits, dtype, keys, teacher=None, given=None, mask=False, **o):
    """rg_act on a raw handle into buffers pre-filled with 0xAA -> dict of arrays (and "mask" u8 [n][n_keys] when asked for)."""
    torch, inner = torch_mod(), inner_mod()
    dev = "cuda:%d" % hd.device
    nk = len(KEYS) if keys is None else len(keys)
    lg = to_device(torch, logits, dev, dtype)
    t = None if teacher is None else to_device(torch, np.asarray(teacher, np.uint8), dev)
    g = None if given is None else to_device(torch, np.asarray(given, np.int32), dev)
    bufs = dict(key=torch.full((hd.n,), 0xAA, dtype=torch.uint8, device=dev), action=torch.full((hd.n,), -7, dtype=torch.int32, device=dev),
                logp=torch.full((hd.n,), 7.0, dtype=torch.float32, device=dev), entropy=torch.full((hd.n,), 7.0, dtype=torch.float32, device=dev),
                source=torch.full((hd.n,), 0xAA, dtype=torch.uint8, device=dev))
    m = torch.full((hd.n, nk), 0xAA, dtype=torch.uint8, device=dev) if mask else None
    torch.cuda.synchronize()
    opts = pu.opts_of(inner, **o)
    hd.check(hd.L.rg_act(hd.h, keys, nk, ptr(lg), dtype, C.byref(opts), ptr(t), ptr(g), *[ptr(bufs[k]) for k in OUTS], ptr(m)))
    hd.check(hd.L.rg_sync(hd.h))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in bufs.items()}
    if mask:
        out["mask"] = m.cpu().numpy()
    return out


def assert_same(got, exp, where):
    for k in OUTS:
        a, b = got[k], exp[k]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b)
            raise AssertionError("%s: %s differs for %d envs, first env %d: device %r, host %r" % (where, k, len(bad), bad[0], got[k][bad[0]], exp[k][bad[0]]))


def sweep(hd, where, rs, teacher=None):
    """Every dtype x key list x mode, and the mixed SAMPLE, on the handle's present states; the sync error of a dead env's '.' is the caller's."""
    states = states_of(hd)
    rng = np.random.RandomState(rs)
    n, sources = hd.n, np.zeros(4, np.int64)
    if teacher is None:
        teacher = np.frombuffer(KEYS, np.uint8)[rng.randint(0, 11, n)]
    for dtype in (0, 1, 2):
        for keys in LISTS:
            nk = 11 if keys is None else len(keys)
            logits = coded(pu.special_rows(rng, n, nk), dtype)
            given = rng.randint(-1, nk + 1, n).astype(np.int32)
            seed, draw = int(rng.randint(1 << 30)) * 4099 + 1, int(rng.randint(1 << 30)) * 65537
            for o in (dict(mode=SAMPLE), dict(mode=GREEDY), dict(mode=GIVEN), dict(mode=SAMPLE, epsilon=0.2, beta=0.3), dict(mode=SAMPLE, inv_temp=0.37)):
                kw = dict(o, seed=seed, draw=draw)
                got = device(hd, logits, dtype, keys, teacher, given, **kw)
                exp = twin(hd, states, logits, dtype, keys, teacher, given, **kw)
                assert_same(got, exp, "%s dtype %d, %d keys, %s" % (where, dtype, nk, o))
                if o.get("beta"):
                    sources += np.bincount(got["source"], minlength=4)[:4]
    return states, sources


def test_kernel_equals_the_host_twin_mini(goldens):
    """200 mini envs (three full waves and a partial one) with enemies, auto-reset, after 0, 30 and 60 random steps."""
    torch_mod()
    cfg = dict(goldens["configs"]["mini"], enemies=mu.ENEMIES)
    hip = HipBatch(cfg, [300 + i for i in range(200)], max_steps=40, auto_reset=True)
    table = mu.key_table(5, 60, 200)
    total = np.zeros(4, np.int64)
    for t in (0, 30, 60):
        _, src = sweep(hip.h, "mini t=%d" % t, 10 + t)
        total += src
        for keys in table[t:t + 30]:
            hip.step(keys)
    hip.sync()
    print("sources under epsilon 0.2, beta 0.3:", total.tolist())
    assert total[0] > 0 and total[1] > 0 and total[2] > 0     # the policy, the uniform draw and the teacher all chose


def test_kernel_equals_the_host_twin_on_edge_rows_and_boundary_words(goldens):
    """256 mini envs as they stand after reset.  policy_edge_rows.edge_batch as the logits of every dtype, mode and inverse temperature; then the committed boundary
    words (u or v exactly on a running sum or a bound), each at ITS env index with equal logits over a list of keys that are all legal there: the kernel answers
    what the twin answers, and at the word's env what rg_policy.h's comment says."""
    torch_mod()
    cfg = dict(goldens["configs"]["mini"], enemies=mu.ENEMIES)
    n = 256
    hip = HipBatch(cfg, [4000 + i for i in range(n)], max_steps=40, auto_reset=True)
    hd = hip.h
    states = states_of(hd)
    x32 = pe.edge_batch(n, 11, seed=7)[0]
    rng = np.random.RandomState(3)
    given = rng.randint(0, 11, n).astype(np.int32)
    teacher = np.frombuffer(KEYS, np.uint8)[rng.randint(0, 11, n)]
    for dtype in (0, 1, 2):
        logits = coded(x32, dtype)
        for inv_temp in pe.INV_TEMPS:
            for o in (dict(mode=SAMPLE), dict(mode=GREEDY), dict(mode=GIVEN), dict(mode=SAMPLE, epsilon=0.2, beta=0.3)):
                kw = dict(o, inv_temp=inv_temp, seed=11, draw=dtype)
                assert_same(device(hd, logits, dtype, None, teacher, given, **kw), twin(hd, states, logits, dtype, None, teacher, given, **kw), "edge rows dtype %d, %s" % (dtype, kw))
    legal = hd.action_mask()
    used = total = 0
    for (kind, value), words in pe.BOUNDARY_WORDS.items():
        for seed, env, draw in words:
            total += 1
            n_keys = pe.U_EXPECT[value][0] if kind == "u" else 4
            if legal[env].sum() < 4:
                continue
            used += 1
            keys = bytes(KEYS[k] for k in np.flatnonzero(legal[env])[:n_keys])
            zeros = np.zeros((n, n_keys), np.float32)
            cases = [(dict(), pe.U_EXPECT[value][1], 0)] if kind == "u" else [(dict(beta=b, epsilon=e), None, src) for b, e, src in pe.V_EXPECT[value]]
            for o, action, src in cases:
                t = np.full(n, keys[2], np.uint8) if o.get("beta") else None
                got = device(hd, zeros, 0, keys, t, **dict(o, seed=seed, draw=draw))
                assert_same(got, twin(hd, states, zeros, 0, keys, t, **dict(o, seed=seed, draw=draw)), "word %s %#x env %d draw %d %s" % (kind, value, env, draw, o))
                assert got["source"][env] == src and (action is None or got["action"][env] == action), (kind, hex(value), env, draw, o, got["action"][env], got["source"][env])
    print("%d of %d boundary words exercised" % (used, total))
    assert 2 * used >= total
    hip.sync()


def test_kernel_equals_the_host_twin_dead_envs(goldens):
    """Run c of the action-mask tests on a handle without auto-reset: envs die and stay dead (keys[0], action 0, logp 0, entropy 0, source 3)."""
    torch_mod()
    _, dead, _, table = mu.oracle_run(goldens, mu.RUN_C)
    cfg, seeds, _ = mu.run_config(goldens, mu.RUN_C)
    hip = HipBatch(cfg, seeds, max_steps=mu.RUN_C["max_steps"], auto_reset=False)
    for t in range(mu.RUN_C["T"]):
        hip.step(np.where(dead[t], np.uint8(ord(".")), table[t]))
    assert int(dead[-1].sum()) >= 30
    # (an env once dead was fed '.', which raises RG_FLAG_ERR_DEAD at every sync: expected here, so the calls below do not go through check)
    hd, L = hip.h, hip.h.L
    assert L.rg_sync(hd.h) != 0 and "Ignored input" in L.rg_last_error(hd.h).decode()
    flags = np.empty(hd.n, np.uint32)
    L.rg_fetch_states(hd.h, None, None, None, flags.ctypes.data)
    assert np.array_equal((flags & 2) != 0, dead[-1])
    states = []
    for e in range(hd.n):
        d, cells = hd.debug_state(e)
        states.append((cells, hd.height, hd.width, d.px, d.py, int(dead[-1][e])))
    torch, inner = torch_mod(), inner_mod()
    rng = np.random.RandomState(4)
    dev = "cuda:%d" % hd.device
    for dtype in (0, 2):
        for mode in (SAMPLE, GREEDY, GIVEN):
            logits = coded(pu.special_rows(rng, hd.n, 11), dtype)
            given = rng.randint(0, 11, hd.n).astype(np.int32)
            lg, g = to_device(torch, logits, dev, dtype), to_device(torch, given, dev)
            bufs = [torch.full((hd.n,), 0xAA, dtype=torch.uint8, device=dev), torch.full((hd.n,), -7, dtype=torch.int32, device=dev),
                    torch.full((hd.n,), 7.0, dtype=torch.float32, device=dev), torch.full((hd.n,), 7.0, dtype=torch.float32, device=dev),
                    torch.full((hd.n,), 0xAA, dtype=torch.uint8, device=dev)]
            torch.cuda.synchronize()
            opts = pu.opts_of(inner, mode=mode, seed=77, draw=dtype)
            assert L.rg_act(hd.h, None, 0, ptr(lg), dtype, C.byref(opts), None, ptr(g), *[ptr(b) for b in bufs], None) == 0, L.rg_last_error(hd.h).decode()
            L.rg_sync(hd.h)
            torch.cuda.synchronize()
            got = dict(zip(OUTS, [b.cpu().numpy() for b in bufs]))
            exp = twin(hd, states, logits, dtype, None, None, given, mode=mode, seed=77, draw=dtype)
            assert_same(got, exp, "dead envs dtype %d mode %d" % (dtype, mode))
            gone = dead[-1]
            assert (got["key"][gone] == KEYS[0]).all() and (got["action"][gone] == 0).all() and (got["source"][gone] == 3).all()
            assert (got["logp"][gone] == 0).all() and (got["entropy"][gone] == 0).all() and (got["source"][~gone] != 3).all()


def test_kernel_equals_the_host_twin_80x24():
    """65 envs of 80 x 24: one wave and one lane."""
    torch_mod()
    hip = HipBatch(mu.DEFAULT_SIZE, [9100 + i for i in range(65)], max_steps=1000, auto_reset=True)
    for keys in mu.key_table(3, 40, 65):
        hip.step(keys)
    sweep(hip.h, "80x24", 3)
    hip.sync()


def test_groups_and_mixed_sizes(goldens):
    """96 envs cycling mini / 80 x 24 / 48 x 20 (the action-mask tests' mixed case): every group reads its envs' rows of the caller's tensors and writes its
    results there (ext), and an env's draw is that of its index in the HANDLE -- the twin is called with it."""
    torch_mod()
    inner = inner_mod()
    mini = goldens["configs"]["mini"]
    enemies = {"enemies": list(range(10))}
    shapes = [dict(mini, enemies=enemies), {"width": 80, "height": 24, "enemies": enemies},
              {"width": 48, "height": 20, "dungeon": {"style": "rogue", "room_num_x": 3, "room_num_y": 2}, "enemies": enemies}]
    n = 96
    hd = inner._Handle([json.dumps(dict(shapes[i % 3], seed=6000 + i)) for i in range(n)], 60, auto_reset=True)
    assert hd.mixed_sizes
    for keys in mu.key_table(1, 25, n):
        hd.check(hd.L.rg_step(hd.h, np.ascontiguousarray(keys).ctypes.data, 0))
    states, _ = sweep(hd, "mixed", 8)
    # the mask of the same call is the action mask's, row by row in the caller's env order
    rng = np.random.RandomState(2)
    logits = pu.special_rows(rng, n, 11)
    got = device(hd, logits, 0, None, mask=True, seed=5, draw=6)
    assert np.array_equal(got["mask"], hd.action_mask().view(np.uint8))
    # the draw is the handle's env index's: two envs of one group with the same row of logits draw differently, each as the twin says with ITS index
    same = np.tile(np.linspace(-1, 1, 11).astype(np.float32), (n, 1))
    got = device(hd, same, 0, None, seed=1, draw=2)
    assert_same(got, twin(hd, states, same, 0, None, seed=1, draw=2), "mixed, one row for all")
    local = twin(hd, states, same, 0, None, env_ids=[e // 3 for e in range(n)], seed=1, draw=2)   # (the index inside the env's own group)
    assert (got["action"] != local["action"]).any()
    hd.close()


def test_mask_output_and_the_env_tensor(goldens):
    torch = torch_mod()
    from rogue_gym.envs.device import HipVecRogueEnv
    n = 200
    cfgs = [dict(goldens["configs"]["mini"], enemies=mu.ENEMIES, seed=500 + i) for i in range(n)]
    env = HipVecRogueEnv(cfgs, max_steps=60, action_mask=True)
    for keys in mu.key_table(6, 20, n):
        env.step_keys(torch.as_tensor(keys).to(env.device))
    hd = env._h
    rng = np.random.RandomState(1)
    for keys in LISTS:
        nk = 11 if keys is None else len(keys)
        got = device(hd, pu.special_rows(rng, n, nk), 0, keys, mask=True, seed=3)
        assert np.array_equal(got["mask"], hd.action_mask(keys).view(np.uint8)), nk
        assert all(got["mask"][e, got["action"][e]] for e in range(n))
    # env.act rewrites env.action_mask with keys=None, and only then
    want = env.legal_mask().clone()
    logits = torch.randn((n, 11), device=env.device)
    env._mask_u8.fill_(0xAA)
    env.act(logits, keys=b".hjklnbuy>s")
    assert bool((env._mask_u8 == 0xAA).all())
    res = env.act(logits)
    assert torch.equal(env.action_mask, want)
    assert bool(env.action_mask.gather(1, res.actions.long()[:, None]).all())
    env.check_errors()
    env.close()


@pytest.mark.parametrize("persistent", [False, True])
def test_act_has_no_side_effects(goldens, persistent):
    """Twin envs on the same seeds and keys, one of which calls act() before every step (and throws the result away): the same observations, rewards and
    dones at every step, the same mirrors, flag words, status and state records of all envs at the end."""
    torch = torch_mod()
    from rogue_gym.envs import DungeonType, ImageSetting, StatusFlag
    from rogue_gym.envs.device import HipVecRogueEnv
    n, steps = 200, 30
    cfgs = [dict(goldens["configs"]["mini"], seed=800 + i) for i in range(n)]
    setting = ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, not persistent)
    table = torch.as_tensor(mu.key_table(7, steps, n))
    trace = []
    for acting in (False, True):
        env = HipVecRogueEnv(cfgs, max_steps=25, image_setting=setting, persistent_obs=persistent, guide="stairs")
        gen = torch.Generator(device=env.device).manual_seed(1)
        per_step = [env.obs.cpu().clone()]
        for t in range(steps):
            if acting:
                before = (env.save_state().clone(), env.obs.clone(), env.reward.clone(), env.done.clone())
                env.act(torch.randn((n, 11), generator=gen, device=env.device), epsilon=0.1, teacher=env.guide_keys, beta=0.2, seed=t)
                after = (env.save_state(), env.obs, env.reward, env.done)
                for x, y, what in zip(before, after, ("state records", "obs", "reward", "done")):
                    assert torch.equal(x, y), "t=%d: act changed %s" % (t, what)
            obs, reward, done = env.step_keys(table[t].to(env.device).contiguous())
            per_step.append((obs.cpu().clone(), reward.cpu().clone(), done.cpu().clone()))
        end = (env.screen.cpu().clone(), env.flags.cpu().clone(), env.status.cpu().clone(), env.save_state().cpu())
        env.check_errors()
        env.close()
        trace.append((per_step, end))
    (a_steps, a_end), (b_steps, b_end) = trace
    assert torch.equal(a_steps[0], b_steps[0])
    for t in range(1, steps + 1):
        for x, y, what in zip(a_steps[t], b_steps[t], ("obs", "reward", "done")):
            assert torch.equal(x, y), "t=%d %s differs" % (t, what)
    for x, y, what in zip(a_end, b_end, ("screen", "flags", "status", "state records")):
        assert torch.equal(x, y), what + " differs at the end"


def test_step_logits_counter_and_determinism(goldens):
    torch = torch_mod()
    from rogue_gym.envs.device import HipVecRogueEnv
    n = 70
    cfgs = [dict(goldens["configs"]["mini"], enemies=mu.ENEMIES, seed=40 + i) for i in range(n)]
    a, b = (HipVecRogueEnv(cfgs, max_steps=50, guide="explore") for _ in range(2))
    gen = torch.Generator(device=a.device).manual_seed(3)
    for t in range(12):
        logits = torch.randn((n, 11), generator=gen, device=a.device)
        if t % 2:
            logits = logits.to(torch.bfloat16)
        kw = dict(temperature=1.5, epsilon=0.1, teacher=None, beta=0.0, seed=9)
        assert a._draw == t == b._draw                                            # the env's own counter: one per call
        oa, ra, da, res = a.step_logits(logits, **kw)
        res_b = b.act(logits, **kw)
        for x, y in zip(res, res_b):
            assert torch.equal(x, y)
        assert res.keys.dtype == torch.uint8 and res.actions.dtype == torch.int32 and res.logp.dtype == torch.float32 and res.source.dtype == torch.uint8
        ob, rb, db = b.step_keys(res_b.keys)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), t
        assert torch.equal(a.guide_keys, b.guide_keys)
    # the same (seed, draw) on the same states: the same result; another draw: another one; an explicit draw leaves the counter alone
    logits = torch.randn((n, 11), generator=gen, device=a.device)
    r1, r2, r3 = a.act(logits, seed=4, draw=100), a.act(logits, seed=4, draw=100), a.act(logits, seed=4, draw=101)
    assert all(torch.equal(x, y) for x, y in zip(r1, r2)) and not torch.equal(r1.actions, r3.actions) and a._draw == 12
    # the DAgger form, and given= returns the stored log-probability again
    mixed = a.act(logits, teacher=a.guide_keys, beta=0.5, seed=4, draw=100)
    assert int((mixed.source == 2).sum()) > n // 5 and bool((mixed.keys[mixed.source == 2] == a.guide_keys[mixed.source == 2]).all())
    again = a.act(logits, given=mixed.actions)
    assert torch.equal(again.logp.view(torch.int32), mixed.logp.view(torch.int32)) and torch.equal(again.keys, mixed.keys) and torch.equal(again.entropy, mixed.entropy)
    # and logp is the masked log-softmax torch computes from action_mask
    ref = torch.log_softmax(logits.masked_fill(~a.legal_mask(), float("-inf")), dim=1).gather(1, mixed.actions.long()[:, None])[:, 0]
    assert float((ref - mixed.logp).abs().max()) < 1e-5
    with pytest.raises(ValueError, match="logits"):
        a.act(logits[:, :10])
    with pytest.raises(ValueError, match="logits"):
        a.act(logits.double())
    with pytest.raises(ValueError, match="temperature"):
        a.act(logits, temperature=0.0)
    with pytest.raises(RuntimeError, match="beta"):
        a.act(logits, beta=0.5)
    for env in (a, b):
        env.check_errors()
        env.close()


def test_the_oracle_plays_the_keys_act_chose(goldens):
    """64 mini envs with enemies for 100 steps: every key act chose is legal by the oracle-side mask, and with the oracle playing those keys the two
    engines stand in the same states at the end."""
    torch_mod()
    cfg = dict(goldens["configs"]["mini"], enemies=mu.ENEMIES)
    seeds = [7300 + i for i in range(64)]
    hip = HipBatch(cfg, seeds, max_steps=60, auto_reset=True)
    oracles = make_oracles(cfg, seeds, max_steps=60)
    rng = np.random.RandomState(6)
    moved = 0
    for t in range(100):
        logits = (rng.standard_normal((64, 11)) * 3).astype(np.float32)
        got = device(hip.h, logits, 0, None, mode=SAMPLE if t % 4 else GREEDY, epsilon=0.0 if t % 4 == 0 else 0.25, seed=1, draw=t)
        rows = np.stack([mu.oracle_row(o) for o in oracles])
        assert all(rows[e, got["action"][e]] for e in range(64)), "t=%d: an illegal key was chosen" % t
        assert np.array_equal(got["key"], np.frombuffer(KEYS, np.uint8)[got["action"]])
        moved += int(((got["action"] >= 1) & (got["action"] <= 8)).sum())
        hip.step(got["key"])
        mu.step_oracles(oracles, got["key"], True)
    hip.sync()
    compare_mirrors(hip, oracles, "end")
    compare_internal(hip, oracles, range(64), "end")
    assert moved > 2000      # (most legal keys are moves)


def test_refusals_launch_nothing(goldens):
    torch, inner = torch_mod(), inner_mod()
    hip = HipBatch(goldens["configs"]["mini"], [1 + i for i in range(70)], max_steps=60, auto_reset=True)
    hd, L = hip.h, hip.h.L
    dev = "cuda:%d" % hd.device
    n = 70
    logits = torch.zeros((n * 33 * 4 + 16,), dtype=torch.uint8, device=dev)
    outs = [torch.full((n * 4,), 0xAA, dtype=torch.uint8, device=dev) for _ in range(5)]
    mask = torch.full((n * 33 + 16,), 0xAA, dtype=torch.uint8, device=dev)
    teacher = torch.full((n,), ord("h"), dtype=torch.uint8, device=dev)
    given = torch.zeros((n,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    lp, mp = logits.data_ptr(), mask.data_ptr()
    assert lp % 16 == 0 and mp % 16 == 0
    ok = dict(keys=None, nk=0, logits=lp, dtype=0, teacher=None, given=None, key=True, mask=mp, null_opts=False)

    def call(o=None, **kw):
        a = dict(ok, **kw)
        opts = pu.opts_of(inner, **(o or {}))
        return L.rg_act(hd.h, a["keys"], a["nk"], None if a["logits"] is None else C.c_void_p(a["logits"]), a["dtype"], None if a["null_opts"] else C.byref(opts),
                        ptr(a["teacher"]), ptr(a["given"]), ptr(outs[0]) if a["key"] else None, ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), ptr(outs[4]),
                        None if a["mask"] is None else C.c_void_p(a["mask"]))

    cases = [(dict(keys=b"h", nk=0), None, ("n_keys", "got 0")), (dict(keys=b"h" * 33, nk=33), None, ("n_keys", "33")), (dict(keys=b"hjxk", nk=4), None, ("keys[2]", "0x78")),
             (dict(dtype=3), None, ("dtype", "got 3")), (dict(), dict(mode=3), ("mode", "got 3")), (dict(null_opts=True), None, ("opts",)),
             (dict(logits=lp + 4), None, ("logits_dev", "16-byte")), (dict(logits=None), None, ("logits_dev",)), (dict(mask=mp + 8), None, ("mask_dev", "16-byte")),
             (dict(), dict(inv_temp=0.0), ("inv_temp",)), (dict(), dict(inv_temp=float("inf")), ("inv_temp",)), (dict(), dict(inv_temp=float("nan")), ("inv_temp",)),
             (dict(), dict(inv_temp=-2.0), ("inv_temp",)), (dict(), dict(epsilon=1.5), ("epsilon",)), (dict(), dict(epsilon=-0.1), ("epsilon",)),
             (dict(teacher=teacher), dict(beta=1.5), ("beta",)), (dict(teacher=teacher), dict(beta=0.6, epsilon=0.6), ("epsilon + opts.beta",)),
             (dict(), dict(beta=0.5), ("beta", "teacher_dev")), (dict(), dict(mode=GIVEN), ("RG_ACT_GIVEN", "given_dev")), (dict(key=False), None, ("key_dev", "draws")),
             (dict(key=False), dict(mode=GREEDY), ("key_dev", "draws"))]
    for kw, o, words in cases:
        rc = call(o, **kw)
        msg = L.rg_last_error(hd.h).decode()
        assert rc != 0 and msg.startswith("rg_act:") and all(w in msg for w in words), (kw, o, msg)
        hip.sync()
        assert all(bool((t == 0xAA).all()) for t in outs) and bool((mask == 0xAA).all()), "a refused call wrote: " + msg
    # and the same buffers are written by a call that is not refused: exactly n of each, nothing behind them
    assert call(dict(mode=GIVEN), given=given, key=False) == 0      # (key_dev may be NULL where nothing is drawn)
    hip.sync()
    assert bool((outs[0] == 0xAA).all()) and bool((outs[1][:4 * n] == 0).all())
    assert call(dict(epsilon=0.5, beta=0.5), teacher=teacher) == 0
    hip.sync()
    assert bool((outs[0][:n] != 0xAA).all()) and bool((outs[0][n:] == 0xAA).all()) and bool((outs[4][:n] <= 2).all()) and bool((outs[4][n:] == 0xAA).all())
    assert bool((mask[:n * 11] <= 1).all()) and bool((mask[n * 11:] == 0xAA).all())


def test_value_api(goldens):
    """RogueEnv.act and ParallelRogueEnv.act (rg_act_host on the fetched grids) equal the device call on the same states."""
    torch_mod()
    from rogue_gym.envs import ParallelRogueEnv, RogueEnv
    cfg = dict(goldens["configs"]["mini"], enemies=mu.ENEMIES)
    rng = np.random.RandomState(12)
    penv = ParallelRogueEnv([dict(cfg, seed=40 + i) for i in range(8)], max_steps=30)
    for t in range(10):
        logits = (rng.standard_normal((8, 11)) * 2).astype(np.float32)
        teacher = np.frombuffer(KEYS, np.uint8)[rng.randint(0, 11, 8)]
        res = penv.act(logits, epsilon=0.2, teacher=teacher, beta=0.3, seed=3, draw=t, temperature=2.0)
        got = device(penv.game._h, logits, 0, None, teacher, inv_temp=0.5, epsilon=0.2, beta=0.3, seed=3, draw=t)
        assert_same(got, dict(zip(OUTS, res)), "ParallelRogueEnv t=%d" % t)
        masks = penv.action_masks()
        assert all(masks[e, res.actions[e]] for e in range(8))
        half = penv.act(logits.astype(np.float16), greedy=True)
        assert np.array_equal(half.actions, device(penv.game._h, logits.astype(np.float16), 1, None, mode=GREEDY)["action"])
        penv.step([int(a) for a in res.actions])
    penv.close()
    env = RogueEnv(config_dict=cfg, max_steps=1000, seed=21)
    for t in range(10):
        logits = (rng.standard_normal(11) * 2).astype(np.float32)
        res = env.act(logits, seed=8, draw=t)
        got = device(env.game._h, logits[None], 0, None, seed=8, draw=t)
        assert_same(got, dict(zip(OUTS, res)), "RogueEnv t=%d" % t)
        assert env.action_mask()[res.actions[0]]
        giv = env.act(logits, given=int(res.actions[0]), teacher="h")
        assert giv.logp.view(np.uint32)[0] == res.logp.view(np.uint32)[0] and giv.keys[0] == res.keys[0]
        env.step(int(res.actions[0]))
