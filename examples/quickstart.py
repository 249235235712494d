"""Quick start: the three ways in, on one MI355X.

    python examples/quickstart.py

1. `RogueEnv`           -- the reference's gym.Env, one game (python/rogue_gym/envs/rogue_env.py): same constructor, same step() tuple.
2. `ParallelRogueEnv`   -- the reference's batched executor (parallel.py): N games, one kernel launch per key, value-object states.
3. `HipVecRogueEnv`     -- the tensor-native form: observations, rewards and dones stay in HBM as PyTorch-ROCm tensors (what bench.py measures).

Needs the built library (`python -c "import __graft_entry__ as g; g.build()"`) and a GPU; there is no CPU fallback."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rogue-gym_amd"))

import numpy as np
import torch

from rogue_gym.envs import DungeonType, HipVecRogueEnv, ImageSetting, ParallelRogueEnv, RogueEnv, StatusFlag

MINI = {"width": 32, "height": 16, "seed": 4, "hide_dungeon": True,
        "dungeon": {"style": "rogue", "room_num_x": 2, "room_num_y": 2}, "enemies": {"enemies": []}}  # the reference's data/config-mini.json

# 1. one game, the gym surface -------------------------------------------------------------------------------------------------------------
env = RogueEnv(config_dict=MINI, max_steps=50, image_setting=ImageSetting(DungeonType.SYMBOL, StatusFlag.DUNGEON_LEVEL | StatusFlag.HP_CURRENT))
state = env.reset()
total = 0.0
for key in "hjklyubn>s" * 3:
    state, reward, done, _ = env.step(key)          # a key of RogueEnv.ACTIONS or its index
    total += reward
    if done:
        state = env.reset()
print("RogueEnv: obs", env.image_setting.expand(state).shape, "gold so far", total)
print(env)                                           # the screen, like the reference's __repr__
print("RogueEnv.action_mask: keys that would do something now:", "".join(k for k, ok in zip(env.ACTIONS, env.action_mask()) if ok))

# 2. many games, value objects -------------------------------------------------------------------------------------------------------------
n = 1024
penv = ParallelRogueEnv([dict(MINI, seed=i) for i in range(n)], max_steps=100)
rng = np.random.RandomState(0)
states = penv.states
for _ in range(50):
    states, rewards, dones, _ = penv.step(rng.randint(0, penv.ACTION_LEN, n))   # terminal envs are reset inside step()
print("ParallelRogueEnv: %d envs, %d finished an episode in the last step, images %s" % (n, sum(dones), states.images(0, 0, False).shape))
penv.close()

# 3. tensors that never leave HBM -----------------------------------------------------------------------------------------------------------
n = 65536
venv = HipVecRogueEnv([dict(MINI, seed=i) for i in range(n)], max_steps=1000, image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), device=0)
actions = torch.randint(0, 11, (64, n), device=venv.device)
for t in range(100):
    obs, reward, done = venv.step(actions[t % 64])   # f32 [N, C, H, W], f32 [N], bool / u8 [N] -- device tensors, reused every step
torch.cuda.synchronize()
t0 = time.perf_counter()
for t in range(500):
    obs, reward, done = venv.step(actions[t % 64])
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print("HipVecRogueEnv: %d envs, obs %s on %s, %.0f M env-steps/s" % (n, tuple(obs.shape), obs.device, n * 500 / dt / 1e6))
venv.close()

# 3b. the same with the observation tensor BOUND to the stepper (opt-in): `obs` is kept current in place -- only the envs whose screen changed are rewritten;
#     contents identical, the caller must not write to it ----------------------------------------------------------------------------------------------
venv = HipVecRogueEnv([dict(MINI, seed=i) for i in range(n)], max_steps=1000, image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), device=0,
                      persistent_obs=True)
for t in range(100):
    obs, reward, done = venv.step(actions[t % 64])
torch.cuda.synchronize()
t0 = time.perf_counter()
for t in range(500):
    obs, reward, done = venv.step(actions[t % 64])
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print("HipVecRogueEnv(persistent_obs=True): %.0f M env-steps/s" % (n * 500 / dt / 1e6))
venv.close()

# 3c. the observation in the type the learner consumes: a bf16 image written by the encode pass itself (bit-identical to obs.to(torch.bfloat16)), and the
#     screen as uint8 symbol ids feeding an nn.Embedding-style lookup ---------------------------------------------------------------------------------
venv = HipVecRogueEnv([dict(MINI, seed=i) for i in range(4096)], image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), device=0, obs_dtype=torch.bfloat16)
obs, reward, done = venv.step(actions[0, :4096])
print("HipVecRogueEnv(obs_dtype=torch.bfloat16): obs %s %s" % (tuple(obs.shape), obs.dtype))
venv.close()
venv = HipVecRogueEnv([dict(MINI, seed=i) for i in range(4096)], image_setting=ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, False), device=0, symbol_ids=True)
obs, reward, done = venv.step(actions[0, :4096])
table = torch.randn(venv.symbols, 8, device=venv.device)
print("HipVecRogueEnv(symbol_ids=True): obs %s %s -> embedded %s" % (tuple(obs.shape), obs.dtype, tuple(table[obs[:, 0].long()].shape)))

# 3d. restart the lanes of your choice -- here the ones that reached level 2, from a mask that never leaves the device -- under any observation mode ----
obs = venv.reset_envs(mask=venv.status[:, 0] >= 2)
obs = venv.reset_envs(env_ids=[17, 4011], seeds=[7, 8])   # ... or by index, on seeds of your choice
print("HipVecRogueEnv.reset_envs: envs 17 and 4011 restarted on level %s" % venv.status[[17, 4011], 0].tolist())
venv.close()

# 3e. the full map plus an egocentric 11x11 window of symbol ids beside it (NLE's chars_crop: 121 bytes per env), both refreshed by every step ----------
venv = HipVecRogueEnv([dict(MINI, seed=i) for i in range(4096)], image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), device=0)
view = venv.add_crop(5, image_setting=ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, False), symbol_ids=True)
obs, reward, done = venv.step(actions[0, :4096])
print("HipVecRogueEnv.add_crop: obs %s %s beside a view %s %s centred on %s" % (tuple(obs.shape), obs.dtype, tuple(view.obs.shape), view.obs.dtype, view.center[0].tolist()))
venv.close()

# 3f. a masked random rollout: every env plays a key drawn among the keys that do something for it now (the engine's own move test, on the device:
#     no "can't move" turns), and `action_mask` is the bool [N, 11] tensor a masked policy would consume ------------------------------------------
venv = HipVecRogueEnv([dict(MINI, seed=i) for i in range(4096)], image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), device=0, action_mask=True)
gold = torch.zeros(4096, device=venv.device)
for t in range(200):
    obs, reward, done = venv.step_keys(venv.sample_keys())
    gold += reward
print("HipVecRogueEnv(action_mask=True): mask %s %s, %.1f legal keys per env, %.0f gold per env in 200 masked random steps"
      % (tuple(venv.action_mask.shape), venv.action_mask.dtype, venv.action_mask.sum(1).float().mean().item(), gold.mean().item()))
venv.close()

# 3g. a guided rollout: every env plays its teacher key -- one move closer to the stairs along the engine's own move graph, '>' on them, 's' (search) where
#     no path is known to the engine yet.  PRIVILEGED: the guide sees stairs, gold and passages the player has not discovered -- a scripted expert for
#     imitation data, or a shaping potential (guide_dist), not an observation -----------------------------------------------------------------------
venv = HipVecRogueEnv([dict(MINI, seed=i) for i in range(4096)], image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), device=0, guide="stairs")
start = venv.status[:, 0].clone()
for t in range(200):
    obs, reward, done = venv.step_keys(venv.guide_keys)
print("HipVecRogueEnv(guide='stairs'): keys %s %s, dist %s %s; dungeon level %.2f -> %.2f per env in 200 guided steps, %.1f moves to the stairs now"
      % (tuple(venv.guide_keys.shape), venv.guide_keys.dtype, tuple(venv.guide_dist.shape), venv.guide_dist.dtype, start.float().mean().item(),
         venv.status[:, 0].float().mean().item(), venv.guide_dist[venv.guide_dist >= 0].float().mean().item()))
venv.close()

# 3h. the same teacher through secrets, and an explorer that does not cheat: guide_secrets plans THROUGH hidden passages and locked doors and searches
#     beside them; guide="explore" plans on the player's own map only -- towards the stairs once they are on it, else towards the nearest known cell
#     beside an unknown one -- and is not privileged: a baseline agent, or realistic exploration trajectories for imitation ---------------------------
for kw in (dict(guide="stairs", guide_secrets=True), dict(guide="explore")):
    venv = HipVecRogueEnv([dict(MINI, seed=i) for i in range(4096)], image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), device=0, **kw)
    for t in range(200):
        obs, reward, done = venv.step_keys(venv.guide_keys)
    print("HipVecRogueEnv(%s): dungeon level %.2f per env after 200 steps, %.1f %% of the envs without a route now"
          % (", ".join("%s=%r" % kv for kv in kw.items()), venv.status[:, 0].float().mean().item(), 100 * (venv.guide_dist < 0).float().mean().item()))
    venv.close()

# 3h'. a policy network in the loop: a random linear "network" reads the gray image and step_logits() turns its [N, 11] logits into keys in one launch -- the
#      softmax over the keys that are legal now, a draw, the behaviour log-probability and the entropy for the rollout buffer (no autograd: the learner's update
#      recomputes log pi from action_mask).  Then the DAgger form: with probability beta the explorer's key is played, logp stays the policy's own ----------
venv = HipVecRogueEnv([dict(MINI, seed=i) for i in range(4096)], image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), device=0, action_mask=True, guide="explore")
net = torch.nn.Linear(venv.obs[0].numel(), len(venv.ACTIONS), device=venv.device)
with torch.no_grad():
    for beta in (0.0, 0.5):
        logp_sum = ent_sum = taught = 0.0
        for t in range(100):
            obs, reward, done, res = venv.step_logits(net(venv.obs.flatten(1)), temperature=1.0, epsilon=0.05, teacher=venv.guide_keys, beta=beta, seed=3)
            logp_sum, ent_sum, taught = logp_sum + res.logp.mean(), ent_sum + res.entropy.mean(), taught + (res.source == 2).float().mean()
        print("HipVecRogueEnv.step_logits(beta=%.1f): keys %s %s, mean behaviour logp %.2f, entropy %.2f nats, %.0f %% of the keys were the explorer's, dungeon level %.2f"
              % (beta, tuple(res.keys.shape), res.keys.dtype, float(logp_sum) / 100, float(ent_sum) / 100, float(taught), venv.status[:, 0].float().mean().item()))
venv.close()

# 3i. episode accounting and the scout reward on the device: what ended (died / time_limit), the finished episode's return and length, and one point per
#     map cell seen for the first time on a level -- no host trip until pop_episodes() ---------------------------------------------------------------
venv = HipVecRogueEnv([dict(MINI, seed=i) for i in range(4096)], max_steps=100, image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), device=0, scout=True, episode_log=8192, guide="explore")
total = sum(venv.step_keys(venv.guide_keys)[1].sum() + venv.scout.sum() for t in range(200))  # gold + scout as one reward
ep = venv.pop_episodes()
print("HipVecRogueEnv(scout=True): reward + scout %.0f over 200 explorer steps; %d episodes finished (%d died, %d time limits), mean return %.1f, length %.1f, scout %.1f"
      % (total.item(), len(ep["env"]), (ep["cause"] == 1).sum(), (ep["cause"] == 2).sum(), ep["ret"].mean(), ep["length"].mean(), ep["scout"].mean()))
venv.close()

# 3i'. count-based novelty on the device: a hash of what each env shows and how often it has shown it -- in its running episode (visit_count) and over every
#      env and episode (visit_count_global).  The bonus is one tensor op of the learner's: 1 / sqrt(count), or NovelD's / BeBold's `first visit` gate -----------
venv = HipVecRogueEnv([dict(MINI, seed=i) for i in range(4096)], max_steps=100, image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), device=0,
                      novelty="screen", novelty_scope="both", novelty_slots=256, novelty_global_slots=1 << 21, guide="explore")
bonus = gate = 0.0
for t in range(200):
    venv.step_keys(venv.guide_keys)
    bonus = bonus + venv.visit_count_global.float().rsqrt().sum()   # a lifetime count bonus
    gate = gate + (venv.visit_count == 1).sum()                      # the episodic first-visit gate
st = venv.novelty_stats()
print("HipVecRogueEnv(novelty='screen'): %.0f of %d explorer steps showed a screen for the first time in their episode; count bonus %.0f; %d distinct states, %d visits dropped"
      % (float(gate), 200 * 4096, float(bonus), st["occupied_global"], st["dropped_global"] + st["dropped_episode"]))
venv.close()

# 3j. the monsters as an entity table and four threat words, kept beside `obs`: what is next to me, where, which letter -- without parsing the image ----------
ENEMIES = dict(MINI, enemies={"enemies": list(range(12))})
venv = HipVecRogueEnv([dict(ENEMIES, seed=i) for i in range(4096)], max_steps=100, image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), device=0,
                      monsters="shown", monster_cap=4, action_mask=True)
for t in range(60):
    venv.step_keys(venv.sample_keys(seed=1))
e = int(venv.threat[:, 0].argmax())                      # an env with a monster next to the player
attackable = venv.threat[:, 2] & (venv.action_mask[:, 1:9].int() << torch.arange(8, device=venv.device)).sum(1)   # the positional mask ANDed with the legal moves
print("HipVecRogueEnv(monsters='shown'): %.1f %% of the envs have a monster next to the player, %.1f %% can attack one; env %d sees %s"
      % (100 * (venv.threat[:, 0] > 0).float().mean().item(), 100 * (attackable != 0).float().mean().item(), e,
         [dict(zip(venv.MONSTER_COLS[:5], (chr(r[0]),) + tuple(r[1:5]))) for r in venv.monsters[e].tolist() if r[0]]))
venv.close()

# 3k. the rest of the level as an object table ordered by WALKING distance, and an option rollout on it: every env picks a target -- its first gold row, else
#     its first stairs row, else its first row (the nearest frontier cell) -- hands the row's (y, x) to route() and plays the key.  objects="known" reads the
#     player's own map: nothing privileged ---------------------------------------------------------------------------------------------------------
venv = HipVecRogueEnv([dict(MINI, seed=i) for i in range(4096)], max_steps=1000, image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), device=0,
                      objects="known", object_kinds="stairs+gold+frontier", object_cap=8)
gold = torch.zeros(4096, device=venv.device)
lanes = torch.arange(4096, device=venv.device)
for t in range(200):
    kind = venv.objects[:, :, 0]
    is_gold, is_stairs = (kind & 2) != 0, (kind & 1) != 0
    pick = torch.where(is_gold.any(1), is_gold.int().argmax(1), torch.where(is_stairs.any(1), is_stairs.int().argmax(1), 0))
    row = venv.objects[lanes, pick].to(torch.int32)
    keys, dist, _ = venv.route(goal=None, known=True, cells=row[:, [5, 4]].contiguous())                            # columns 5, 4: (y, x); dist == row[:, 3]
    keys = torch.where(row[:, 3] == 0, torch.where((row[:, 0] & 1) != 0, ord(">"), ord("s")), keys.int()).to(torch.uint8)   # standing on it: descend, or search
    obs, reward, done = venv.step_keys(keys)
    gold += reward
e = int((venv.objects[:, :, 0] != 0).sum(1).argmax())
print("HipVecRogueEnv(objects='known'): %.0f gold per env in 200 option steps, dungeon level %.2f; counts (stairs, gold, door, frontier) of env %d: %s, its table %s"
      % (gold.mean().item(), venv.status[:, 0].float().mean().item(), e, venv.object_count[e].tolist(),
         [dict(zip(venv.OBJECT_COLS[:6], r[:6])) for r in venv.objects[e].tolist() if r[0]]))
venv.close()

# 3l. pixels: the player-centred 11 x 11 window drawn through the built-in 8 x 8 tileset, 88 x 88 gray, kept current beside `obs` (what a CNN agent reads after
#     `.float() / 255`), and a few rgb_array frames -- a mosaic of six envs per frame -- written as .npy for a video writer ---------------------------------
venv = HipVecRogueEnv([dict(MINI, seed=i) for i in range(256)], max_steps=1000, image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), device=0,
                      pixels="gray", pixel_crop=5)
frames = []
for t in range(40):
    venv.step_keys(venv.sample_keys(seed=2))
    if t % 10 == 9:
        frames.append(venv.frame(range(6), cols=3).cpu().numpy())        # uint8 [2 * 128, 3 * 256, 3]
np.save("rogue_frames.npy", np.stack(frames))
print("HipVecRogueEnv(pixels='gray', pixel_crop=5): pixels %s %s, %.1f %% of the pixels are ink (the paper's luminance is 17); wrote %d frames %s to rogue_frames.npy"
      % (tuple(venv.pixels.shape), venv.pixels.dtype, 100 * (venv.pixels > 17).float().mean().item(), len(frames), frames[0].shape))
venv.close()
