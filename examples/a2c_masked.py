"""A2C with masked actions, both halves of the policy loop on the device: `env.act` chooses the keys and records the behaviour log-probability, and
`rogue_gym.masked_logp` recomputes log pi and the entropy for the stored actions under the stored masks with a backward pass; `rogue_gym.gae` turns the stored
rewards, ends and values of the rollout into advantages and returns in one launch, a time-limit end bootstrapping where a death does not.

    python examples/a2c_masked.py [--updates 8]

256 mini envs, a linear policy and a linear value head on the one-hot 5 x 5 window of symbol ids around the player, rollouts of 16 steps.  An illustration
of the calls, not a tuned learner.  Needs the built library (`python -c "import __graft_entry__ as g; g.build()"`) and a GPU; there is no CPU fallback."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rogue-gym_amd"))

import torch

import rogue_gym
from rogue_gym.envs import DungeonType, HipVecRogueEnv, ImageSetting, StatusFlag

MINI = {"width": 32, "height": 16, "hide_dungeon": True, "dungeon": {"style": "rogue", "room_num_x": 2, "room_num_y": 2}, "enemies": {"enemies": []}}
N, T, GAMMA, LAMBDA, ENT_COEF, VALUE_COEF, SYMBOLS = 256, 16, 0.99, 0.95, 0.01, 0.5, 64

ap = argparse.ArgumentParser()
ap.add_argument("--updates", type=int, default=8)
updates = ap.parse_args().updates

env = HipVecRogueEnv([dict(MINI, seed=i) for i in range(N)], max_steps=200, image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), action_mask=True,
                     episodes=True)
window = env.add_crop(2, ImageSetting(DungeonType.SYMBOL, StatusFlag.EMPTY, False), symbol_ids=True)     # uint8 [N, 1, 5, 5], refreshed by every step
dev, n_keys = env.device, len(env.ACTIONS)
features = 25 * SYMBOLS


def encode(ids):
    return torch.nn.functional.one_hot(ids.reshape(N, 25).long().clamp_(max=SYMBOLS - 1), SYMBOLS).reshape(N, features).float()


policy, value = torch.nn.Linear(features, n_keys).to(dev), torch.nn.Linear(features, 1).to(dev)
torch.nn.init.zeros_(policy.weight)
optim = torch.optim.Adam(list(policy.parameters()) + list(value.parameters()), lr=3e-3)

env.reset()
for update in range(updates):
    obs_buf, mask_buf, act_buf, logp_buf, rew_buf, done_buf, limit_buf = [], [], [], [], [], [], []
    with torch.no_grad():
        for t in range(T):
            x = encode(window.obs)
            res = env.act(policy(x), seed=update * T + t)       # one launch: keys, action indices, behaviour logp, entropy
            obs_buf.append(x)
            mask_buf.append(env.action_mask.clone())              # the mask the action was drawn under: the learner needs this one, not the next step's
            act_buf.append(res.actions)
            logp_buf.append(res.logp)
            _, reward, done = env.step_keys(res.keys)
            rew_buf.append(reward.float().clone())
            done_buf.append(done.bool().clone())
            limit_buf.append(env.time_limit.clone())              # which of the ends were time limits: the episode ended, the state did not
        obs = torch.stack(obs_buf)
        # one launch for the whole [T, N] rollout; a time limit bootstraps from the step's own value (the rebuild has replaced the state it cut off)
        adv, returns = rogue_gym.gae(torch.stack(rew_buf), value(obs)[..., 0], torch.stack(done_buf), value(encode(window.obs))[:, 0], gamma=GAMMA, lam=LAMBDA,
                                     truncated=torch.stack(limit_buf))
    masks, actions, old_logp = torch.stack(mask_buf), torch.stack(act_buf), torch.stack(logp_buf)
    # the learner's half: T x N rows in one launch forward and one backward
    logits = policy(obs)                                          # [T, N, n_keys]
    logp, entropy = rogue_gym.masked_logp(logits, actions, masks)
    values = value(obs)[..., 0]
    loss = -(logp * adv).mean() - ENT_COEF * entropy.mean() + VALUE_COEF * (returns - values).pow(2).mean()
    optim.zero_grad()
    loss.backward()
    optim.step()
    ratio = torch.exp(logp.detach() - old_logp)                   # unchanged weights since the rollout: 1 (exactly, where the two matmuls gave equal logits)
    print("update %d: loss %.4f, mean reward per step %.4f, entropy %.3f, illegal keys masked %.0f %%, ratio in [%.6f, %.6f]" % (
        update, float(loss.detach()), float(torch.stack(rew_buf).mean()), float(entropy.detach().mean()), 100.0 * float((~masks).float().mean()), float(ratio.min()), float(ratio.max())))
env.check_errors()
env.close()
