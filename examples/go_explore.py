"""Go-Explore's first phase on the device: remember the best way into every cell seen so far, return there, explore from there.

    python examples/go_explore.py [--envs 256] [--rounds 30] [--explore 40]

256 mini envs on ONE dungeon (one seed): the cell is the player's position and dungeon level (novelty="pos"), the score the gold in the pack, ties broken by the
shorter episode.  Every step offers each env's state to the cell archive behind the novelty pass (archive=cells: no host trip, no Python dict); every round
draws one occupied cell per env with Go-Explore's 1 / sqrt(seen + 1) weights (archive_sample: plain torch ops), restores the envs from the cells' state
records (archive_restore) and explores with masked random keys (sample_keys).  For keys of your own -- say the hash xor a per-seed salt, to keep the cells of
different dungeons apart -- and a shaped return as the score, pass archive_auto=False and call archive_update(keys, score) yourself.

Needs the built library (`python -c "import __graft_entry__ as g; g.build()"`) and a GPU; there is no CPU fallback."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rogue-gym_amd"))

import torch

from rogue_gym.envs import DungeonType, HipVecRogueEnv, ImageSetting, StatusFlag

MINI = {"width": 32, "height": 16, "seed": 4, "hide_dungeon": True,
        "dungeon": {"style": "rogue", "room_num_x": 2, "room_num_y": 2}, "enemies": {"enemies": []}}  # the reference's data/config-mini.json

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=256)
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--explore", type=int, default=40)
ap.add_argument("--cells", type=int, default=1 << 14)
a = ap.parse_args()

env = HipVecRogueEnv([dict(MINI) for _ in range(a.envs)], max_steps=10 * a.explore, image_setting=ImageSetting(DungeonType.GRAY, StatusFlag.EMPTY, False), device=0,
                     novelty="pos", archive=a.cells)
gen = torch.Generator(device=env.device).manual_seed(0)
deepest = 1
for r in range(a.rounds):
    for t in range(a.explore):                                    # explore: every step offers every env's state to its cell
        env.step_keys(env.sample_keys(seed=r))
        deepest = max(deepest, int(env.status[:, 0].max()))
    slots = env.archive_sample(a.envs, "seen", generator=gen)    # select: rarely seen cells first
    env.archive_restore(slots)                                    # return: no replay of actions, the state records are the way back
    if r % 5 == 4 or r == a.rounds - 1:
        st = env.archive_stats()
        occupied = env.archive.key != 0
        print("round %2d: %5d cells found, deepest level %d, best gold %d, %d records written, %d offers dropped"
              % (r + 1, st["occupied"], deepest, int(env.archive.score[occupied].max()), st["written"], st["dropped"]))
env.check_errors()
env.close()
