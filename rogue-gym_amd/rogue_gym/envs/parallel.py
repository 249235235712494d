"""`ParallelRogueEnv`: many Rogue games stepped in lock step by ONE batched kernel launch per key.

Same public surface as the reference's thread-per-env executor (/root/reference/python/rogue_gym/envs/parallel.py:19-77): `step` takes a
string of N keys or N action indices and returns (states, rewards, dones, infos); terminal envs are reset inside `step` and report the
post-reset state with `is_terminal` still true (python/src/thread_impls.rs:69-79); rewards are the clipped gold deltas.  The states come
back as a StateBatch -- a sequence of PlayerState backed by one pinned host snapshot -- and `images()` turns a whole batch into a
[N, C, H, W] array with one launch, so nothing in the per-step path is O(N) Python.
Saving and restoring game states is not offered here: use HipVecRogueEnv.save_state / load_state (or RogueEnv's).
"""
import json
from typing import Dict, Iterable, List, Tuple, Union

import numpy as np

from rogue_gym_python._rogue_gym import ParallelGameState, StateBatch, Tileset, VisitCounter

from ._gym_compat import Discrete
from .rogue_env import ImageSetting, RogueEnv

_KEY_OF_ACTION = np.frombuffer("".join(RogueEnv.ACTIONS).encode(), np.uint8)


class ParallelRogueEnv:
    metadata = RogueEnv.metadata
    SYMBOLS = RogueEnv.SYMBOLS
    ACTION_MEANINGS = RogueEnv.ACTION_MEANINGS
    ACTIONS = RogueEnv.ACTIONS
    ACTION_LEN = RogueEnv.ACTION_LEN

    def __init__(self, config_dicts: Iterable[dict], max_steps: int = 1000, image_setting: ImageSetting = ImageSetting()) -> None:
        configs = [json.dumps(d) for d in config_dicts]
        self.num_workers, self.max_steps, self.image_setting = len(configs), max_steps, image_setting
        self.game = ParallelGameState(max_steps, configs)
        height, width = self.game.screen_size()
        self.action_space = Discrete(self.ACTION_LEN)
        self.observation_space = image_setting.detect_space(height, width, self.game.symbols())
        self.states: StateBatch = self.game.states()
        self._infos = [{}] * self.num_workers
        self._visits, self._visit_key = None, None

    def get_key_to_action(self) -> Dict[str, str]:
        return self.ACTION_MEANINGS

    def get_configs(self) -> dict:
        return json.loads(self.game.dump_config())

    def _keys_of(self, action: Union[Iterable[int], str]) -> np.ndarray:
        """A string with one raw key per env, or one action index per env."""
        if isinstance(action, str) and len(action) == self.num_workers:
            return np.frombuffer(action.encode("latin-1"), np.uint8)
        idx = None
        try:
            idx = np.asarray(action if isinstance(action, np.ndarray) else list(action))
        except TypeError:
            pass
        if idx is None or idx.dtype.kind not in "iu" or (idx.size and (idx.max() >= self.ACTION_LEN or idx.min() < -self.ACTION_LEN)):
            raise ValueError("Invalid action: {}".format(action))
        return _KEY_OF_ACTION[idx]  # negative indices count from the end, like the list lookup they replace

    def step(self, action: Union[Iterable[int], str]) -> Tuple[StateBatch, List[float], List[bool], List[dict]]:
        before = self.states
        after = self.game.step(self._keys_of(action))
        m = min(len(before), len(after))
        gained = np.maximum(after.gold[:m].astype(np.int64) - before.gold[:m].astype(np.int64), 0)
        self.states = after
        if self._visits is not None and m == len(after):  # (a stepped prefix leaves the counts where they are)
            self._visits.visit(after.screen, after.dungeon_level, after.is_terminal)
        return after, gained.tolist(), after.is_terminal.tolist(), self._infos

    def images(self, states: StateBatch = None) -> np.ndarray:
        """[N, C, H, W] float32 image of every env under `image_setting` (default: the states of the last step)."""
        return self.image_setting.expand_batch(self.states if states is None else states)

    def render_frames(self, states: StateBatch = None, tileset=None):
        """RogueEnv.render("rgb_array") for the whole batch: uint8 [N, H*th, W*8, 3] (a list of per-env frames when the batch mixes screen sizes)."""
        ts = Tileset.default() if tileset is None else tileset
        screens = (self.states if states is None else states).screen
        frames = [np.ascontiguousarray(ts.render(scr, rgb=True).transpose(1, 2, 0)) for scr in screens]
        return frames if isinstance(screens, list) else np.stack(frames)

    def action_masks(self) -> np.ndarray:
        """bool [N, ACTION_LEN]: entry [i, a] says whether ACTIONS[a] would do anything for env i now (RogueEnv.action_mask for the whole batch)."""
        return self.game.action_masks()

    def act(self, logits, **opts):
        """ActResult(keys, actions, logp, entropy, source) of numpy arrays [N]: RogueEnv.act for the whole batch, logits [N, ACTION_LEN] float32 or float16,
        teacher uint8 [N] key bytes, given int32 [N] action indices.  `logp` is the behaviour log-probability for the rollout buffer; there is no autograd
        (rogue_gym.masked_logp_np is the learner's numpy form)."""
        return self.game.act(logits, **opts)

    def path_keys(self, goal: str = "stairs"):
        """(keys uint8 [N], dist int32 [N]): RogueEnv.path_key for the whole batch, as key bytes and distances with -1 for unreachable."""
        return self.game.path_keys(goal)

    def route_keys(self, goal: str = "stairs", fallback=None, secrets: bool = False, known: bool = False):
        """(keys uint8 [N], dist int32 [N], tier uint8 [N]): RogueEnv.route_key for the whole batch, as key bytes, distances with -1 for unreachable and
        tiers with 255 for neither."""
        return self.game.route_keys(goal, fallback, secrets, known)

    def monster_tables(self, mode: str = "shown", cap: int = 4):
        """(table int16 [N, cap, 8], threat int32 [N, 4]): RogueEnv.monsters for the whole batch; mode "all" is privileged."""
        return self.game.monster_tables(mode, cap)

    def object_tables(self, kinds: str = "stairs+gold+door", known: bool = False, secrets: bool = False, cap: int = 8):
        """(table int16 [N, cap, 8], count int32 [N, 4]): RogueEnv.objects for the whole batch; without known=True it is privileged."""
        return self.game.object_tables(kinds, known, secrets, cap)

    def visit_counts(self, what: str = "screen", crop=None) -> np.ndarray:
        """int32 [N]: RogueEnv.visit_count for the whole batch -- how often each env's running episode has shown the state it is in now.  The first call
        starts the counting (the present states are first visits); from then on every step() counts, an env whose step ended its episode starts a new
        one with the state of its new game, and reset() starts all anew.  Not for batches that mix screen sizes.  On device tensors:
        HipVecRogueEnv(novelty=...)."""
        if self._visits is None or self._visit_key != (what, crop):
            if isinstance(self.states.screen, list):
                raise ValueError("visit_counts: the envs of this batch differ in screen size")
            self._visits, self._visit_key = VisitCounter(self.num_workers, what, crop), (what, crop)
            self._visits.visit(self.states.screen, self.states.dungeon_level, True)
        return self._visits.counts.copy()

    def reset(self) -> StateBatch:
        batch = self.states = self.game.reset()
        if self._visits is not None:
            self._visits.visit(batch.screen, batch.dungeon_level, True)
        return batch

    def seed(self, seeds: List[int]) -> None:
        """One seed per env, used from the next reset on."""
        self.game.seed(seeds)

    def close(self) -> None:
        self.game.close()
