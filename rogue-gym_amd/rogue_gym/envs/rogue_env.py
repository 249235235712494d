"""Single-environment gym surface of the HIP stepper: `RogueEnv`, `ImageSetting`, `StatusFlag`, `DungeonType`.

The public names, constructor arguments, return shapes and numeric conventions are those of the reference package
(/root/reference/python/rogue_gym/envs/rogue_env.py; pinned by python/tests/*.py, re-expressed in tests/test_gpu_reference_suite.py),
so code written against `rogue_gym.envs` runs unchanged.  The implementation is this repository's own: every observation is produced by
librogue_gym_hip.so on the GPU (rogue_gym_python._rogue_gym), and image requests on states that came out of one batch are served by a
single whole-batch kernel launch (StateBatch.images) instead of one encode per state.
"""
import enum
import json
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from rogue_gym_python import _rogue_gym as rogue_gym_inner
from rogue_gym_python._rogue_gym import GameState, PlayerState, StateBatch, VisitCounter

from ._gym_compat import Box, Discrete, Env

# (kind, with_hist) -> PlayerState method; kind 0 = gray, 1 = symbol (python/src/lib.rs:162-205)
_IMAGE_METHODS = {
    (0, False): "gray_image", (0, True): "gray_image_with_hist",
    (1, False): "symbol_image", (1, True): "symbol_image_with_hist",
}


def _read_text(path: str) -> str:
    with open(path, "r") as fh:
        return fh.read()


def _write_text(path: str, text: str) -> None:
    with open(path, "w") as fh:
        fh.write(text)


def _require_state(obj) -> None:
    if not isinstance(obj, PlayerState):
        raise TypeError("Needs PlayerState, but {} was given".format(type(obj)))


class StatusFlag(enum.Flag):
    """Which entries of the player status become constant image planes / vector entries.  Bit b selects entry b of
    [dungeon_level, hp_current, hp_max, str_current, str_max, defense, player_level, exp, hunger] (StatusFlagInner, python/src/flags.rs:45-55)."""

    EMPTY = 0
    DUNGEON_LEVEL = 1 << 0
    HP_CURRENT = 1 << 1
    HP_MAX = 1 << 2
    STR_CURRENT = 1 << 3
    STR_MAX = 1 << 4
    DEFENSE = 1 << 5
    PLAYER_LEVEL = 1 << 6
    EXP = 1 << 7
    HUNGER = 1 << 8
    FULL = (1 << 9) - 1

    def count_one(self) -> int:
        return bin(self.value & 0x1FF).count("1")

    def _image_of(self, state: PlayerState, kind: int, with_hist: bool) -> np.ndarray:
        _require_state(state)
        return getattr(state, _IMAGE_METHODS[(kind, with_hist)])(flag=self.value)

    def symbol_image(self, state: PlayerState) -> np.ndarray:
        return self._image_of(state, 1, False)

    def symbol_image_with_hist(self, state: PlayerState) -> np.ndarray:
        return self._image_of(state, 1, True)

    def gray_image(self, state: PlayerState) -> np.ndarray:
        return self._image_of(state, 0, False)

    def gray_image_with_hist(self, state: PlayerState) -> np.ndarray:
        return self._image_of(state, 0, True)

    def status_vec(self, state: PlayerState) -> List[int]:
        _require_state(state)
        return state.status_vec(self.value)


class DungeonType(enum.Enum):
    GRAY = 1
    SYMBOL = 2


class ImageSetting(NamedTuple):
    """How a PlayerState becomes a [C, H, W] float image: the dungeon as one gray plane or as one-hot symbol planes, followed by one constant
    plane per selected status entry and optionally the visited-history plane."""

    dungeon: DungeonType = DungeonType.SYMBOL
    status: StatusFlag = StatusFlag.FULL
    includes_hist: bool = False

    @property
    def _kind(self) -> int:
        return 1 if self.dungeon == DungeonType.SYMBOL else 0

    def dim(self, channels: int) -> int:
        return (channels if self._kind else 1) + self.status.count_one() + int(bool(self.includes_hist))

    def detect_space(self, h: int, w: int, symbols: int) -> Box:
        return Box(low=0, high=1, shape=(self.dim(symbols), h, w), dtype=np.float32)

    def expand(self, state: PlayerState) -> np.ndarray:
        return self.status._image_of(state, self._kind, bool(self.includes_hist))

    def expand_batch(self, states: Union[StateBatch, Sequence[PlayerState]]) -> np.ndarray:
        """[n, C, H, W] for a whole batch of states: one kernel launch when `states` is the StateBatch a ParallelRogueEnv returned."""
        if isinstance(states, StateBatch):
            return states.images(self._kind, self.status.value, bool(self.includes_hist))
        return np.stack([self.expand(s) for s in states])


# Symbol order of core/src/symbol.rs:17-40 / tile.rs: 17 fixed glyphs, then the 26 monster letters
_FIXED_SYMBOLS = " @#.-%+^!?])/*:=,"
# (key, meaning) in action-index order.  The j / k labels are the reference's own (python/rogue_gym/envs/rogue_env.py:145-157); the keymap that
# actually runs is KeyMap::ai (input.rs:73-100), where j moves down and k moves up.
_ACTION_TABLE = (
    (".", "NO_OPERATION"), ("h", "MOVE_LEFT"), ("j", "MOVE_UP"), ("k", "MOVE_DOWN"), ("l", "MOVE_RIGHT"), ("n", "MOVE_RIGHTDOWN"),
    ("b", "MOVE_LEFTDOWN"), ("u", "MOVE_RIGHTUP"), ("y", "MOVE_LEFTUP"), (">", "DOWNSTAIR"), ("s", "SEARCH"),
)


class RogueEnv(Env):
    """One Rogue game (GameState: no auto-reset; after death every further action key raises)."""

    metadata = {"render.modes": ["human", "ascii", "rgb_array"]}
    SYMBOLS = list(_FIXED_SYMBOLS) + [chr(ord("A") + i) for i in range(26)]
    ACTION_MEANINGS = dict(_ACTION_TABLE)
    ACTIONS = [key for key, _ in _ACTION_TABLE]
    ACTION_LEN = len(ACTIONS)

    def __init__(self, config_path: Optional[str] = None, config_dict: Optional[dict] = None, max_steps: int = 1000,
                 image_setting: ImageSetting = ImageSetting(), **kwargs) -> None:
        Env.__init__(self)
        if config_path is not None and config_path != "":
            config_json = _read_text(config_path)
        else:  # keyword arguments are top-level GameConfig fields (seed=..., width=..., ...) laid over config_dict
            config_json = json.dumps({**(config_dict or {}), **kwargs})
        self.game = GameState(max_steps, config_json)
        self.max_steps, self.image_setting = max_steps, image_setting
        height, width = self.game.screen_size()
        self.action_space = Discrete(self.ACTION_LEN)
        self.observation_space = image_setting.detect_space(height, width, self.game.symbols())
        self.result: PlayerState = self.game.prev()

    # ---- queries ----
    def screen_size(self) -> Tuple[int, int]:
        """(height, width)"""
        return self.game.screen_size()

    def get_key_to_action(self) -> Dict[str, str]:
        return self.ACTION_MEANINGS

    def get_dungeon(self) -> List[str]:
        """The screen as `height` strings of `width` characters."""
        return list(self.result.dungeon)

    def get_config(self) -> dict:
        return json.loads(self.game.dump_config())

    def save_config(self, fname: str) -> None:
        _write_text(fname, self.game.dump_config())

    def save_actions(self, fname: str) -> None:
        """The keys of this episode as the reference's InputCode JSON (replayable by its devui / act2gif tools)."""
        _write_text(fname, self.game.dump_history())

    def state_to_image(self, state: PlayerState, setting: Optional[ImageSetting] = None) -> np.ndarray:
        return (self.image_setting if setting is None else setting).expand(state)

    # ---- stepping ----
    def _keys_of(self, action: Union[int, str]) -> str:
        if isinstance(action, (str, bytes)):
            return action if isinstance(action, str) else action.decode("latin-1")
        try:
            return self.ACTIONS[action]
        except (IndexError, TypeError) as why:
            raise ValueError("Invalid action: {} causes {}".format(action, why)) from None

    def step(self, action: Union[int, str]) -> Tuple[PlayerState, float, bool, dict]:
        """`action` is an index into ACTIONS or a string of raw keys ("hjk", "hh>"): every key of the string is played and the reward is
        the gold collected over the whole string."""
        purse = self.result.gold
        for key in self._keys_of(action):
            self.game.react(ord(key))
        state = self.result = self.game.prev()
        self._visit(False)
        return state, state.gold - purse, state.is_terminal, {}

    def save_state(self) -> bytes:
        """The running game as a state record (bytes): everything of the episode, its action log included.  A record also loads into a
        HipVecRogueEnv of the same config (seed aside) and back."""
        return self.game.save_state()

    def load_state(self, state: bytes) -> PlayerState:
        """Put the game back into a saved state and return that state (also `self.result`).  PlayerState values handed out earlier keep
        what they were.  The seed stays this env's: the next reset builds from it."""
        self.game.load_state(state)
        state = self.result = self.game.prev()
        self._visit(True)
        return state

    def action_mask(self) -> np.ndarray:
        """bool [ACTION_LEN]: entry i says whether ACTIONS[i] would do anything now.  False = the game would answer the key with "can't move", with
        "no downstairs", or -- after death -- ignore it.  The rule is the engine's own move test (walls, hidden and locked cells, the corner-cutting rule
        for diagonals, the surface under the player for '>'), which the screen does not show completely."""
        return self.game.action_mask()

    def act(self, logits, **opts):
        """ActResult(keys, actions, logp, entropy, source) of numpy arrays of length 1: one masked categorical action from a row of policy logits
        [ACTION_LEN] (float32 or float16), by the rule HipVecRogueEnv.act runs on the device -- the softmax over the keys action_mask() calls legal, and
        bit for bit the device call's answer on the same state.  Options as there: greedy, temperature, epsilon, teacher (a key byte), beta, given (an
        action index), seed, draw (default 0: the caller counts), keys.  `logp` is the behaviour log-probability for the rollout buffer; there is no autograd
        (rogue_gym.masked_logp_np is the learner's numpy form: logp, entropy and a grad_fn for stored actions and masks)."""
        if opts.get("teacher") is not None:
            t = opts["teacher"]
            opts["teacher"] = [ord(t) if isinstance(t, (str, bytes)) else int(t)]
        if opts.get("given") is not None:
            opts["given"] = [int(opts["given"])]
        return self.game.act(logits, **opts)

    def path_key(self, goal: str = "stairs"):
        """(key, dist): the key of ACTIONS -- a str of length 1 -- that takes the player one move closer to the nearest goal cell ("stairs", "gold" or
        "stairs+gold") and the number of moves to it, or ('s', None) when none can be reached; '>' on the stairs.  Shortest paths under the engine's
        own move test.  PRIVILEGED: it sees stairs, gold and passages the player has not discovered -- a teacher, not an observation."""
        key, dist = self.game.path_key(goal)
        return key.decode("latin-1"), dist

    def route_key(self, goal: str = "stairs", fallback: Optional[str] = None, secrets: bool = False, known: bool = False):
        """(key, dist, tier): path_key with two switches and a fallback goal.  secrets=True plans THROUGH hidden and locked cells and answers 's' when the
        next cell of the route is one (Search works on the eight cells around the player).  known=True plans on the player's own map only -- the cells
        that are drawn or in view -- so nothing is privileged.  fallback ("stairs", "gold", "stairs+gold", or "frontier" with known=True: the known
        cells beside an unknown one) answers when `goal` cannot be reached; tier says which answered (0, 1, None = neither; dist is None then).
        route_key("stairs", "frontier", known=True) is a scripted explorer that sees what the player sees."""
        key, dist, tier = self.game.route_key(goal, fallback, secrets, known)
        return key.decode("latin-1"), dist, tier

    def monsters(self, mode: str = "shown", cap: int = 4):
        """(table, threat): the nearest `cap` (1 .. 16) monsters as an int16 array [cap, 8] -- columns tile, dx, dy, cheb, shown, active, hp, slot; a row
        whose tile is 0 is empty -- ordered by distance from the player, and the int32 threat words [4]: shown monsters next to the player, the distance of
        the nearest shown one (-1 = none), a bit per move key of ACTIONS[1:9] whose target cell holds a shown monster (AND it with action_mask() for
        legality), and the number of monsters that qualify.  mode "shown" lists what a redraw of the screen would show now.  mode "all" lists every
        living monster of the level with its hit points and is PRIVILEGED, as path_key is: a teacher or a shaping term, not an observation."""
        return self.game.monsters(mode, cap)

    def objects(self, kinds: str = "stairs+gold+door", known: bool = False, secrets: bool = False, cap: int = 8):
        """(table, count): the stairs, gold and doors of the level (kinds: names joined with '+'; "frontier" with known=True only) as an int16 array
        [cap, 8] -- columns kind (1 stairs | 2 gold | 4 door | 8 frontier), dx, dy, walk, x, y, cheb, 0; a row whose kind is 0 is empty -- ordered by
        walk, the number of moves it takes to reach the cell, and the int32 counts [4] of the cells of each kind, listed or not.  known=True reads the
        player's own map only; without it the answer is PRIVILEGED, as path_key is.  secrets=True walks through hidden and locked cells."""
        return self.game.objects(kinds, known, secrets, cap)

    def _visit(self, new_episode: bool) -> None:
        counter = getattr(self, "_visits", None)
        if counter is not None:
            counter.visit(self.result._map[None], [self.result.dungeon_level], new_episode)

    def visit_count(self, what: str = "screen", crop=None) -> int:
        """How often this episode has shown the state the game is in now, this time included: count-based novelty (the episodic count of RIDE, the
        `count == 1` gate of NovelD).  what: "screen" hashes the rows of the screen that show tiles, "pos" the player's cell, "crop" the window of
        crop = r or (ry, rx) around the player; the dungeon level is hashed in.  The first call starts the counting with the present state as a first
        visit (an env that never asks pays nothing); from then on every step() counts the state it ends in, and reset() and load_state() start a new
        episode of counts.  Another what or crop starts anew.  The hash is the rule of HipVecRogueEnv's device pass, on the host (rg_novelty_hash_host)."""
        counter = getattr(self, "_visits", None)
        if counter is None or self._visit_key != (what, crop):
            self._visits, self._visit_key = VisitCounter(1, what, crop), (what, crop)
            self._visit(True)
        return int(self._visits.counts[0])

    def seed(self, seed: int) -> None:
        """Takes effect at the next reset."""
        self.game.set_seed(seed)

    def reset(self) -> PlayerState:
        self.game.reset()
        state = self.result = self.game.prev()
        self._visit(True)
        return state

    def render(self, mode: str = "human", close: bool = False, tileset=None):
        """"human" / "ascii": prints the screen and the status line.  "rgb_array": returns the screen as a uint8 frame [H*th, W*8, 3] drawn through `tileset`
        (a Tileset; None = the built-in 8 x 8 one) -- the rule of rg_obs_pixels, on the CPU; the status line is not part of the frame."""
        if mode == "rgb_array":
            ts = rogue_gym_inner.Tileset.default() if tileset is None else tileset
            return np.ascontiguousarray(ts.render(self.result._map, rgb=True).transpose(1, 2, 0))
        print(repr(self.result))

    def replay(self, interval_ms: int = 100) -> None:
        """Needs the reference's terminal UI: raises (out of scope for the HIP stepper)."""
        rogue_gym_inner.replay(self.game, interval_ms=interval_ms)

    def play_cli(self) -> None:
        """Needs the reference's terminal UI: raises (out of scope for the HIP stepper)."""
        rogue_gym_inner.play_cli(game=self.game)

    def __repr__(self) -> str:
        return repr(self.result)

    @property
    def unwrapped(self):
        return self
