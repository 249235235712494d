from .parallel import ParallelRogueEnv
from .rogue_env import DungeonType, ImageSetting, PlayerState, RogueEnv, StatusFlag
from .wrappers import FirstFloorEnv, StairRewardEnv, StairRewardParallel
from .device import MONSTER_COLS, OBJECT_COLS, HipVecFirstFloor, HipVecRogueEnv, HipVecStairReward, Tileset

__all__ = ["ParallelRogueEnv", "DungeonType", "ImageSetting", "PlayerState", "RogueEnv", "StatusFlag", "FirstFloorEnv", "StairRewardEnv",
           "StairRewardParallel", "HipVecRogueEnv", "HipVecStairReward", "HipVecFirstFloor", "MONSTER_COLS", "OBJECT_COLS", "Tileset"]
