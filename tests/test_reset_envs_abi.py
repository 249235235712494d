"""The partial-reset entry points at the drop-in boundary (no GPU needed): declared in the header, exported by the built library, bound with a ctypes
signature, and present on the Python classes."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rg_reset_envs", "rg_reset_mask", "rg_seed_envs")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


def test_reset_entry_points_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "rogue_gym_hip.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(rg_t \*h, " % name, hdr, re.M), "%s is not declared in the header" % name
        assert hasattr(lib, name), "missing export %s" % name
        assert getattr(lib, name).argtypes is not None, "%s has no ctypes signature" % name
    assert len(lib.rg_reset_envs.argtypes) == 4 and len(lib.rg_reset_mask.argtypes) == 2 and len(lib.rg_seed_envs.argtypes) == 5


def test_python_surface():
    from rogue_gym.envs import HipVecFirstFloor, HipVecRogueEnv, HipVecStairReward

    assert callable(getattr(HipVecRogueEnv, "reset_envs"))
    assert issubclass(HipVecFirstFloor, HipVecStairReward)
