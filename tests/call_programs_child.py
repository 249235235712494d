"""Child process of tests/test_gpu_call_programs.py: one program in a process of its own, because the envs per step wave (ROGUE_GYM_HIP_EPW) are read once,
when the library first launches a step.

usage: call_programs_child.py PROFILE SEED"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rogue-gym_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from call_runner import run_program  # noqa: E402

if __name__ == "__main__":
    print("%s seed %s (ROGUE_GYM_HIP_EPW=%s): %s" % (sys.argv[1], sys.argv[2], os.environ.get("ROGUE_GYM_HIP_EPW"), run_program(sys.argv[1], int(sys.argv[2]))))
    print("OK")
