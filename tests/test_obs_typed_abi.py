"""The typed-observation entry points at the drop-in boundary (no GPU needed), and the yardstick of their GPU tests: tests/typed_util.py's
round-to-nearest-even against torch's own conversion on the CPU, for every f32 value the encoders can emit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import typed_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rg_obs_dtype_bytes", "rg_obs_typed", "rg_step_obs_typed")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


def test_typed_entry_points_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "rogue_gym_hip.h")).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, hdr, re.M), "%s is not declared in the header" % name
        assert hasattr(lib, name), "missing export %s" % name
        assert getattr(lib, name).argtypes is not None, "%s has no ctypes signature" % name
    for macro, val in (("RG_OBS_F32", 0), ("RG_OBS_F16", 1), ("RG_OBS_BF16", 2), ("RG_OBS_U8", 3)):
        assert re.search(r"^#define %s\s+%d\b" % (macro, val), hdr, re.M), macro
    assert (tu.RG_OBS_F32, tu.RG_OBS_F16, tu.RG_OBS_BF16, tu.RG_OBS_U8) == (0, 1, 2, 3)


def test_dtype_bytes_needs_no_device(lib):
    assert [lib.rg_obs_dtype_bytes(d) for d in (0, 1, 2, 3)] == [4, 2, 2, 1]
    for d in (4, -1, 255, 1 << 20):
        assert lib.rg_obs_dtype_bytes(d) == -1


def encoder_values():
    """Every f32 the encoders can emit: k / symbols by ONE f32 division (python/src/lib.rs:84), and status values -- i32 converted to f32: integers,
    sampled up to 2^24, every integer around the powers of two where a 16-bit mantissa's ties lie, and the binary16 overflow threshold."""
    k = np.arange(256, dtype=np.float32)
    gray = np.concatenate([k / np.float32(s) for s in range(2, 65)])
    rng = np.random.RandomState(0)
    ints = [np.arange(0, 70000), rng.randint(0, 1 << 24, 200000), np.array([65503, 65504, 65519, 65520, 65521, 65535, 65536, (1 << 24) - 1, 1 << 24])]
    for p in range(8, 17):  # the ties of bf16 (8 mantissa bits) and f16 (11) around 2^8 .. 2^16
        ints.append(np.arange((1 << p) - 600, (1 << p) + 600))
    ints = np.concatenate(ints).astype(np.int64)
    ints = np.concatenate([ints, -ints]).astype(np.int32).astype(np.float32)
    return np.concatenate([gray, ints, np.array([0.0, 1.0], np.float32)])


def test_numpy_rounding_helpers_agree_with_torch_on_the_cpu():
    torch = pytest.importorskip("torch")
    x = encoder_values()
    t = torch.from_numpy(x)
    exp_bf = t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(tu.bf16_bits(x), exp_bf), "bf16 helper differs from torch at %r" % x[np.nonzero(tu.bf16_bits(x) != exp_bf)[0][:5]]
    exp_h = t.to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(tu.f16_bits(x), exp_h), "f16 helper differs from torch at %r" % x[np.nonzero(tu.f16_bits(x) != exp_h)[0][:5]]
    assert np.array_equal(tu.bits16(x, tu.RG_OBS_BF16), exp_bf) and np.array_equal(tu.bits16(x, tu.RG_OBS_F16), exp_h)
    # (the constants the one-hot and history planes select between)
    assert tu.bf16_bits(np.float32(1))[()] == 0x3F80 and tu.f16_bits(np.float32(1))[()] == 0x3C00
    assert tu.f16_bits(np.float32(70000))[()] == 0x7C00  # overflow to infinity, as IEEE and torch


def test_symbol_table_is_symbol_from_tile():
    """core/src/symbol.rs:17-40, spot values and shape: 17 fixed glyphs, 'A'..'Z' -> 17..42, everything else no symbol."""
    ids = tu.symbol_ids(np.frombuffer(b" @#.-|%+^!?])/*:=,AZ", np.uint8))
    assert ids.tolist() == [0, 1, 2, 3, 4, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 42]
    assert int((tu.SYMBOL_OF_TILE != 255).sum()) == 18 + 26 and tu.SYMBOL_OF_TILE[ord("a")] == 255 and tu.SYMBOL_OF_TILE[0] == 255
