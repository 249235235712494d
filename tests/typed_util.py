"""numpy yardsticks of the typed observation tests: f32 -> bf16 / f16 by round-to-nearest-even written out in integer arithmetic (bf16) or taken from
numpy's own binary16 (f16), and Symbol::from_tile as a table.  tests/test_obs_typed_abi.py pins the bf16 helper to torch.Tensor.to(torch.bfloat16) on
the CPU, so that the GPU tests compare the kernels with something that is not the kernels."""
import numpy as np

RG_OBS_F32, RG_OBS_F16, RG_OBS_BF16, RG_OBS_U8 = 0, 1, 2, 3


def bf16_bits(x):
    """uint16 bit patterns of the bfloat16 nearest to each f32 of x (ties to even; NaN stays NaN, infinities stay)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (u >> 16) | 0x40, r)
    return r.astype(np.uint16)


def f16_bits(x):
    """uint16 bit patterns of the IEEE binary16 nearest to each f32 of x (numpy's conversion: ties to even, overflow to infinity)."""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(x, np.float32).astype(np.float16).view(np.uint16)


def bits16(x, dtype):
    """x (f32) rounded to RG_OBS_F16 / RG_OBS_BF16, as uint16 bit patterns."""
    return f16_bits(x) if dtype == RG_OBS_F16 else bf16_bits(x)


# Symbol::from_tile (core/src/symbol.rs:17-40), written out: glyph byte -> symbol id, 255 = not a symbol
SYMBOL_OF_TILE = np.full(256, 255, np.uint8)
for _i, _g in enumerate(" @#."):
    SYMBOL_OF_TILE[ord(_g)] = _i
SYMBOL_OF_TILE[ord("-")] = SYMBOL_OF_TILE[ord("|")] = 4
for _i, _g in enumerate("%+^!?])/*:=,"):
    SYMBOL_OF_TILE[ord(_g)] = 5 + _i
for _i in range(26):
    SYMBOL_OF_TILE[ord("A") + _i] = 17 + _i


def symbol_ids(screen):
    """u8 ids of a screen of glyph bytes (any shape)."""
    return SYMBOL_OF_TILE[np.asarray(screen, np.uint8)]
