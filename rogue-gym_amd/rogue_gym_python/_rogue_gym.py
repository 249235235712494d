"""`rogue_gym_python._rogue_gym` -- host mirror of the reference's PyO3 module
(/root/reference/python/src/lib.rs:355-366) over the HIP C-ABI (include/rogue_gym_hip.h).

Same classes, method names, argument meaning and error behaviour as the Rust module:
GameState, ParallelGameState, PlayerState.  All game logic runs in librogue_gym_hip.so on an
MI355X; this file only marshals.  There is no CPU fallback: importing works anywhere, but
constructing a GameState without the built library or without a HIP device raises.
"""
import collections
import ctypes as C
import functools
import operator
import weakref
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("ROGUE_GYM_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "librogue_gym_hip.so")  # (override: A/B runs of two builds)

RG_FLAG_TERMINAL = 0x1
RG_FLAG_DEAD = 0x2
RG_FLAG_MSG_SHIFT = 8
RG_FLAG_MSG_MASK = 0x7F00
RG_FLAG_ERR_MASK = 0x00FF0000

STATUS_KEYS = ("dungeon_level", "gold", "hp_current", "hp_max", "str_current", "str_max", "defense", "player_level", "exp", "hunger")


class RgDebugState(C.Structure):
    _fields_ = [
        ("px", C.c_int32), ("py", C.c_int32), ("dungeon_level", C.c_int32), ("hp", C.c_int32), ("hp_max", C.c_int32),
        ("player_level", C.c_int32), ("n_monsters", C.c_int32), ("n_gold", C.c_int32),
        ("exp", C.c_uint32), ("food_left", C.c_uint32), ("quiet", C.c_uint32), ("pack_gold", C.c_uint32), ("steps", C.c_uint32),
        ("rng", C.c_uint32 * 12),
        ("mon_x", C.c_int32 * 384), ("mon_y", C.c_int32 * 384), ("mon_type", C.c_int32 * 384), ("mon_active", C.c_int32 * 384), ("mon_hp", C.c_int32 * 384),
        ("mon_exp", C.c_uint32 * 384),
        ("gold_x", C.c_int32 * 384), ("gold_y", C.c_int32 * 384), ("gold_amount", C.c_int32 * 384),
        ("n_rooms", C.c_int32), ("room_rect", C.c_uint32 * 384), ("room_meta", C.c_int32 * 384),
    ]


class RgEpisodeArrays(C.Structure):
    """rg_episode_arrays_t (include/rogue_gym_hip.h): device pointers."""
    _fields_ = [(k, C.c_void_p) for k in ("ret", "len", "depth", "died", "time_limit", "last_return", "last_length", "last_depth", "last_cause", "scout", "seen")] + [("seen_bytes", C.c_int32)]


class RgNoveltyArrays(C.Structure):
    """rg_novelty_arrays_t (include/rogue_gym_hip.h): device pointers."""
    _fields_ = [(k, C.c_void_p) for k in ("hash", "count", "gcount")]


class RgActOpts(C.Structure):
    """rg_act_opts (include/rogue_gym_hip.h)."""
    _fields_ = [("inv_temp", C.c_float), ("epsilon", C.c_float), ("beta", C.c_float), ("mode", C.c_uint32), ("seed", C.c_uint64), ("draw", C.c_uint64)]


class RgArchiveArrays(C.Structure):
    """rg_archive_arrays_t (include/rogue_gym_hip.h): device pointers."""
    _fields_ = [(k, C.c_void_p) for k in ("key", "score", "steps", "seen", "chosen", "when", "records", "slot", "stored", "score_in", "steps_in")]


RG_EP_STATS, RG_EP_SCOUT = 1, 2
RG_NOV_POS, RG_NOV_SCREEN, RG_NOV_CROP = 1, 2, 3
RG_NOV_EPISODE, RG_NOV_GLOBAL = 1, 2
NOVELTY_WHAT = {"pos": RG_NOV_POS, "screen": RG_NOV_SCREEN, "crop": RG_NOV_CROP}
NOVELTY_SCOPE = {"episode": RG_NOV_EPISODE, "global": RG_NOV_GLOBAL, "both": RG_NOV_EPISODE | RG_NOV_GLOBAL}
NOVELTY_STATS = ("occupied_global", "dropped_global", "dropped_episode", "calls")   # the words of rg_novelty_stats
ARCHIVE_STATS = ("occupied", "dropped", "written", "calls")                          # the words of rg_archive_stats
ARCHIVE_SLOT = [("key", "<u8"), ("score", "<i4"), ("steps", "<u4"), ("seen", "<u4"), ("chosen", "<u4"), ("when", "<u4"), ("zero", "<u4")]  # a slot of rg_archive_offer_host's table
RG_EP_DIED, RG_EP_TIME_LIMIT, RG_EP_CUT = 1, 2, 3
RG_MON_SHOWN, RG_MON_ALL, RG_MON_MAX_CAP, RG_MON_COLS = 0, 1, 16, 8
MONSTER_MODES = {"shown": RG_MON_SHOWN, "all": RG_MON_ALL}
MONSTER_COLS = ("tile", "dx", "dy", "cheb", "shown", "active", "hp", "slot")   # the int16 columns of a monster-table row (rg_monsters)
THREAT_COLS = ("adjacent", "nearest", "attack_mask", "count")                  # the int32 threat words
RG_OBJ_STAIRS, RG_OBJ_GOLD, RG_OBJ_DOOR, RG_OBJ_FRONTIER, RG_OBJ_MAX_CAP, RG_OBJ_COLS = 1, 2, 4, 8, 32, 8
OBJECT_KINDS = {"stairs": RG_OBJ_STAIRS, "gold": RG_OBJ_GOLD, "door": RG_OBJ_DOOR, "frontier": RG_OBJ_FRONTIER}   # joined with '+' in a kinds string
OBJECT_COLS = ("kind", "dx", "dy", "walk", "x", "y", "cheb", "zero")           # the int16 columns of an object-table row (rg_objects)
OBJECT_COUNT_COLS = ("stairs", "gold", "door", "frontier")                     # the int32 count words, one per kind bit
EPISODE_REC = [("serial", "<u4"), ("env", "<i4"), ("ret", "<f4"), ("length", "<i4"), ("depth", "<i4"), ("cause", "<u4"), ("scout", "<i4"), ("zero", "<u4")]  # rg_episode_rec

_lib = None

vp, i32, u32, u64, sz, i64 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_size_t, C.c_int64
_P = C.POINTER

# The C-ABI (include/rogue_gym_hip.h), every entry point once: name -> (argtypes, restype, may be absent).  In the two tables below a plain list is the
# argtypes of an entry point that returns int; a pair is (argtypes, restype) of one that does not.  tests/test_cabi_load.py holds them against the header.
_ABI = {}


def _abi(may_be_absent, table):
    for name, spec in table.items():
        argtypes, restype = spec if isinstance(spec, tuple) else (spec, C.c_int)
        _ABI[name] = (argtypes, restype, may_be_absent)


_abi(False, {
    "rg_create": [_P(C.c_char_p), i32, u64, i32, i32, _P(vp)],
    "rg_destroy": ([vp], None),
    "rg_last_error": ([vp], C.c_char_p),
    "rg_build_id": ([], C.c_char_p),
    "rg_dims": [vp] + [_P(i32)] * 4,
    "rg_env_symbols": [vp, vp], "rg_env_dims": [vp, vp, vp],
    "rg_set_stream": [vp, vp],
    "rg_seed": [vp, _P(u64), _P(u64), i32],
    "rg_reset": [vp],
    "rg_step": [vp, vp, i32],
    "rg_step_prefix": [vp, vp, i32, i32],
    "rg_step_obs_gray": [vp, vp, i32, u32, i32, vp],
    "rg_step_fetch": [vp, vp, i32, vp, vp, vp, vp],
    "rg_sync": [vp],
    "rg_screen": [vp, _P(vp)], "rg_hist": [vp, _P(vp)], "rg_status": [vp, _P(vp)], "rg_flags": [vp, _P(vp)],
    "rg_reward": [vp, _P(vp)], "rg_done": [vp, _P(vp)], "rg_set_stair_reward": [vp, C.c_float],
    "rg_obs_gray": [vp, u32, i32, vp], "rg_obs_symbol": [vp, u32, i32, vp], "rg_obs_channels": [vp, i32, u32, i32],
    "rg_fetch_states": [vp, vp, vp, vp, vp],
    "rg_encode_host": [i32, vp, vp, vp, i32, i32, i32, u32, i32, i32, vp],
    "rg_encode_host_batch": [i32, i32, vp, vp, vp, i32, i32, i32, u32, i32, i32, vp],
    "rg_obs_host": [vp, i32, u32, i32, vp],
    "rg_host_alloc": [sz, _P(vp)], "rg_host_free": ([vp], None),
    "rg_dev_alloc": [i32, sz, _P(vp)], "rg_dev_free": ([i32, vp], None), "rg_snapshot_take": [vp, vp], "rg_dev_read": [vp, vp, vp, sz], "rg_dev_read_rows": [vp, vp, sz, vp, sz, i32],
    "rg_compact_record_bytes": [vp, i32], "rg_pack_compact": [vp, i32, vp], "rg_expand_compact": [vp, vp, i32, i32, i32, u32, i32, vp],
    "rg_comm_unique_id": [vp], "rg_comm_init": [vp, vp, i32, i32], "rg_comm_destroy": [vp], "rg_comm_count": [vp, vp, vp], "rg_allgather_compact": [vp, i32, vp],
    "rg_status_vec": [vp, u32, vp],
    "rg_history_enable": [vp, i32], "rg_history_keys": [vp, i32, i32, vp, sz, _P(u32)],
    "rg_dump_history": [vp, i32, i32, C.c_char_p, sz, _P(sz)],
    "rg_counters": [vp, _P(u64), i32], "rg_counters_ex": [vp, _P(u64), i32, i32], "rg_probe_sclk": [vp, _P(C.c_double)],
    "rg_timing_enable": [vp, i32], "rg_timing_read": [vp, _P(C.c_double), _P(u64)],
    "rg_timing_read_all": [vp, i32, _P(C.c_double), _P(u64), _P(u64)],
    "rg_dump_config": [vp, i32, C.c_char_p, sz], "rg_config_canonical": [C.c_char_p, C.c_char_p, sz],
    "rg_config_resolved": [C.c_char_p, C.c_char_p, sz], "rg_config_schema": [C.c_char_p, sz, _P(sz)],
    "rg_debug_fetch": [vp, i32, _P(RgDebugState), vp], "rg_debug_descend": [vp],
})
# Entry points that a library named by ROGUE_GYM_HIP_LIB -- an older build in a same-box A/B run -- may lack; the product library exports every symbol of the header.
_abi(True, {
    "rg_timing_read_samples": [vp, i32, _P(C.c_float), i32, _P(i32)],
    "rg_obs_bind": [vp, i32, u32, i32, vp],
    "rg_state_record_bytes": [vp], "rg_state_save": [vp, vp, i32, i32, vp], "rg_state_load": [vp, vp, sz, vp, i32, i32],
    "rg_obs_crop": [vp, i32, i32, i32, u32, i32, vp, vp],
    "rg_obs_dtype_bytes": [i32], "rg_obs_typed": [vp, i32, i32, u32, i32, vp], "rg_step_obs_typed": [vp, vp, i32, i32, i32, u32, i32, vp],
    "rg_obs_crop_typed": [vp, i32, i32, i32, i32, u32, i32, vp, vp], "rg_step_obs_crop_typed": [vp, vp, i32, i32, i32, i32, i32, u32, i32, vp, vp],
    "rg_reset_envs": [vp, vp, i32, i32], "rg_reset_mask": [vp, vp], "rg_seed_envs": [vp, vp, _P(u64), _P(u64), i32],
    "rg_tail_encode": [vp, i32],
    "rg_action_mask": [vp, vp, i32, vp, vp, u64, u64], "rg_action_mask_host": [vp, i32, i32, i32, i32, i32, vp, i32, vp],
    "rg_sample_index": ([u64, u32, u64, u32], u32),
    "rg_act": [vp, vp, i32, vp, i32, _P(RgActOpts), vp, vp, vp, vp, vp, vp, vp, vp],
    "rg_act_host": [vp, i32, i32, i32, i32, i32, vp, i32, vp, i32, _P(RgActOpts), u32, i32, i32, vp, vp, vp, vp, vp],
    "rg_policy_eval": [vp, i64, i32, vp, i32, vp, vp, C.c_float, vp, vp], "rg_policy_grad": [vp, i64, i32, vp, i32, vp, vp, C.c_float, vp, vp, vp],
    "rg_policy_eval_host": [i64, i32, vp, i32, vp, vp, C.c_float, vp, vp], "rg_policy_grad_host": [i64, i32, vp, i32, vp, vp, C.c_float, vp, vp, vp],
    "rg_gae": [vp, i64, i64, vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp], "rg_gae_host": [i64, i64, vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp],
    "rg_vtrace": [vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp] + [C.c_float] * 5 + [vp, vp], "rg_vtrace_host": [i64, i64, vp, vp, vp, vp, vp, vp, vp, vp] + [C.c_float] * 5 + [vp, vp],
    "rg_path": [vp, u32, vp, vp, vp, vp], "rg_path_host": [vp, i32, i32, i32, i32, i32, u32, i32, i32, vp, vp, vp],
    "rg_route": [vp, u32, u32, u32, vp, vp, vp, vp], "rg_route_host": [vp, i32, i32, i32, i32, i32, u32, u32, u32, i32, i32, vp, vp, vp, vp],
    "rg_episode_enable": [vp, u32, i32], "rg_episode_update": [vp], "rg_episode_cut": [vp, vp, i32, i32, vp, i32], "rg_episode_arrays": [vp, _P(RgEpisodeArrays)],
    "rg_episode_log_read": [vp, vp, i32, _P(i32), _P(u64)], "rg_scout_host": [vp, i32, i32, vp, _P(i32)],
    "rg_novelty_enable": [vp, i32, u32, i32, i32, i32, i32], "rg_novelty_update": [vp], "rg_novelty_cut": [vp, vp, i32, i32, vp],
    "rg_novelty_arrays": [vp, _P(RgNoveltyArrays)], "rg_novelty_stats": [vp, _P(u64)], "rg_novelty_table_read": [vp, vp, vp, i32, _P(i32)],
    "rg_novelty_clear": [vp], "rg_novelty_hash_host": [i32, i32, i32, i32, vp, i32, i32, i32, i32, _P(u64)],
    "rg_novelty_finish_host": ([u64, u64], u64), "rg_novelty_insert_host": [vp, i32, u32, u64, _P(u32)],
    "rg_archive_enable": [vp, i32], "rg_archive_update": [vp, vp, vp, vp], "rg_archive_arrays": [vp, _P(RgArchiveArrays)],
    "rg_archive_restore": [vp, vp, vp, i32, i32], "rg_archive_stats": [vp, _P(u64)], "rg_archive_clear": [vp],
    "rg_archive_offer_host": [vp, i32, u64, C.c_int32, u32, u32, _P(C.c_int32), _P(C.c_int32)],
    "rg_monsters": [vp, u32, i32, vp, vp],
    "rg_monsters_host": [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, u32, i32, vp, vp],
    "rg_objects": [vp, u32, u32, i32, vp, vp], "rg_objects_host": [vp, i32, i32, i32, i32, i32, u32, u32, i32, vp, vp],
    "rg_tileset_default": [_P(i32), vp, vp], "rg_tileset_set": [vp, i32, vp, vp],
    "rg_obs_pixels": [vp, i32, vp], "rg_obs_pixels_crop": [vp, i32, i32, i32, vp, vp],
    "rg_step_obs_pixels": [vp, vp, i32, i32, vp], "rg_step_obs_pixels_crop": [vp, vp, i32, i32, i32, i32, vp, vp],
    "rg_pixels_host": [i32, vp, vp, i32, i32, i32, vp, i32, i32, i32, i32, vp],
})

_INT_FUNCS = tuple(name for name, (_, restype, _absent) in _ABI.items() if restype is C.c_int)


def load_library():
    """Load librogue_gym_hip.so (built in-tree by __graft_entry__.build() / csrc/build.sh)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise RuntimeError(
            "librogue_gym_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or rogue-gym_amd/csrc/build.sh -- there is no CPU fallback." % _SO
        )
    try:
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (same soname, libamdhip64.so.7).
        # Importing torch first makes the dynamic loader satisfy our NEEDED entry with that copy; loading ours
        # first would put two runtimes in the process and the second one sees no GPU.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(_SO)
    other_build = bool(os.environ.get("ROGUE_GYM_HIP_LIB"))
    for name, (argtypes, restype, may_be_absent) in _ABI.items():
        if may_be_absent and other_build and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.argtypes, fn.restype = argtypes, restype
    _lib = L
    return L


class Tileset:
    """A tileset of the pixel passes (rg_obs_pixels): `font` uint8 [256, th], a monochrome bitmap font of glyphs 8 pixels wide and th rows high (8 <= th <= 16;
    bit 7 of a row byte is the leftmost pixel), and `palette` uint8 [257, 3], the RGB ink of glyph byte g, entry 256 the paper.  Both may be given as numpy
    arrays or torch tensors and are kept as contiguous numpy arrays."""

    def __init__(self, font, palette):
        font, palette = (np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)) for t in (font, palette))
        if font.dtype != np.uint8 or font.ndim != 2 or font.shape[0] != 256 or not 8 <= font.shape[1] <= 16:
            raise ValueError("Tileset: font must be uint8 [256, th] with 8 <= th <= 16, got %s %s" % (font.dtype, font.shape))
        if palette.dtype != np.uint8 or palette.shape != (257, 3):
            raise ValueError("Tileset: palette must be uint8 [257, 3], got %s %s" % (palette.dtype, palette.shape))
        self.font, self.palette = font, palette

    @property
    def th(self):
        return int(self.font.shape[1])

    @classmethod
    def default(cls):
        """The built-in tileset (rg_tileset_default): an 8 x 8 font for 0x21 .. 0x7E and a palette on a dark paper."""
        L = load_library()
        th, font, pal = C.c_int(0), np.zeros(256 * 16, np.uint8), np.zeros((257, 3), np.uint8)
        if L.rg_tileset_default(C.byref(th), font.ctypes.data, pal.ctypes.data):
            raise RuntimeError("Error in rogue-gym: " + L.rg_last_error(None).decode())
        return cls(font[:256 * th.value].reshape(256, th.value).copy(), pal)

    def render(self, screen, rgb=True, center=None, crop=None):
        """The rule on the CPU (rg_pixels_host) for one screen uint8 [H, W]: uint8 [C, H*th, W*8], or with crop = (ry, rx) and center = (cy, cx) the window
        [C, (2ry+1)*th, (2rx+1)*8]."""
        L = load_library()
        screen = np.ascontiguousarray(screen, dtype=np.uint8)
        H, W = screen.shape
        ch = 3 if rgb else 1
        ry, rx = (-1, 0) if crop is None else crop
        cy, cx = (0, 0) if center is None else center
        out = np.zeros((ch, (H if crop is None else 2 * ry + 1) * self.th, (W if crop is None else 2 * rx + 1) * 8), np.uint8)
        if L.rg_pixels_host(self.th, self.font.ctypes.data, self.palette.ctypes.data, ch, H, W, screen.ctypes.data, int(cy), int(cx), int(ry), int(rx), out.ctypes.data):
            raise RuntimeError("Error in rogue-gym: " + L.rg_last_error(None).decode())
        return out


class VisitCounter:
    """Episodic visit counts for the value API (RogueEnv.visit_count, ParallelRogueEnv.visit_counts): the hash is the library's rule on the host
    (rg_novelty_hash_host, the twin of the device pass behind HipVecRogueEnv's visit_count), the memory a dict per env that a new episode empties.  what: "pos",
    "screen" or "crop" with crop = r or (ry, rx); for "pos" and "crop" the player's cell is where the screen shows '@'."""

    def __init__(self, n, what="screen", crop=None):
        if not isinstance(what, str) or what not in NOVELTY_WHAT:
            raise ValueError("what must be 'pos', 'screen' or 'crop', got %r" % (what,))
        if (what == "crop") != (crop is not None):
            raise ValueError("crop goes with what='crop' and only with it, got what=%r, crop=%r" % (what, crop))
        ry, rx = (0, 0) if crop is None else (crop, crop) if isinstance(crop, int) else crop
        self.what, self.radii, self.seen = NOVELTY_WHAT[what], (int(ry), int(rx)), [dict() for _ in range(n)]
        self.hashes, self.counts = np.zeros(n, np.uint64), np.zeros(n, np.int32)

    def visit(self, screens, levels, new_episode):
        """Count the states now standing in the envs: screens uint8 [n, H, W], levels [n]; new_episode [n] bool (or one bool for all): that env's memory is emptied first."""
        L = load_library()
        out = C.c_uint64(0)
        new_episode = np.broadcast_to(np.asarray(new_episode, bool), (len(self.seen),))
        for e, seen in enumerate(self.seen):
            scr = np.ascontiguousarray(screens[e], np.uint8)
            px = py = 0
            if self.what != RG_NOV_SCREEN:
                at = np.argwhere(scr == ord("@"))
                if len(at) != 1:
                    raise RuntimeError("Error in rogue-gym: the screen of env %d shows %d player glyphs" % (e, len(at)))
                py, px = int(at[0][0]), int(at[0][1])
            if L.rg_novelty_hash_host(self.what, int(levels[e]), scr.shape[0], scr.shape[1], scr.ctypes.data, px, py, self.radii[0], self.radii[1], C.byref(out)):
                raise RuntimeError("Error in rogue-gym: " + L.rg_last_error(None).decode())
            if new_episode[e]:
                seen.clear()
            k = int(out.value)
            seen[k] = seen.get(k, 0) + 1
            self.hashes[e], self.counts[e] = k, seen[k]
        return self.counts


def _default_device():
    return int(os.environ.get("ROGUE_GYM_HIP_DEVICE", os.environ.get("LOCAL_RANK", "0")))


class _Pool:
    """Buffers of one kind on loan, kept by size: take(nbytes) gives an address, give(address, nbytes) takes it back.  alloc(nbytes, byref) and free(pointer)
    are the library's pair for the kind.  The handle keeps two.  `pool`: page-locked host buffers for the per-step D2H copies of the value-object API -- a
    StateBatch borrows its buffers and hands them back when it is collected, so a stepping loop settles on two or three buffer sets and the copies run at full
    PCIe rate.  `dev_pool`: device buffers for the StateBatch snapshots."""

    def __init__(self, L, alloc, free):
        self.L, self.alloc, self.release, self.free, self.closed = L, alloc, free, {}, False

    def take(self, nbytes):
        lst = self.free.get(nbytes)
        if lst:
            return lst.pop()
        p = C.c_void_p()
        if self.alloc(nbytes, C.byref(p)):
            raise RuntimeError("Error in rogue-gym: " + self.L.rg_last_error(None).decode())
        return p.value

    def give(self, ptr, nbytes):
        if self.closed:
            self.release(C.c_void_p(ptr))
        else:
            self.free.setdefault(nbytes, []).append(ptr)

    def close(self):
        self.closed = True
        for lst in self.free.values():
            for ptr in lst:
                self.release(C.c_void_p(ptr))
        self.free = {}


class _Lease:
    """One pooled buffer on loan.  A pinned one goes back to the pool when the LAST array that views it is collected -- not when the StateBatch
    that asked for it is: `obs = env.images()` kept in a rollout buffer stays valid (and unchanged) for as long as the caller holds it, like the
    independent arrays the reference returns (python/src/lib.rs:78,95).  A device one is on loan to one StateBatch (its snapshot of the screen / history
    mirrors)."""
    __slots__ = ("pool", "ptr", "nbytes")

    def __init__(self, pool, nbytes):
        self.pool, self.nbytes = pool, nbytes
        self.ptr = pool.take(nbytes)

    def __del__(self):
        try:
            self.pool.give(self.ptr, self.nbytes)  # a closed pool frees it instead
        except Exception:
            pass


def _leased(pool, shape, dtype):
    """A numpy array over a freshly leased pinned buffer; every view / slice of it keeps the lease (numpy base -> ctypes array -> lease)."""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    lease = _Lease(pool, nbytes)
    raw = (C.c_uint8 * nbytes).from_address(lease.ptr)
    raw._lease = lease
    return np.frombuffer(raw, dtype=dtype).reshape(shape)


def _leased_many(pool, specs):
    """Several arrays over ONE leased pinned buffer (a lease costs a few microseconds of Python; a small batch's step has four): 16-byte aligned sections."""
    sizes = [(int(np.prod(sh)) * np.dtype(dt).itemsize + 15) & ~15 for sh, dt in specs]
    lease = _Lease(pool, sum(sizes))
    raw = (C.c_uint8 * sum(sizes)).from_address(lease.ptr)
    raw._lease = lease
    whole, out, off = np.frombuffer(raw, dtype=np.uint8), [], 0
    for (sh, dt), sz in zip(specs, sizes):
        out.append(whole[off:off + int(np.prod(sh)) * np.dtype(dt).itemsize].view(dt).reshape(sh))
        off += sz
    return out


N_ACTION_KEYS = 11  # RG_ACTION_KEYS


def _mask_keys(keys):
    """(pointer argument, n_keys) of a key list for rg_action_mask: None = the library's default list; bytes / str are passed on as they are (the
    library checks them)."""
    if keys is None:
        return None, N_ACTION_KEYS
    if isinstance(keys, str):
        keys = keys.encode("latin-1")
    if not isinstance(keys, (bytes, bytearray)):
        raise TypeError("keys must be bytes, str or None, got %s" % type(keys).__name__)
    return bytes(keys), len(keys)


RG_ACT_SAMPLE, RG_ACT_GREEDY, RG_ACT_GIVEN = 0, 1, 2
ACT_SOURCES = ("policy", "uniform", "teacher", "none")   # the values of an act result's `source`
ActResult = collections.namedtuple("ActResult", "keys actions logp entropy source")
ACT_DTYPES = {"float32": 0, "float16": 1, "bfloat16": 2}  # RG_OBS_F32 / RG_OBS_F16 / RG_OBS_BF16 by the name of the element type


def _act_opts(greedy=False, temperature=1.0, epsilon=0.0, beta=0.0, given=False, seed=0, draw=0):
    """The rg_act_opts of an act call.  The library checks the values (and names the one it refuses); temperature 0 is refused here, where it would divide."""
    temperature = float(temperature)
    if not temperature > 0.0:
        raise ValueError("temperature must be > 0, got %r (greedy=True takes the argmax)" % (temperature,))
    if greedy and given:
        raise ValueError("greedy=True and given= cannot be combined")
    mode = RG_ACT_GIVEN if given else RG_ACT_GREEDY if greedy else RG_ACT_SAMPLE
    inv = np.float32(1.0) / np.float32(temperature)
    return RgActOpts(float(inv), float(epsilon), float(beta), mode, int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFFFFFFFFFF)


PATH_GOALS = {"stairs": 1, "gold": 2, "stairs+gold": 3}  # RG_GOAL_STAIRS, RG_GOAL_GOLD; RG_GOAL_CELL (4) comes with a caller's cells


def _monster_args(mode, cap):
    """(RG_MON_* mode, cap) of rg_monsters for a mode name and a row count."""
    if not isinstance(mode, str) or mode not in MONSTER_MODES:
        raise ValueError("mode must be one of %s, got %r" % (", ".join(repr(m) for m in MONSTER_MODES), mode))
    try:
        cap = operator.index(cap)
    except TypeError:
        cap = -1
    if not 1 <= cap <= RG_MON_MAX_CAP:
        raise ValueError("cap must be an int in 1 .. %d, got %r" % (RG_MON_MAX_CAP, cap))
    return MONSTER_MODES[mode], cap


def _object_args(kinds="stairs+gold+door", known=False, secrets=False, cap=8):
    """(kinds, mode, cap) of rg_objects.  kinds: names of OBJECT_KINDS joined with '+' ("frontier" with known=True only); known / secrets: rg_route's mode
    bits; cap: the rows of the table, 1 .. RG_OBJ_MAX_CAP."""
    names = kinds.split("+") if isinstance(kinds, str) else [None]
    if any(k not in OBJECT_KINDS for k in names):
        raise ValueError("kinds must be names of %s joined with '+', got %r" % (", ".join(repr(k) for k in OBJECT_KINDS), kinds))
    word = 0
    for k in names:
        word |= OBJECT_KINDS[k]
    if (word & RG_OBJ_FRONTIER) and not known:
        raise ValueError("the kind 'frontier' needs known=True: the frontier is of the player's own map")
    try:
        cap = operator.index(cap)
    except TypeError:
        cap = -1
    if not 1 <= cap <= RG_OBJ_MAX_CAP:
        raise ValueError("cap must be an int in 1 .. %d, got %r" % (RG_OBJ_MAX_CAP, cap))
    return word, (ROUTE_SECRETS if secrets else 0) | (ROUTE_KNOWN if known else 0), cap


def _path_goals(goal, with_cells=False):
    """The goal bits of rg_path for a goal name (None = the caller's cells alone)."""
    if goal is None and with_cells:
        return 4
    if not isinstance(goal, str) or goal not in PATH_GOALS:
        raise ValueError("goal must be one of %s%s, got %r" % (", ".join(repr(g) for g in PATH_GOALS), " (or None with cells)" if with_cells else "", goal))
    return PATH_GOALS[goal] | (4 if with_cells else 0)


# rg_route: its goal names (RG_GOAL_*; "frontier" = RG_GOAL_FRONTIER, with known=True only), its mode bits, and the guide that is a route of its own
ROUTE_GOALS = {"stairs": 1, "gold": 2, "stairs+gold": 3, "frontier": 8}
ROUTE_SECRETS, ROUTE_KNOWN = 1, 2  # RG_ROUTE_*
ROUTE_NO_TIER = 255
# guide="explore": (goal, fallback, secrets, known).  known alone: with secrets it would read the LOCKED bit of a door that the player's map shows as a wall
EXPLORE = ("stairs", "frontier", False, True)


def _route_args(goal, fallback=None, secrets=False, known=False, with_cells=False):
    """(goals, fallback_goals, mode) of rg_route.  goal: a name of ROUTE_GOALS, or None with cells (the caller's cells alone); with cells RG_GOAL_CELL joins
    `goal`'s word, never the fallback's.  fallback: a name of ROUTE_GOALS or None."""
    def word(name, what):
        if not isinstance(name, str) or name not in ROUTE_GOALS:
            raise ValueError("%s must be one of %s, got %r" % (what, ", ".join(repr(g) for g in ROUTE_GOALS), name))
        return ROUTE_GOALS[name]
    goals = 4 if (goal is None and with_cells) else word(goal, "goal") | (4 if with_cells else 0)
    fb = 0 if fallback is None else word(fallback, "fallback")
    if ((goals | fb) & 8) and not known:
        raise ValueError("the goal 'frontier' needs known=True: the frontier is of the player's own map")
    return goals, fb, (ROUTE_SECRETS if secrets else 0) | (ROUTE_KNOWN if known else 0)


class _Handle:
    """Owns one rg_t."""

    def __init__(self, configs, max_steps, auto_reset, device=None):
        L = load_library()
        self.L = L
        self.device = _default_device() if device is None else device
        n = len(configs)
        arr = (C.c_char_p * n)()
        for i, cfg in enumerate(configs):
            arr[i] = None if cfg is None else cfg.encode("utf-8")
        h = C.c_void_p()
        rc = L.rg_create(arr, n, int(max_steps), self.device, int(auto_reset), C.byref(h))
        if rc:
            msg = L.rg_last_error(None).decode()
            if msg.startswith("Failed to parse config"):
                raise RuntimeError(msg)  # pyresult_with(.., "Failed to parse config") (python/src/lib.rs:219,275)
            raise RuntimeError("Error in rogue-gym: " + msg)
        self.h = h
        # ROGUE_GYM_HIP_NO_TAIL_ENCODE=1, read when the handle is created: rg_step_obs_gray runs the step and the full observation pass one after the other
        # (rg_tail_encode; the same bits -- A/B runs and the twin-handle tests)
        if os.environ.get("ROGUE_GYM_HIP_NO_TAIL_ENCODE", "0") not in ("", "0") and hasattr(L, "rg_tail_encode"):
            L.rg_tail_encode(h, 0)
        hh, ww, ss, nn = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        L.rg_dims(h, C.byref(hh), C.byref(ww), C.byref(ss), C.byref(nn))
        self.height, self.width, self.symbols, self.n = hh.value, ww.value, ss.value, nn.value
        self.env_symbols = np.empty(self.n, np.int32)  # per env: configs of one batch may differ (PlayerState.symbols is the env's own)
        L.rg_env_symbols(h, self.env_symbols.ctypes.data)
        self.uniform_symbols = bool((self.env_symbols == self.symbols).all())
        self.env_heights, self.env_widths = np.empty(self.n, np.int32), np.empty(self.n, np.int32)  # ... and in size (python/src/lib.rs:270-294)
        L.rg_env_dims(h, self.env_heights.ctypes.data, self.env_widths.ctypes.data)
        self.mixed_sizes = bool((self.env_heights != self.height).any() or (self.env_widths != self.width).any())
        self.pool = _Pool(L, L.rg_host_alloc, L.rg_host_free)
        self.dev_pool = _Pool(L, functools.partial(L.rg_dev_alloc, self.device), functools.partial(L.rg_dev_free, self.device))
        self.lazy = {}  # id -> weakref of the StateBatches whose screens still live only in their device snapshot (materialised before the handle goes)
        self.epoch = 0  # bumped by every call that changes the device-side states (a StateBatch remembers the epoch it was taken at)
        self.fast_step = True  # rg_step_fetch applies (cleared by the first refusal: a handle with config groups)
        self._scratch = (None, -1)  # the device scratch buffer of the host readers below (address, bytes; -1: none yet): kept between calls, grow-only, freed in close()

    def check(self, rc):
        if rc:
            raise RuntimeError("Error in rogue-gym: " + self.L.rg_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            for ref in list(self.lazy.values()):  # value semantics: states handed out earlier stay readable after close()
                b = ref()
                if b is not None:
                    b._materialise()
            if self._scratch[0]:
                self.L.rg_dev_free(self.device, C.c_void_p(self._scratch[0]))
                self._scratch = (None, -1)
            self.L.rg_destroy(self.h)
            self.h = None
            self.pool.close()
            self.dev_pool.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def fetch(self):
        """Fresh numpy copies of the mirrors (screen, hist, status, flags)."""
        n = self.n
        screen = np.empty((n, self.height, self.width), np.uint8)
        hist = np.empty((n, self.height, self.width), np.uint8)
        status = np.empty((n, 10), np.int32)
        flags = np.empty(n, np.uint32)
        self.check(self.L.rg_fetch_states(self.h, screen.ctypes.data, hist.ctypes.data, status.ctypes.data, flags.ctypes.data))
        return screen, hist, status, flags

    def snapshot(self):
        """The current states of all envs as one StateBatch (one D2H copy into pinned memory)."""
        return StateBatch(self)

    def step_keys_host(self, keys):
        """rg_step_prefix + rg_sync: the general form of a value-object step (config groups, mixed sizes); StateBatch(keys=...) uses rg_step_fetch where it applies."""
        self.check(self.L.rg_step_prefix(self.h, keys.ctypes.data, int(keys.shape[0]), 0))
        self.epoch += 1
        self.check(self.L.rg_sync(self.h))

    def states(self):
        return self.snapshot()

    def debug_state(self, env):
        out = RgDebugState()
        inside = 0 <= env < self.n  # (an env out of range is the library's to refuse)
        # the grid of the env's OWN size: in a mixed-size batch the handle's height and width are its first group's, and a larger env would write past them
        cells = np.empty((int(self.env_heights[env]), int(self.env_widths[env])) if inside else (self.height, self.width), np.uint16)
        self.check(self.L.rg_debug_fetch(self.h, env, C.byref(out), cells.ctypes.data))
        return out, cells

    def _scratch_grow(self, nbytes):
        """The address of the device scratch buffer, which holds at least nbytes afterwards (a larger one replaces it; it never shrinks)."""
        if self._scratch[1] < nbytes:
            if self._scratch[0]:
                self.L.rg_dev_free(self.device, C.c_void_p(self._scratch[0]))
                self._scratch = (None, -1)
            p = C.c_void_p()
            if self.L.rg_dev_alloc(self.device, nbytes, C.byref(p)):
                raise RuntimeError("Error in rogue-gym: " + self.L.rg_last_error(None).decode())
            self._scratch = (p.value, nbytes)
        return self._scratch[0]

    def _scratch_read(self, nbytes):
        """The first nbytes of the device scratch buffer as a numpy uint8 array of its own (one rg_dev_read)."""
        out = np.empty(nbytes, np.uint8)
        self.check(self.L.rg_dev_read(self.h, C.c_void_p(self._scratch[0]), out.ctypes.data, nbytes))
        return out

    def action_mask(self, keys=None):
        """bool [n, n_keys]: which of `keys` (bytes / str; None = RG_ACTION_KEYS, RogueEnv.ACTIONS in index order) would do anything for each env now
        (rg_action_mask into a device scratch buffer the handle keeps, one rg_dev_read)."""
        kb, nk = _mask_keys(keys)
        base = self._scratch_grow(self.n * nk)
        self.check(self.L.rg_action_mask(self.h, kb, nk, C.c_void_p(base), None, 0, 0))
        return self._scratch_read(self.n * nk).reshape(self.n, nk).view(np.bool_)

    def act(self, logits, greedy=False, temperature=1.0, epsilon=0.0, teacher=None, beta=0.0, given=None, seed=0, draw=0, keys=None):
        """The value form of rg_act: ActResult of numpy arrays [n] (keys u8, actions i32, logp f32, entropy f32, source u8) for `logits`, a numpy array
        [n, n_keys] of float32 or float16 -- through rg_act_host, the CPU twin of the device rule, env by env on the grids rg_debug_fetch hands out (bit for
        bit what the device call gives on the same states).  teacher: key bytes u8 [n]; given: action indices [n] (their log-probability, no draw)."""
        kb, nk = _mask_keys(keys)
        logits = np.ascontiguousarray(logits)
        if logits.dtype not in (np.float32, np.float16) or logits.shape != (self.n, nk):
            raise ValueError("act: logits must be a float32 / float16 array [%d, %d], got %s %s" % (self.n, nk, logits.shape, logits.dtype))
        teacher = None if teacher is None else np.ascontiguousarray(teacher, dtype=np.uint8).reshape(self.n)
        given = None if given is None else np.ascontiguousarray(given, dtype=np.int32).reshape(self.n)
        opts = _act_opts(greedy, temperature, epsilon, beta, given is not None, seed, draw)
        flags = np.empty(self.n, np.uint32)
        self.check(self.L.rg_fetch_states(self.h, None, None, None, flags.ctypes.data))
        out = ActResult(np.zeros(self.n, np.uint8), np.zeros(self.n, np.int32), np.zeros(self.n, np.float32), np.zeros(self.n, np.float32), np.zeros(self.n, np.uint8))
        dtype = ACT_DTYPES[logits.dtype.name]
        for e in range(self.n):
            d, cells = self.debug_state(e)
            h, w = int(self.env_heights[e]), int(self.env_widths[e])
            rc = self.L.rg_act_host(cells.ctypes.data, h, w, d.px, d.py, int(flags[e] >> 1) & 1, kb, nk, logits[e].ctypes.data, dtype, C.byref(opts), e,
                                    -1 if teacher is None else int(teacher[e]), 0 if given is None else int(given[e]),
                                    out.keys[e:].ctypes.data, out.actions[e:].ctypes.data, out.logp[e:].ctypes.data, out.entropy[e:].ctypes.data, out.source[e:].ctypes.data)
            if rc:
                raise RuntimeError("Error in rogue-gym: " + self.L.rg_last_error(None).decode())
        return out

    def path_keys(self, goal="stairs"):
        """(keys u8 [n], dist i32 [n]) towards `goal` ("stairs", "gold", "stairs+gold"): rg_path into the device scratch buffer the handle keeps, one
        rg_dev_read.  dist -1 = unreachable."""
        goals, n = _path_goals(goal), self.n
        base = self._scratch_grow(5 * n)  # dist i32 [n], then keys u8 [n]
        self.check(self.L.rg_path(self.h, goals, None, None, C.c_void_p(base), C.c_void_p(base + 4 * n)))
        out = self._scratch_read(5 * n)
        return out[4 * n:].copy(), out[:4 * n].view(np.int32).copy()

    def _tables(self, cap, cols, launch):
        """(table i16 [n, cap, cols], words i32 [n, 4]) of a table pass: launch(table address, words address) into the device scratch buffer, one rg_dev_read."""
        tb = self.n * cap * cols * 2
        base = self._scratch_grow(tb + self.n * 16)  # table i16 [n][cap][8], then the words i32 [n][4]: both on multiples of 16 bytes
        self.check(launch(C.c_void_p(base), C.c_void_p(base + tb)))
        out = self._scratch_read(tb + self.n * 16)
        return out[:tb].view(np.int16).reshape(self.n, cap, cols).copy(), out[tb:].view(np.int32).reshape(self.n, 4).copy()

    def monster_tables(self, mode="shown", cap=4):
        """(table i16 [n, cap, 8], threat i32 [n, 4]) of rg_monsters (_monster_args names the arguments): into the device scratch buffer the handle keeps,
        one rg_dev_read."""
        m, cap = _monster_args(mode, cap)
        return self._tables(cap, RG_MON_COLS, lambda table, threat: self.L.rg_monsters(self.h, m, cap, table, threat))

    def object_tables(self, kinds="stairs+gold+door", known=False, secrets=False, cap=8):
        """(table i16 [n, cap, 8], count i32 [n, 4]) of rg_objects (_object_args names the arguments): into the device scratch buffer the handle keeps,
        one rg_dev_read."""
        kw, mode, cap = _object_args(kinds, known, secrets, cap)
        return self._tables(cap, RG_OBJ_COLS, lambda table, count: self.L.rg_objects(self.h, kw, mode, cap, table, count))

    def route_keys(self, goal="stairs", fallback=None, secrets=False, known=False):
        """(keys u8 [n], dist i32 [n], tier u8 [n]) of rg_route (_route_args names the arguments): into the device scratch buffer the handle keeps, one
        rg_dev_read.  dist -1 = unreachable, tier 255 = neither tier reached the player."""
        (goals, fb, mode), n = _route_args(goal, fallback, secrets, known), self.n
        base = self._scratch_grow(6 * n)  # dist i32 [n], then keys u8 [n], then tier u8 [n]
        self.check(self.L.rg_route(self.h, goals, fb, mode, None, C.c_void_p(base), C.c_void_p(base + 4 * n), C.c_void_p(base + 5 * n)))
        out = self._scratch_read(6 * n)
        return out[4 * n:5 * n].copy(), out[:4 * n].view(np.int32).copy(), out[5 * n:].copy()

    def history_keys(self, env, previous=False):
        n = C.c_uint32()
        rc = self.L.rg_history_keys(self.h, env, int(previous), None, 0, C.byref(n))
        self.check(rc)
        buf = (C.c_uint8 * max(1, n.value))()
        self.check(self.L.rg_history_keys(self.h, env, int(previous), buf, len(buf), C.byref(n)))
        return bytes(buf[: n.value])

    def state_bytes(self):
        """R: bytes of one state record of this handle (rg_state_record_bytes)."""
        r = self.L.rg_state_record_bytes(self.h)
        if r < 0:
            self.check(1)
        return r

    def save_state_host(self, env=0):
        """env's state record as bytes (rg_state_save into a pooled device buffer, one synchronous D2H copy); errors as rg_sync."""
        r = self.state_bytes()
        ptr = self.dev_pool.take(r)
        try:
            ids = (C.c_int32 * 1)(int(env))
            self.check(self.L.rg_state_save(self.h, ids, 1, 0, C.c_void_p(ptr)))
            buf = (C.c_uint8 * r)()
            self.check(self.L.rg_dev_read(self.h, C.c_void_p(ptr), buf, r))
            self.check(self.L.rg_sync(self.h))
        finally:
            self.dev_pool.give(ptr, r)
        return bytes(buf)

    def load_state_host(self, record, env=0):
        """Restore env from a record made by save_state_host (or one row of HipVecRogueEnv.save_state); raises if it does not fit."""
        import torch

        data = bytes(record)
        if len(data) < 64 or len(data) % 16:
            raise ValueError("not a state record (%d bytes)" % len(data))
        dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(torch.device("cuda", self.device))
        torch.cuda.synchronize(dev.device)  # (the handle's stream is not torch's: the upload is complete before the load is enqueued)
        ids = (C.c_int32 * 1)(int(env))
        self.check(self.L.rg_state_load(self.h, C.c_void_p(dev.data_ptr()), len(data), ids, 1, 0))
        self.epoch += 1
        self.check(self.L.rg_sync(self.h))

    def dump_history(self, env, previous=False):
        need = C.c_size_t()
        self.check(self.L.rg_dump_history(self.h, env, int(previous), None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        self.check(self.L.rg_dump_history(self.h, env, int(previous), buf, need.value, None))
        return buf.value.decode()


_EAGER_MAX_BYTES = 1 << 16  # rg_step_fetch: batches of at most this many screen bytes get their screens written to pinned memory by the step itself
_LAZY_MIN_BYTES = 1 << 20   # batches with at least this many screen bytes keep their screens on the device until they are looked at
_LAZY_MAX_BYTES = 1 << 30   # device bytes all not-yet-read snapshots of a handle may pin together (65 536 mini envs: 8 batches); older ones move to the host
_IMAGE_BATCH_LIMIT = 1 << 28  # bytes: above this a batch does not cache whole-batch images (one-hot images of large batches are GBs)


class StateBatch:
    """What ParallelGameState::states/step/reset return (`Vec<PlayerState>`, python/src/lib.rs:308-328), kept as ONE snapshot of the batch
    instead of n Python objects: a read-only sequence whose items are PlayerState views, plus vector accessors (gold, dungeon_level,
    is_terminal) and whole-batch images computed by one kernel launch."""

    def __init__(self, handle, keys=None):
        """keys: step the batch with these keys first (ParallelGameState.step), through rg_step_fetch where it applies -- one call, one stream wait."""
        self._hd = handle
        n, h, w = handle.n, handle.height, handle.width
        self.n, self.symbols = n, handle.symbols
        # pinned, pooled buffers; each array owns its lease, so an array (or any slice of it) a caller keeps outlives this batch safely
        self.mixed_sizes = handle.mixed_sizes
        eager = keys is not None and handle.fast_step and not self.mixed_sizes and (h * w) % 4 == 0 and n * h * w <= _EAGER_MAX_BYTES
        if eager:  # (one lease for the four arrays of a small batch's step)
            self.status, self.flags, self._screen, self._hist = _leased_many(handle.pool, [((n, 10), np.int32), ((n,), np.uint32), ((n, h, w), np.uint8), ((n, h, w), np.uint8)])
        else:
            self.status = _leased(handle.pool, (n, 10), np.int32)
            self.flags = _leased(handle.pool, (n,), np.uint32)
        self._snap = None
        if keys is not None and not (handle.fast_step and not self.mixed_sizes and (h * w) % 4 == 0):
            handle.step_keys_host(keys)
            keys = None
        if keys is not None:
            # the step and its results in ONE call (rg_step_fetch): k_step reads the keys from pinned memory, one kernel writes status / flags -- and the
            # screens of a small batch -- straight into the pinned arrays below; a larger batch keeps its screens in a device snapshot, as without keys
            L = handle.L
            if eager:
                scr, hst = self._screen.ctypes.data, self._hist.ctypes.data
            else:
                self._screen = self._hist = None
                self._snap = _Lease(handle.dev_pool, 2 * n * h * w)
                scr, hst = self._snap.ptr, self._snap.ptr + n * h * w
            rc = L.rg_step_fetch(handle.h, keys.ctypes.data, int(keys.shape[0]), C.c_void_p(scr), C.c_void_p(hst), self.status.ctypes.data, self.flags.ctypes.data)
            if rc and b"config groups" in L.rg_last_error(handle.h):  # (refused before anything was stepped: the general path from now on)
                handle.fast_step = False
                self._snap = None
                handle.step_keys_host(keys)
                keys = None
            else:
                handle.epoch += 1
                handle.check(rc)
                if self._snap is not None:
                    self._register_lazy()
        if keys is not None:
            pass
        elif self.mixed_sizes:  # envs of different width / height (ParallelGameState::new takes any config per env): ragged buffers, `screen` / `hist` are lists of per-env views
            off = np.concatenate(([0], np.cumsum(handle.env_heights.astype(np.int64) * handle.env_widths)))
            rs, rh = _leased(handle.pool, (int(off[-1]),), np.uint8), _leased(handle.pool, (int(off[-1]),), np.uint8)
            self._screen = [rs[off[i]:off[i + 1]].reshape(handle.env_heights[i], handle.env_widths[i]) for i in range(n)]
            self._hist = [rh[off[i]:off[i + 1]].reshape(handle.env_heights[i], handle.env_widths[i]) for i in range(n)]
            handle.check(handle.L.rg_fetch_states(handle.h, rs.ctypes.data, rh.ctypes.data, self.status.ctypes.data, self.flags.ctypes.data))
        elif n * h * w < _LAZY_MIN_BYTES:  # small batch: one call, four copies
            self._screen = _leased(handle.pool, (n, h, w), np.uint8)
            self._hist = _leased(handle.pool, (n, h, w), np.uint8)
            handle.check(handle.L.rg_fetch_states(handle.h, self._screen.ctypes.data, self._hist.ctypes.data, self.status.ctypes.data, self.flags.ctypes.data))
        else:
            # The RL loop reads gold and is_terminal of every state and nothing else (parallel.py:59-64): status + flags (44 B per env) come to the host
            # now, the screens (1 KB per env) are snapshotted device-to-device (~30 us for 65 536 envs) and cross PCIe only when somebody looks at them
            self._screen = self._hist = None
            self._snap = _Lease(handle.dev_pool, 2 * n * h * w)
            handle.check(handle.L.rg_snapshot_take(handle.h, C.c_void_p(self._snap.ptr)))
            handle.check(handle.L.rg_fetch_states(handle.h, None, None, self.status.ctypes.data, self.flags.ctypes.data))  # (synchronises the stream)
            self._register_lazy()
        self._epoch = handle.epoch
        self._items = {}
        self._images = {}

    def _register_lazy(self):
        handle = self._hd
        key, lazy = id(self), handle.lazy
        lazy[key] = weakref.ref(self, lambda _r, key=key, lazy=lazy: lazy.pop(key, None))
        # Every lazy batch pins 2 * n * H * W bytes of HBM until it is collected or looked at: a caller that keeps the states of a whole rollout
        # (128 steps of 65 536 mini envs = 17 GB) must not exhaust the device silently.  Beyond _LAZY_MAX_BYTES the OLDEST batches get their host
        # copies now (what every batch cost before the lazy path existed) and hand their device buffer back.
        live = [b for b in (r() for r in list(lazy.values())) if b is not None and b._snap is not None]
        total = sum(b._snap.nbytes for b in live)
        for b in live:
            if total <= _LAZY_MAX_BYTES:
                break
            if b is not self:
                total -= b._snap.nbytes
                b._materialise()

    def _materialise(self):
        """Host copies of the whole snapshot (one D2H of screen + history into pinned memory); the device buffer goes back to the pool."""
        if self._snap is None:
            return
        hd = self._hd
        if hd.h is None:
            raise RuntimeError("Error in rogue-gym: the game was closed")
        n, h, w = self.n, hd.height, hd.width
        both = _leased(hd.pool, (2, n, h, w), np.uint8)
        hd.check(hd.L.rg_dev_read(hd.h, C.c_void_p(self._snap.ptr), both.ctypes.data, both.nbytes))
        self._screen, self._hist, self._snap = both[0], both[1], None
        hd.lazy.pop(id(self), None)

    @property
    def screen(self):
        """u8 [n, H, W] glyph mirrors (a list of per-env arrays when the batch mixes sizes)."""
        if self._screen is None:
            self._materialise()
        return self._screen

    @property
    def hist(self):
        if self._hist is None:
            self._materialise()
        return self._hist

    def _row(self, i):
        """Screen and history of env i: views of the host copies if they exist, else 2 x H*W bytes fetched from the device snapshot."""
        if self._snap is None:
            return self._screen[i], self._hist[i]
        hd = self._hd
        n, h, w = self.n, hd.height, hd.width
        both = np.empty((2, h, w), np.uint8)  # one 2-row copy: env i's screen and, n * H * W bytes further, its history
        hd.check(hd.L.rg_dev_read_rows(hd.h, C.c_void_p(self._snap.ptr + i * h * w), n * h * w, both.ctypes.data, h * w, 2))
        return both[0], both[1]

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(self.n))]
        if i < 0:
            i += self.n
        if not 0 <= i < self.n:
            raise IndexError(i)
        st = self._items.get(i)
        if st is None:
            # one state costs one small synchronous copy (~25 us); the whole snapshot costs its bytes at PCIe rate -- cheaper from the first access
            # for a small batch, from the ~100th for a 65 536-env one (67 MB: ~2.7 ms)
            if self._snap is not None and (self._snap.nbytes <= (16 << 20) or len(self._items) >= 128):
                self._materialise()
            scr, hist = self._row(i)
            st = self._items[i] = PlayerState(scr, hist, self.status[i], int(self._hd.env_symbols[i]), int(self.flags[i]), self._hd.device,
                                              batch=self, index=i, batch_images=self._hd.uniform_symbols and not self.mixed_sizes)
        return st

    def __iter__(self):
        return (self[i] for i in range(self.n))

    def __eq__(self, other):
        if isinstance(other, StateBatch):
            other = list(other)
        return list(self) == other

    @property
    def gold(self):
        return self.status[:, 1]

    @property
    def dungeon_level(self):
        return self.status[:, 0]

    @property
    def is_terminal(self):
        return (self.flags & RG_FLAG_TERMINAL) != 0

    def status_vec(self, flag):
        cols = [c for b, c in enumerate((0, 2, 3, 4, 5, 6, 7, 8, 9)) if int(flag) & (1 << b)]  # StatusFlagInner::to_vector (flags.rs:67-87)
        return self.status[:, cols]

    def images(self, kind, flag, with_hist):
        """f32 [n, C, H, W]: PlayerState::{gray,symbol}_image[_with_hist] of every state of the batch."""
        flag = 0 if flag is None else int(flag) & 0x1FF
        key = (int(kind), flag, bool(with_hist))
        img = self._images.get(key)
        if img is not None:
            return img
        if self.mixed_sizes:  # no common [N, C, H, W]: one image per env, each in its own size (what the reference's per-state expand gives)
            img = self._images[key] = [self[i]._image(kind, flag, with_hist) for i in range(self.n)]
            return img
        hd, L = self._hd, self._hd.L
        h, w = hd.height, hd.width
        c = (self.symbols if kind else 1) + bin(flag).count("1") + (1 if with_hist else 0)
        nbytes = self.n * c * h * w * 4
        if nbytes <= _IMAGE_BATCH_LIMIT and not hd.pool.closed:  # pinned, pooled: a fresh 16 MB numpy array per step costs more in page faults than the copy
            img = _leased(hd.pool, (self.n, c, h, w), np.float32)
        else:
            img = np.empty((self.n, c, h, w), np.float32)
        if hd.h is not None and hd.epoch == self._epoch:
            hd.check(L.rg_obs_host(hd.h, int(kind), flag, int(with_hist), img.ctypes.data))  # the device still holds exactly these states
        elif hd.uniform_symbols:  # the envs have moved on: encode the snapshot itself
            rc = L.rg_encode_host_batch(hd.device, self.n, self.screen.ctypes.data, self.hist.ctypes.data, self.status.ctypes.data, h, w, self.symbols, flag,
                                        int(with_hist), int(kind), img.ctypes.data)
            if rc:
                raise RuntimeError("Error in rogue-gym: " + L.rg_last_error(None).decode())
        else:  # configs with different `symbols` in one batch: env by env, each with its own (gray values divide by the env's symbols)
            if kind:
                raise RuntimeError("Error in rogue-gym: a batch whose configs differ in `symbols` has no common symbol-image shape once the envs moved on")
            for i in range(self.n):
                img[i] = self[i]._image(kind, flag, with_hist)
        if img.nbytes <= _IMAGE_BATCH_LIMIT:
            self._images[key] = img
        return img


class PlayerState:
    """A memory efficient representation of Agent observation (python/src/lib.rs:27-206): a value
    object holding host copies of the mirror screen, history plane, status and flags."""

    def __init__(self, screen, hist, status, symbols, flags, device=0, batch=None, index=0, batch_images=True):
        self._map = np.ascontiguousarray(screen, np.uint8)
        self._hist = np.ascontiguousarray(hist, np.uint8)
        self._status = np.ascontiguousarray(status, np.int32)
        self._symbols = int(symbols)
        self._flags = int(flags)
        self._terminal = bool(flags & RG_FLAG_TERMINAL)
        self._device = device
        self._batch, self._index = batch, index  # keeps the batch (and its pinned buffers, which these arrays are views of) alive while this view exists
        self._batch_images = batch is not None and batch_images  # images of the whole batch by one launch (not when the batch mixes `symbols`)

    def __repr__(self):
        s = self._status  # Status::fmt (player.rs:433-449)
        hunger = {0: "", 1: "hungry", 2: "weak"}[int(s[9])]
        status = "Level: %2d Gold: %5d Hp: %2d(%2d) Str: %2d(%2d) Arm: %2d Exp: %2d/%2d %s" % (
            s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], hunger)
        return "".join(row + "\n" for row in self.dungeon) + status

    __str__ = __repr__

    def __eq__(self, other):
        return (isinstance(other, PlayerState) and np.array_equal(self._map, other._map) and np.array_equal(self._hist, other._hist)
                and np.array_equal(self._status, other._status) and self._symbols == other._symbols
                and (self._flags & RG_FLAG_MSG_MASK) == (other._flags & RG_FLAG_MSG_MASK) and self._terminal == other._terminal)

    @property
    def status(self):
        return {k: int(v) & 0xFFFFFFFF for k, v in zip(STATUS_KEYS, self._status)}

    @property
    def dungeon(self):
        return [bytes(row).decode("latin-1") for row in self._map]

    @property
    def dungeon_level(self):
        return int(self._status[0])

    @property
    def gold(self):
        return int(self._status[1])

    @property
    def symbols(self):
        return self._symbols

    @property
    def is_terminal(self):
        return self._terminal

    @property
    def message_flags(self):
        """MessageFlagInner bits (python/src/flags.rs:6-39); not exposed by the reference's Python API."""
        return (self._flags & RG_FLAG_MSG_MASK) >> RG_FLAG_MSG_SHIFT

    def status_vec(self, flag):
        order = (0, 2, 3, 4, 5, 6, 7, 8, 9)  # StatusFlagInner::to_vector (flags.rs:67-87)
        return [int(self._status[order[b]]) for b in range(9) if flag & (1 << b)]

    def _image(self, kind, flag, with_hist):
        flag = 0 if flag is None else int(flag)
        h, w = self._map.shape
        c = (self._symbols if kind else 1) + bin(flag & 0x1FF).count("1") + (1 if with_hist else 0)
        b = self._batch
        if self._batch_images and b.n * c * h * w * 4 <= _IMAGE_BATCH_LIMIT:
            return b.images(kind, flag, with_hist)[self._index].copy()  # one launch serves every state of the batch
        L = load_library()
        out = np.empty((c, h, w), np.float32)
        rc = L.rg_encode_host(self._device, self._map.ctypes.data, self._hist.ctypes.data, self._status.ctypes.data, h, w, self._symbols,
                              flag, int(with_hist), kind, out.ctypes.data)
        if rc:
            raise RuntimeError("Error in rogue-gym: " + L.rg_last_error(None).decode())
        return out

    def gray_image(self, flag=None):
        return self._image(0, flag, False)

    def gray_image_with_hist(self, flag=None):
        return self._image(0, flag, True)

    def symbol_image(self, flag=None):
        return self._image(1, flag, False)

    def symbol_image_with_hist(self, flag=None):
        return self._image(1, flag, True)


_HISTORY_CAP_MAX = 1 << 20


def _keys_array(input):
    if isinstance(input, (bytes, bytearray)):
        return np.frombuffer(bytes(input), np.uint8)
    if isinstance(input, np.ndarray):
        return np.ascontiguousarray(input.astype(np.int64) & 0xFF, dtype=np.uint8)
    return np.ascontiguousarray(np.fromiter((int(k) & 0xFF for k in input), dtype=np.int64), dtype=np.uint8)


class GameState:
    """python/src/lib.rs:208-258 (one env, no auto-reset)."""

    def __init__(self, max_steps, config_str=None, device=None):
        self._h = _Handle([config_str], max_steps, auto_reset=False, device=device)
        self._max_steps = int(max_steps)
        # saved_inputs lives on the device: react() beyond max_steps + 1 keys is a no-op, so the log never outgrows that
        self._h.check(self._h.L.rg_history_enable(self._h.h, min(self._max_steps + 2, _HISTORY_CAP_MAX)))
        self._prev = None

    def screen_size(self):
        return (self._h.height, self._h.width)

    def set_seed(self, seed):
        lo = (C.c_uint64 * 1)(int(seed) & 0xFFFFFFFFFFFFFFFF)
        hi = (C.c_uint64 * 1)(0)  # `seed as u128` of a u64 (python/src/lib.rs:229-232)
        self._h.check(self._h.L.rg_seed(self._h.h, lo, hi, 1))

    def reset(self):
        self._h.check(self._h.L.rg_reset(self._h.h))
        self._h.epoch += 1
        self._prev = None

    def prev(self):
        if self._prev is None:
            self._prev = self._h.snapshot()[0]
        return self._prev

    def react(self, input):
        keys = (C.c_uint8 * 1)(int(input) & 0xFF)
        self._h.check(self._h.L.rg_step(self._h.h, keys, 0))
        self._h.epoch += 1
        self._prev = None
        self._h.check(self._h.L.rg_sync(self._h.h))

    def dump_history(self):
        return self._h.dump_history(0)

    def action_mask(self, keys=None):
        """numpy bool [n_keys]: which keys would do anything now (not part of the reference's API; rg_action_mask)."""
        return self._h.action_mask(keys)[0]

    def act(self, logits, **opts):
        """ActResult of arrays of length 1 for a row of logits [n_keys] (not part of the reference's API; rg_act_host)."""
        return self._h.act(np.asarray(logits)[None], **opts)

    def path_key(self, goal="stairs"):
        """(key byte as bytes of length 1, distance or None): the key that takes the player one move closer to the nearest goal cell and the number of
        moves to it (not part of the reference's API; rg_path -- privileged: it sees what the player has not discovered)."""
        keys, dist = self._h.path_keys(goal)
        return bytes(keys[:1]), (None if dist[0] < 0 else int(dist[0]))

    def route_key(self, goal="stairs", fallback=None, secrets=False, known=False):
        """(key byte as bytes of length 1, distance or None, tier or None): rg_route for this game (not part of the reference's API).  secrets: plan through
        hidden / locked cells and search beside them; known: plan on the player's own map only (nothing privileged then); fallback: the goal that
        answers when `goal` is not reached ("frontier" with known=True: the explorer)."""
        keys, dist, tier = self._h.route_keys(goal, fallback, secrets, known)
        return bytes(keys[:1]), (None if dist[0] < 0 else int(dist[0])), (None if tier[0] == ROUTE_NO_TIER else int(tier[0]))

    def monsters(self, mode="shown", cap=4):
        """(table numpy i16 [cap, 8], threat numpy i32 [4]): the nearest monsters of this game as rows of MONSTER_COLS and the threat words (not part of the
        reference's API; rg_monsters -- mode "all" is privileged: it lists monsters the screen does not show)."""
        table, threat = self._h.monster_tables(mode, cap)
        return table[0], threat[0]

    def objects(self, kinds="stairs+gold+door", known=False, secrets=False, cap=8):
        """(table numpy i16 [cap, 8], count numpy i32 [4]): the stairs, gold, doors and (known=True) frontier cells of this game's level as rows of
        OBJECT_COLS, ordered by the number of moves it takes to walk there, and the number of cells of each kind (not part of the reference's API;
        rg_objects -- without known=True it is privileged: it lists what the player has not discovered)."""
        table, count = self._h.object_tables(kinds, known, secrets, cap)
        return table[0], count[0]

    def save_state(self):
        """The running game as a state record (bytes; layout: include/rogue_gym_hip.h rg_state_save).  The key log goes with it, so dump_history
        after a load_state dumps the saved episode's keys."""
        return self._h.save_state_host(0)

    def load_state(self, state):
        """Put the game back into a state saved by save_state (or by HipVecRogueEnv.save_state of a handle with the same config, seed aside).
        The seed stays this game's: the next reset builds from it."""
        self._h.load_state_host(state, 0)
        self._prev = None

    def dump_config(self):
        buf = C.create_string_buffer(1 << 16)
        self._h.check(self._h.L.rg_dump_config(self._h.h, 0, buf, len(buf)))
        return buf.value.decode()

    def symbols(self):
        return self._h.symbols


class ParallelGameState:
    """python/src/lib.rs:260-335: the reference's one-OS-thread-per-env ThreadConductor becomes one
    batched kernel launch; envs auto-reset on terminal (thread_impls.rs:69-79).  states/step/reset return a StateBatch
    (a sequence of PlayerState, like the reference's Vec<PlayerState>).  Saving and restoring game states is not offered here (it is on GameState
    and HipVecRogueEnv)."""

    def __init__(self, max_steps, configs, device=None, history=0):
        self._h = _Handle(list(configs), max_steps, auto_reset=True, device=device)
        if history:
            self.enable_history(history)

    def screen_size(self):
        return (self._h.height, self._h.width)

    def symbols(self):
        return self._h.symbols

    def seed(self, seed):
        seed = [int(s) for s in seed][: self._h.n]  # zip (thread_impls.rs:45-50)
        n = len(seed)
        if n == 0:
            return
        lo = (C.c_uint64 * n)(*[s & 0xFFFFFFFFFFFFFFFF for s in seed])
        hi = (C.c_uint64 * n)(*[(s >> 64) & 0xFFFFFFFFFFFFFFFF for s in seed])
        self._h.check(self._h.L.rg_seed(self._h.h, lo, hi, n))

    def states(self):
        return self._h.snapshot()

    def step(self, input):
        """One key per env.  Like ThreadConductor::step the keys are zipped with the envs (thread_impls.rs:62-64): surplus keys are dropped,
        and with fewer keys than envs only that prefix is stepped (the reference would then wait forever for the others' replies)."""
        keys = _keys_array(input)
        return StateBatch(self._h, keys=keys)

    def reset(self):
        self._h.check(self._h.L.rg_reset(self._h.h))
        self._h.epoch += 1
        return self._h.snapshot()

    def action_masks(self, keys=None):
        """numpy bool [n, n_keys]: which keys would do anything for each env now (not part of the reference's API; rg_action_mask)."""
        return self._h.action_mask(keys)

    def act(self, logits, **opts):
        """ActResult of numpy arrays [n] for logits [n, n_keys] (not part of the reference's API; rg_act_host)."""
        return self._h.act(logits, **opts)

    def path_keys(self, goal="stairs"):
        """(keys numpy u8 [n], dist numpy i32 [n], -1 = unreachable) towards `goal` (not part of the reference's API; rg_path)."""
        return self._h.path_keys(goal)

    def route_keys(self, goal="stairs", fallback=None, secrets=False, known=False):
        """(keys numpy u8 [n], dist numpy i32 [n], tier numpy u8 [n]) of rg_route (not part of the reference's API; GameState.route_key names the arguments)."""
        return self._h.route_keys(goal, fallback, secrets, known)

    def monster_tables(self, mode="shown", cap=4):
        """(table numpy i16 [n, cap, 8], threat numpy i32 [n, 4]) of rg_monsters (not part of the reference's API; GameState.monsters names the arguments)."""
        return self._h.monster_tables(mode, cap)

    def object_tables(self, kinds="stairs+gold+door", known=False, secrets=False, cap=8):
        """(table numpy i16 [n, cap, 8], count numpy i32 [n, 4]) of rg_objects (not part of the reference's API; GameState.objects names the arguments)."""
        return self._h.object_tables(kinds, known, secrets, cap)

    def dump_config(self, env=0):
        buf = C.create_string_buffer(1 << 16)
        self._h.check(self._h.L.rg_dump_config(self._h.h, int(env), buf, len(buf)))
        return buf.value.decode()

    def enable_history(self, cap_per_env):
        """Keep the keys of the running and of the previous episode of every env on the device (not part of the reference's API)."""
        self._h.check(self._h.L.rg_history_enable(self._h.h, int(cap_per_env)))

    def dump_history(self, env, previous=False):
        """GameState::dump_history for env `env` of the batch; previous=True: the episode that ended with the last auto-reset."""
        return self._h.dump_history(int(env), previous)

    def close(self):
        self._h.close()


def replay(game, interval_ms=100):
    raise RuntimeError("replay needs the reference's terminal UI (devui), which is out of scope for the HIP stepper")


def play_cli(game):
    raise RuntimeError("play_cli needs the reference's terminal UI (devui), which is out of scope for the HIP stepper")
