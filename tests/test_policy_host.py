"""The action rule of rogue-gym_amd/csrc/rg_policy.h without a GPU, through rg_act_host (the twin the kernel k_act shares the rule with): every clause on
hand-made 5 x 5 grids, the random word and its bit fields against Python integers, logp and entropy against a float64 masked log-softmax, the chosen-action
and source counts against their expectations, the refusals -- and the rule's source in a stand-alone program built with -fsanitize=address,undefined
(tests/policy_host_main.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mask_util as mu
import policy_edge_rows as pe
import policy_util as pu
from policy_util import GIVEN, GREEDY, KEYS, STAIR, WALL, grid5

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = np.float32(-np.inf)
# the largest |difference| of logp and of entropy between the host rule and float64 over the 10 000 rows of test_accuracy_against_float64, measured on the
# CPU: 1.09e-6 and 2.29e-7 -- a few f32 ulps of the row's ln S (ln 11 = 2.4 has an ulp of 2.4e-7; d = x - m up to 25 has one of 1.9e-6).  The test asserts
# four times that: the sample is finite and the polynomials' worst case need not be in it.
MEASURED_LOGP, MEASURED_ENTROPY = 1.09e-6, 2.29e-7


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from rogue_gym_python import _rogue_gym as inner
    return inner.load_library()


@pytest.fixture(scope="module")
def inner():
    from rogue_gym_python import _rogue_gym as inner
    return inner


def test_entry_points_declared_exported_and_bound(lib, inner):
    hdr = open(os.path.join(ROOT, "include", "rogue_gym_hip.h")).read()
    for n in ("rg_act", "rg_act_host"):
        assert re.search(r"^int %s\(" % n, hdr, re.M), "not declared: " + n
        assert hasattr(lib, n), "not exported: " + n
        assert getattr(lib, n).argtypes is not None and n in inner._INT_FUNCS
    assert len(inner._ABI["rg_act"][0]) == 14 and len(inner._ABI["rg_act_host"][0]) == 19
    m = re.search(r"typedef struct rg_act_opts \{([^}]*)\}", hdr)
    assert " ".join(m.group(1).split()) == "float inv_temp, epsilon, beta; uint32_t mode; uint64_t seed, draw;"
    assert C.sizeof(inner.RgActOpts) == 32 and [f for f, _ in inner.RgActOpts._fields_] == ["inv_temp", "epsilon", "beta", "mode", "seed", "draw"]
    for name, val in (("RG_ACT_SAMPLE", 0), ("RG_ACT_GREEDY", 1), ("RG_ACT_GIVEN", 2)):
        assert re.search(r"#define %s\s+%du" % (name, val), hdr) and getattr(inner, name) == val
    from rogue_gym.envs import ParallelRogueEnv, RogueEnv
    from rogue_gym.envs.device import HipVecRogueEnv
    for cls in (RogueEnv, ParallelRogueEnv, HipVecRogueEnv):
        assert callable(cls.act) and "no autograd" in cls.act.__doc__
    assert callable(HipVecRogueEnv.step_logits)
    assert inner.ActResult._fields == ("keys", "actions", "logp", "entropy", "source") and inner.ACT_SOURCES == ("policy", "uniform", "teacher", "none")


def test_an_illegal_key_is_never_chosen(lib, inner):
    g = grid5(x3y2=WALL)   # 'l' and the diagonals beside it ('n', 'u') are illegal, and so is '>'
    legal = mu.host_row(lib, g, 2, 2, 0).astype(bool)
    assert list(np.flatnonzero(~legal)) == [KEYS.index(b"l"), KEYS.index(b"n"), KEYS.index(b"u"), KEYS.index(b">")]
    x = np.zeros(11, np.float32)
    x[~legal] = 50.0       # the largest logits by far
    seen = set()
    for e in range(4096):
        key, a, lp, ent, src = pu.act_host(lib, inner, g, 2, 2, x, env=e, seed=3, draw=1)
        assert legal[a] and key == KEYS[a] and src == 0
        assert abs(lp + np.log(7)) < 1e-6 and abs(ent - np.log(7)) < 1e-6
        seen.add(a)
    assert seen == set(np.flatnonzero(legal))
    assert pu.act_host(lib, inner, g, 2, 2, x, mode=GREEDY)[1] == 0     # ... nor by the argmax: the first of the seven equal legal logits


def test_greedy_given_temperature(lib, inner):
    g = grid5(x2y2=STAIR)   # everything legal
    x = np.array([0.5, 2.0, -1.0, 2.0, 0.0, 1.0, 2.0, -3.0, 0.25, 1.5, -0.5], np.float32)
    lp64, ent64 = pu.softmax64(x, np.ones(11, bool))
    key, a, lp, ent, src = pu.act_host(lib, inner, g, 2, 2, x, mode=GREEDY)
    assert (a, key, src) == (1, KEYS[1], 0) and abs(lp - lp64[1]) < 1e-6 and abs(ent - ent64) < 1e-6    # ties: the lowest index
    gw = grid5(x2y2=STAIR, x1y2=WALL)                                                                    # 'h' (index 1) and its diagonals go
    assert pu.act_host(lib, inner, gw, 2, 2, x, mode=GREEDY)[1] == 3
    for k in range(11):
        key, a, lp, _, src = pu.act_host(lib, inner, g, 2, 2, x, mode=GIVEN, given=k)
        assert (key, a, src) == (KEYS[k], k, 0) and abs(lp - lp64[k]) < 1e-6
    legal = mu.host_row(lib, gw, 2, 2, 0).astype(bool)
    lpw, _ = pu.softmax64(x, legal)
    for k in range(11):
        _, a, lp, _, _ = pu.act_host(lib, inner, gw, 2, 2, x, mode=GIVEN, given=k)
        assert a == k and (abs(lp - lpw[k]) < 1e-6 if legal[k] else lp == NINF)
    for bad in (-1, 11, 1 << 30, -(1 << 31)):
        key, a, lp, _, _ = pu.act_host(lib, inner, g, 2, 2, x, mode=GIVEN, given=bad)
        assert a == bad and lp == NINF and key == KEYS[0]
    for temp in (0.25, 2.0, 10.0):
        inv = float(np.float32(1.0) / np.float32(temp))
        lpt, entt = pu.softmax64((x * np.float32(inv)).astype(np.float32), np.ones(11, bool))
        _, _, lp, ent, _ = pu.act_host(lib, inner, g, 2, 2, x, mode=GIVEN, given=4, inv_temp=inv)
        assert abs(lp - lpt[4]) < 2e-6 and abs(ent - entt) < 2e-6, temp


def test_teacher_and_epsilon(lib, inner):
    g = grid5(x3y2=WALL)
    legal = mu.host_row(lib, g, 2, 2, 0).astype(bool)
    x = np.linspace(-2, 2, 11).astype(np.float32)
    lp64, _ = pu.softmax64(x, legal)
    for e in range(300):
        pol = pu.act_host(lib, inner, g, 2, 2, x, env=e, seed=9, draw=2)
        # beta = 1: the teacher's key where it is legal and listed ...
        key, a, lp, _, src = pu.act_host(lib, inner, g, 2, 2, x, env=e, seed=9, draw=2, beta=1.0, teacher=ord("j"))
        assert (key, a, src) == (ord("j"), 2, 2) and abs(lp - lp64[2]) < 1e-6     # (logp stays the policy's)
        # ... the policy's own draw where it is illegal ('l'), not listed ('J') or not a key at all
        for t in (ord("l"), ord("J"), 0, 255):
            assert pu.act_host(lib, inner, g, 2, 2, x, env=e, seed=9, draw=2, beta=1.0, teacher=t) == pol
        # epsilon = 1: the uniform draw among the legal keys, by the low 16 bits of the word
        key, a, lp, _, src = pu.act_host(lib, inner, g, 2, 2, x, env=e, seed=9, draw=2, epsilon=1.0)
        idx = (pu.fields(pu.word(9, e, 2))[2] * 7) >> 16
        assert a == np.flatnonzero(legal)[idx] and src == 1 and key == KEYS[a] and abs(lp - lp64[a]) < 1e-6
    # the first position of a key that is listed twice
    assert pu.act_host(lib, inner, g, 2, 2, x[:4], keys=b"kjjh", beta=1.0, teacher=ord("j"))[1:3:1][0] == 1


def test_dead_env_and_rows_without_weight(lib, inner):
    g = grid5()
    x = np.arange(11, dtype=np.float32)
    for mode in (0, GREEDY, GIVEN):
        assert pu.act_host(lib, inner, g, 2, 2, x, dead=1, mode=mode, given=3, env=5) == (KEYS[0], 0, 0.0, 0.0, 3)
    assert pu.act_host(lib, inner, g, 2, 2, x[:3], keys=b">>>") == (ord(">"), 0, 0.0, 0.0, 3)     # alive, but no listed key is legal
    legal = mu.host_row(lib, g, 2, 2, 0).astype(bool)    # all but '>'
    ln10 = np.float32(np.log(10))
    for fill in (np.nan, -np.inf):
        row = np.full(11, fill, np.float32)
        row[9] = 100.0    # '>' is illegal: its weight does not count
        for e in range(64):
            key, a, lp, ent, src = pu.act_host(lib, inner, g, 2, 2, row, env=e, seed=1)
            idx = (pu.fields(pu.word(1, e, 0))[2] * 10) >> 16
            assert a == np.flatnonzero(legal)[idx] and src == 1 and abs(lp + ln10) < 1e-6 and abs(ent - ln10) < 1e-6
        assert pu.act_host(lib, inner, g, 2, 2, row, mode=GREEDY)[1:5:3] == (0, 1)
    # one NaN / -inf among ordinary logits: probability 0, logp -inf, never drawn
    row = np.zeros(11, np.float32)
    row[2], row[4] = np.nan, -np.inf
    for k in (2, 4):
        assert pu.act_host(lib, inner, g, 2, 2, row, mode=GIVEN, given=k)[2] == NINF
    _, _, lp, ent, _ = pu.act_host(lib, inner, g, 2, 2, row, mode=GIVEN, given=0)
    assert abs(lp + np.log(8)) < 1e-6 and abs(ent - np.log(8)) < 1e-6
    assert all(pu.act_host(lib, inner, g, 2, 2, row, env=e)[1] not in (2, 4, 9) for e in range(512))
    # +inf is the largest finite value: it takes everything, two of them share
    row = np.zeros(11, np.float32)
    row[3] = np.inf
    assert pu.act_host(lib, inner, g, 2, 2, row, mode=GREEDY)[1:4] == (3, 0.0, 0.0)
    row[6] = np.inf
    _, a, lp, ent, _ = pu.act_host(lib, inner, g, 2, 2, row, mode=GREEDY)
    assert a == 3 and abs(lp + np.log(2)) < 1e-6 and abs(ent - np.log(2)) < 1e-6
    # +-80: the small weight underflows to 0 -- no subnormal, no NaN -- and its logp is -inf
    row = np.full(11, -80.0, np.float32)
    row[5] = 80.0
    assert pu.act_host(lib, inner, g, 2, 2, row, mode=GREEDY)[1:4] == (5, 0.0, 0.0)
    assert pu.act_host(lib, inner, g, 2, 2, row, mode=GIVEN, given=1)[2] == NINF
    assert all(pu.act_host(lib, inner, g, 2, 2, row, env=e)[1] == 5 for e in range(256))
    # ... while -80 against 0 still weighs (2^-115): a finite logp
    row = np.zeros(11, np.float32)
    row[1] = -80.0
    assert abs(pu.act_host(lib, inner, g, 2, 2, row, mode=GIVEN, given=1)[2] - (-80.0 - np.log(9))) < 1e-5


def test_16_bit_logits_equal_their_widening(lib, inner):
    g = grid5(x2y2=STAIR, x2y1=WALL)
    rng = np.random.RandomState(5)
    x = pu.special_rows(rng, 64, 11)
    x[0, :4] = [6.0e-8, -6.0e-8, 6.1e-5, 65504.0]     # binary16 subnormals, the smallest normal, the largest
    for e in range(64):
        with np.errstate(over="ignore"):
            h = x[e].astype(np.float16)   # (3e38 becomes infinity)
        b = pu.to_bf16(x[e])
        wide_b = (b.astype(np.uint32) << 16).view(np.float32)
        for o in (dict(), dict(mode=GREEDY), dict(epsilon=0.5), dict(inv_temp=0.37)):
            assert pu.act_host(lib, inner, g, 2, 2, h, env=e, **o) == pu.act_host(lib, inner, g, 2, 2, h.astype(np.float32), env=e, **o), (e, o)
            assert pu.act_host(lib, inner, g, 2, 2, b, env=e, dtype=pu.BF16, **o) == pu.act_host(lib, inner, g, 2, 2, wide_b, env=e, **o), (e, o)
    # every binary16 pattern widens exactly (the widening is integer code of the rule's own)
    allh = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    keep = np.isfinite(allh)
    for h in allh[keep][::257]:
        row16, row32 = np.array([h, 0], np.float16), np.array([h, 0], np.float32)
        assert pu.act_host(lib, inner, g, 2, 2, row16, keys=b".s", mode=GIVEN, given=0) == pu.act_host(lib, inner, g, 2, 2, row32, keys=b".s", mode=GIVEN, given=0), h


def test_the_random_word_and_its_bit_fields(lib, inner):
    g = grid5(x2y2=STAIR)
    four, two = np.zeros(4, np.float32), np.zeros(2, np.float32)
    rnd = np.random.RandomState(2)
    cases = [(0, 0, 0), (pu.M64, 0xFFFFFFFF, pu.M64), (1 << 63, 1 << 31, 1 << 63)]
    cases += [(int(rnd.randint(0, 1 << 62)) * 3 + 1, int(rnd.randint(0, 1 << 31)) * 2 + 1, int(rnd.randint(0, 1 << 62)) * 5) for _ in range(2000)]
    for seed, env, draw in cases:
        u, v, lo = pu.fields(pu.word(seed, env, draw))
        # bits 63..40: equal weights make the draw floor(u * n) -- the running sum k + 1 first exceeds u * n there (all of it exact in f32)
        assert pu.act_host(lib, inner, g, 2, 2, four, keys=b"hjkl", env=env, seed=seed, draw=draw)[1] == int(u * 4), (seed, env, draw)
        assert pu.act_host(lib, inner, g, 2, 2, two, keys=b"hj", env=env, seed=seed, draw=draw)[1] == int(u >= 0.5)
        # bits 39..16: the source, against beta and beta + epsilon (0.25 and 0.5 are exact)
        src = pu.act_host(lib, inner, g, 2, 2, four, keys=b"hjkl", env=env, seed=seed, draw=draw, beta=0.25, epsilon=0.25, teacher=ord("k"))[4]
        assert src == (2 if v < 0.25 else 1 if v < 0.5 else 0), (seed, env, draw, v)
        # bits 15..0: the uniform index by multiply-high
        for keys in (b"hjkl", b"hjklyub"):
            a = pu.act_host(lib, inner, g, 2, 2, np.zeros(len(keys), np.float32), keys=keys, env=env, seed=seed, draw=draw, epsilon=1.0)[1]
            assert a == (lo * len(keys)) >> 16
    # a stream of its own: with equal seed and draw the uniform index is not rg_sample_index's
    same = sum(((pu.fields(pu.word(5, e, 9))[2] * 11) >> 16) == lib.rg_sample_index(5, e, 9, 11) for e in range(4096))
    assert same < 2 * 4096 / 11, same


def test_words_whose_fields_stand_on_a_boundary(lib, inner):
    """policy_edge_rows.BOUNDARY_WORDS: random words whose u or v field is EXACTLY a running sum or a bound.  `c > t`, `v < beta` and `v < beta + epsilon` are strict,
    and u keeps all its 24 bits -- random words never say so (a 24-bit field hits a given value once in 1.7e7 draws)."""
    g = grid5(x2y2=STAIR)
    for (kind, value), words in pe.BOUNDARY_WORDS.items():
        assert len(words) >= 4
        for seed, env, draw in words:
            u, v, _ = pu.fields(pu.word(seed, env, draw))
            assert pe.field_of(kind, seed, env, draw) == value and (u if kind == "u" else v) * (1 << 24) == value, (kind, value, seed, env, draw)
            if kind == "u":
                n, want = pe.U_EXPECT[value]
                got = pu.act_host(lib, inner, g, 2, 2, np.zeros(n, np.float32), keys=b"hjkl"[:n], env=env, seed=seed, draw=draw)
                assert got[1] == want and got[4] == 0, (hex(value), env, draw, got)
                # the same boundary under a temperature and a common offset: equal logits stay equal
                assert pu.act_host(lib, inner, g, 2, 2, np.full(n, -3.5, np.float32), keys=b"hjkl"[:n], env=env, seed=seed, draw=draw, inv_temp=0.37)[1] == want
            else:
                pol = pu.act_host(lib, inner, g, 2, 2, np.zeros(4, np.float32), keys=b"hjkl", env=env, seed=seed, draw=draw)
                for beta, epsilon, src in pe.V_EXPECT[value]:
                    got = pu.act_host(lib, inner, g, 2, 2, np.zeros(4, np.float32), keys=b"hjkl", env=env, seed=seed, draw=draw, beta=beta, epsilon=epsilon, teacher=ord("k"))
                    assert got[4] == src and got == pol, (hex(value), beta, epsilon, got, pol)
                # ... and one step of the bound further the word IS below it: the teacher's, the uniform draw's
                up = float(np.nextafter(np.float32(value / float(1 << 24)), np.float32(1)))
                assert pu.act_host(lib, inner, g, 2, 2, np.zeros(4, np.float32), keys=b"hjkl", env=env, seed=seed, draw=draw, beta=up, teacher=ord("k"))[4] == 2
                assert pu.act_host(lib, inner, g, 2, 2, np.zeros(4, np.float32), keys=b"hjkl", env=env, seed=seed, draw=draw, epsilon=up)[4] == 1


def test_given_mode_on_a_flat_row(lib, inner):
    """RG_ACT_GIVEN answers source 0 whatever the row: on a row no legal key of which weighs (SAMPLE and GREEDY say source 1 there), logp = -ln count."""
    g = grid5()                                          # all legal but '>'
    for fill in (np.nan, -np.inf):
        row = np.full(11, fill, np.float32)
        row[9] = 4.0                                     # the illegal key's logit does not count
        for k in (0, 3, 10):
            key, a, lp, ent, src = pu.act_host(lib, inner, g, 2, 2, row, mode=GIVEN, given=k, env=k)
            assert (key, a, src) == (KEYS[k], k, 0) and abs(lp + np.log(10)) < 1e-6 and abs(ent - np.log(10)) < 1e-6, (fill, k, lp, ent, src)
        assert pu.act_host(lib, inner, g, 2, 2, row, mode=GIVEN, given=9)[2:5:2] == (NINF, 0)       # the illegal key: -inf, and still source 0
        assert pu.act_host(lib, inner, g, 2, 2, row, mode=GREEDY)[4] == 1 and pu.act_host(lib, inner, g, 2, 2, row)[4] == 1


def test_two_largest_keys_beside_one_infinitely_far_below(lib, inner):
    """+inf is FLT_MAX and a key at -3e38 stands at d = -inf below it: it weighs 0 and adds NOTHING to the sums (0 * -inf would be NaN), so two +inf keys share the
    row: logp -ln 2, entropy ln 2."""
    g = grid5(x2y2=STAIR)
    for row in (np.array([np.inf, np.inf, -3.0e38], np.float32), np.array([-3.0e38, np.finfo(np.float32).max, np.inf], np.float32)):
        k = int(np.argmax(row))
        _, _, lp, ent, _ = pu.act_host(lib, inner, g, 2, 2, row, keys=b"hjk", mode=GIVEN, given=k)
        assert abs(lp + np.log(2)) < 1e-6 and abs(ent - np.log(2)) < 1e-6, (row, lp, ent)
        assert pu.act_host(lib, inner, g, 2, 2, row, keys=b"hjk", mode=GIVEN, given=int(np.argmin(row)))[2] == NINF


def test_the_weight_cut_off_on_either_side(lib, inner):
    """w = 0 where d * log2 e is below -125, from the f32 product: d_in weighs 2^-125 (logp = d - ln S, finite), its neighbour d_out weighs nothing (-inf)."""
    g = grid5(x2y2=STAIR)
    d_in, d_out = pe.cutoff_pair()
    for d, finite in ((d_in, True), (d_out, False)):
        row = np.array([0.0, d], np.float32)            # m = 0: x - m is d itself
        _, _, lp, ent, _ = pu.act_host(lib, inner, g, 2, 2, row, keys=b"hj", mode=GIVEN, given=1)
        if finite:
            assert np.isfinite(lp) and abs(float(lp) - float(d)) <= 1e-5, (d, lp)
            assert 0 < ent < 1e-34                       # 2^-125 * 86.6 = 2.0e-36: the weight is in the sums
        else:
            assert lp == NINF and ent == 0, (d, lp, ent)
        # the dominant key is unmoved either way, and the light key is never drawn
        assert pu.act_host(lib, inner, g, 2, 2, row, keys=b"hj", mode=GIVEN, given=0)[2] == 0.0
        assert all(pu.act_host(lib, inner, g, 2, 2, row, keys=b"hj", env=e)[1] == 0 for e in range(64))


def test_the_polynomials_exhaustively(tmp_path):
    """tests/policy_poly_main.cpp: rg_pol_exp2 over every float32 of [-125, -2^-12] and rg_pol_ln over every one of [1, 32] against float64 libm, no worse than
    the worst case measured (written beside the bounds there); 6 s of CPU time on up to 16 threads.  No sanitizer: the program is arithmetic on registers."""
    cxx = shutil.which("g++") or shutil.which("clang++") or ("/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    if not os.path.exists(os.path.join(rocm_inc, "hip", "hip_runtime.h")):
        pytest.skip("no ROCm include directory (the rule headers include hip/hip_runtime.h for __host__ __device__)")
    exe = str(tmp_path / "policy_poly_main")
    # the rule headers that are swept: the checkout's, or the copy that tests/rule_mutants.py names when it runs this file against a mutant (RULE_MUTANT_PKG)
    pkg = os.environ.get("RULE_MUTANT_PKG") or os.path.join(ROOT, "rogue-gym_amd")
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I", rocm_inc, "-I", os.path.join(pkg, "csrc"), "-I", pkg,
                    os.path.join(ROOT, "tests", "policy_poly_main.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("policy_poly_main: 0 bad") and "83385 steps back, 0 of them more than one ulp" in r.stdout, r.stdout


def random_case(lib, rng):
    """(grid, key list, legal bool [11]) with at least one legal key: random walls around the player, the stairs under it or not."""
    while True:
        g = grid5(x2y2=STAIR if rng.randint(2) else pu.FLOOR)
        for x, y in ((1, 1), (2, 1), (3, 1), (1, 2), (3, 2), (1, 3), (2, 3), (3, 3)):
            if rng.randint(3) == 0:
                g[y, x] = WALL
        keys = None if rng.randint(2) else b"hjklnbuy>hj"    # the second list has no key that is always legal: down to one legal key
        legal = mu.host_row(lib, g, 2, 2, 0, KEYS if keys is None else keys).astype(bool)
        if legal.any():
            return g, keys, legal



def test_accuracy_against_float64(lib, inner):
    rng = np.random.RandomState(17)
    worst_lp = worst_ent = 0.0
    counts = np.zeros(12, np.int64)
    for _ in range(10000):
        g, keys, legal = random_case(lib, rng)
        counts[legal.sum()] += 1
        x = (rng.standard_normal(11) * 3).astype(np.float32)
        lp64, ent64 = pu.softmax64(x, legal)
        k = int(rng.choice(np.flatnonzero(legal)))
        _, _, lp, ent, _ = pu.act_host(lib, inner, g, 2, 2, x, keys=keys, mode=GIVEN, given=k)
        worst_lp, worst_ent = max(worst_lp, abs(float(lp) - lp64[k])), max(worst_ent, abs(float(ent) - ent64))
    print("largest |logp - float64| %.3g, largest |entropy - float64| %.3g, rows by legal keys %s" % (worst_lp, worst_ent, counts[1:].tolist()))
    assert counts[1] > 0 and counts[11] > 0 and (counts[1:] > 0).sum() >= 9
    assert worst_lp <= 4 * MEASURED_LOGP and worst_ent <= 4 * MEASURED_ENTROPY


def test_action_and_source_counts(lib, inner):
    """Three fixed rows, env indices 0 .. 65 535 at one (seed, draw): every action's count within 5 sigma + 1 of N p, p from float64."""
    n = 65536
    g = grid5(x2y2=STAIR, x2y3=WALL)     # 'j' and its diagonals ('n', 'b') are illegal
    legal = mu.host_row(lib, g, 2, 2, 0).astype(bool)
    assert legal.sum() == 8
    rows = [np.zeros(11, np.float32), np.linspace(-3, 3, 11).astype(np.float32), np.array([5, -2, 9, 0.5, 0.5, 7, 1, -4, 2.5, 3, -1], np.float32)]

    def within(counts, p, what):
        bound = 5 * np.sqrt(n * p * (1 - p)) + 1
        assert (np.abs(counts - n * p) <= bound).all(), (what, counts, n * p, bound)

    opts = pu.opts_of(inner, seed=2024, draw=6)
    mixed = pu.opts_of(inner, seed=2024, draw=6, epsilon=0.2, beta=0.3)
    act, src = C.c_int32(), C.c_uint8()
    key = C.c_uint8()
    for r, x in enumerate(rows):
        lp64, _ = pu.softmax64(x, legal)
        hist, srcs, chosen = np.zeros(11, np.int64), np.zeros(4, np.int64), np.zeros(11, np.int64)
        for e in range(n):
            lib.rg_act_host(g.ctypes.data, 5, 5, 2, 2, 0, None, 0, x.ctypes.data, 0, C.byref(opts), e, -1, 0, C.byref(key), C.byref(act), None, None, None)
            hist[act.value] += 1
            lib.rg_act_host(g.ctypes.data, 5, 5, 2, 2, 0, None, 0, x.ctypes.data, 0, C.byref(mixed), e, ord("h"), 0, C.byref(key), C.byref(act), None, None, C.byref(src))
            srcs[src.value] += 1
            chosen[act.value] += 1
        p = np.exp(lp64)
        within(hist, p, "row %d actions" % r)
        assert hist[~legal].sum() == 0
        within(srcs, np.array([0.5, 0.2, 0.3, 0.0]), "row %d sources" % r)
        teacher = np.zeros(11)
        teacher[1] = 1.0
        within(chosen, 0.5 * p + 0.2 * legal / 8.0 + 0.3 * teacher, "row %d mixed actions" % r)


def test_refusals_name_the_argument_and_write_nothing(lib, inner):
    g = grid5()
    x = np.zeros(32, np.float32)

    def refused(words, keys=None, nk=0, dtype=0, px=2, teacher=-1, cells=True, logits=True, key=True, null_opts=False, **o):
        k, a = C.c_uint8(0xAA), C.c_int32(-7)
        opts = pu.opts_of(inner, **o)
        rc = lib.rg_act_host(g.ctypes.data if cells else None, 5, 5, px, 2, 0, keys, nk, x.ctypes.data if logits else None, dtype, None if null_opts else C.byref(opts), 0,
                             teacher, 0, C.byref(k) if key else None, C.byref(a), None, None, None)
        msg = lib.rg_last_error(None).decode()
        assert rc != 0 and msg.startswith("rg_act_host:") and all(w in msg for w in words), (words, msg)
        assert k.value == 0xAA and a.value == -7

    refused(("n_keys", "got 0"), b"h", 0)
    refused(("n_keys", "33"), b"h" * 33, 33)
    refused(("keys[2]", "0x78"), b"hjxk", 4)
    refused(("dtype", "got 3"), dtype=3)
    refused(("dtype", "got -1"), dtype=-1)
    refused(("opts",), null_opts=True)
    refused(("mode", "got 3"), mode=3)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused(("inv_temp",), inv_temp=bad)
    for bad in (-0.01, 1.01, float("nan")):
        refused(("epsilon",), epsilon=bad)
        refused(("beta",), beta=bad, teacher=ord("h"))
    refused(("epsilon + opts.beta",), epsilon=0.6, beta=0.5, teacher=ord("h"))
    refused(("beta", "teacher"), beta=0.5)
    refused(("key", "draws"), key=False)
    refused(("cells", "logits"), cells=False)
    refused(("cells", "logits"), logits=False)
    refused(("(px, py)",), px=5)
    # RG_ACT_GIVEN draws nothing: key may be NULL there
    opts, lp = pu.opts_of(inner, mode=GIVEN), C.c_float(7.0)
    assert lib.rg_act_host(g.ctypes.data, 5, 5, 2, 2, 0, None, 0, x.ctypes.data, 0, C.byref(opts), 0, -1, 4, None, None, C.byref(lp), None, None) == 0
    assert abs(lp.value + np.log(10)) < 1e-6


def test_rule_source_under_address_and_undefined_sanitizers(tmp_path):
    """rg_act_host's source (csrc/rg_policy.h and rg_readers_host.h) in a stand-alone program of its own -- nothing sanitized is loaded into python."""
    cxx = shutil.which("g++") or shutil.which("clang++") or ("/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    if not os.path.exists(os.path.join(rocm_inc, "hip", "hip_runtime.h")):
        pytest.skip("no ROCm include directory (the rule headers include hip/hip_runtime.h for __host__ __device__)")
    exe = str(tmp_path / "policy_host_main")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []   # the runtimes inside the program (clang's default)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   ["-D__HIP_PLATFORM_AMD__", "-I", rocm_inc, "-I", os.path.join(ROOT, "rogue-gym_amd", "csrc"), "-I", os.path.join(ROOT, "rogue-gym_amd"),
                    os.path.join(ROOT, "tests", "policy_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith(", 0 bad"), r.stdout
