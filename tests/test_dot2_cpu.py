"""CPU tier: the packed-pair primitives of csrc/fixmath.h (dot2_i16, pair_at / pair_next) in their CA_HOST_EMU form
(tests/emu/dot2_emu.cpp) against a Python reference: c + lo*lo + hi*hi on the signed 16-bit halves, wrapping mod 2^32 --
the arithmetic of a chain of the reference's MAC16_16. The device form (v_dot2c_i32_i16) is driven at the same corner
values by tests/test_pitch_dot2_gpu.py through the pitch_xcorr hook."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "dot2_emu.cpp")
HDRS = [os.path.join(ROOT, "concentus_amd", "csrc", f) for f in ("fixmath.h", "wave.h")]
PATH = os.path.join(ROOT, "tests", "emu", "libdot2_emu.so")

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


@pytest.fixture(scope="module")
def emu():
    newest = max(os.path.getmtime(f) for f in HDRS + [SRC])
    if not os.path.exists(PATH) or os.path.getmtime(PATH) < newest:
        subprocess.check_call(["g++", "-O2", "-fwrapv", "-std=c++17", "-shared", "-fPIC", "-w", "-o", PATH, SRC])
    return C.CDLL(PATH)


def _pack(lo, hi):
    return ((np.asarray(lo, np.int64) & 0xffff) | ((np.asarray(hi, np.int64) & 0xffff) << 16)).astype(np.uint32)


def _wrap32(v):
    """Python int (arbitrary precision) -> the int32 it wraps to"""
    return ((int(v) + 2 ** 31) % 2 ** 32) - 2 ** 31


def _ref_dot2(alo, ahi, blo, bhi, c):
    return np.array([_wrap32(int(c[i]) + int(alo[i]) * int(blo[i]) + int(ahi[i]) * int(bhi[i])) for i in range(len(c))], np.int32)


def _run_dot2(emu, alo, ahi, blo, bhi, c):
    a, b = _pack(alo, ahi), _pack(blo, bhi)
    c = np.asarray(c, np.int32)
    out = np.zeros(len(c), np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    emu.emu_dot2_i16(p(a), p(b), p(c), p(out), len(c))
    return out


def test_dot2_random_pairs(emu):
    rng = np.random.default_rng(20)
    n = 4096
    alo, ahi, blo, bhi = (rng.integers(-32768, 32768, n) for _ in range(4))
    c = rng.integers(INT32_MIN, INT32_MAX + 1, n)
    assert np.array_equal(_run_dot2(emu, alo, ahi, blo, bhi, c), _ref_dot2(alo, ahi, blo, bhi, c))


def test_dot2_corners(emu):
    """Every combination of the extreme halves with the extreme accumulators; (-32768, -32768).(-32768, -32768) is the
    one pair whose sum alone is 2^31 and must wrap, not clamp."""
    h = [-32768, -32767, -1, 0, 1, 32767]
    acc = [INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX]
    grid = np.array([(a, b, x, y, c) for a in h for b in h for x in h for y in h for c in acc], np.int64)
    alo, ahi, blo, bhi, c = grid.T
    got = _run_dot2(emu, alo, ahi, blo, bhi, c)
    assert np.array_equal(got, _ref_dot2(alo, ahi, blo, bhi, c))
    m = [-32768]
    assert _run_dot2(emu, m, m, m, m, [0])[0] == INT32_MIN                  # 2^31 wraps to INT32_MIN
    assert _run_dot2(emu, m, m, m, m, [INT32_MIN])[0] == 0
    assert _run_dot2(emu, m, m, m, m, [INT32_MAX])[0] == -1
    assert _run_dot2(emu, [0], [0], [0], [0], [INT32_MAX])[0] == INT32_MAX
    assert _run_dot2(emu, [0], [0], m, m, [INT32_MIN])[0] == INT32_MIN


def test_pair_at_and_pair_next(emu):
    rng = np.random.default_rng(21)
    n = 2048
    s = rng.integers(-32768, 32768, (n, 4))
    s[:8] = [[-32768] * 4, [32767] * 4, [0] * 4, [-1] * 4, [-32768, 32767, -32768, 32767], [0, -1, 0, -1],
             [1, 2, 3, 4], [-1, 0, 0, -32768]]
    w0, w1 = _pack(s[:, 0], s[:, 1]), _pack(s[:, 2], s[:, 3])
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    for odd in (0, 1):
        out = np.zeros(n, np.uint32)
        emu.emu_pair_at(p(w0), p(w1), p(np.full(n, odd, np.int32)), p(out), n)
        assert np.array_equal(out, _pack(s[:, odd], s[:, odd + 1])), odd
    out = np.zeros(n, np.uint32)
    emu.emu_pair_next(p(w0), p(w1), p(out), n)
    assert np.array_equal(out, _pack(s[:, 1], s[:, 2]))
