"""CPU tier: the second front stage of the frame kernel with both channels in one index space (mdct_forward_wave2,
band_energies_joint, normalise_bands_joint -- what celt_front2_kernel runs) against the single-channel routines called once
per channel on the same input. Host build of the kernel sources (tests/emu/front2_joint_emu.cpp); equality is bitwise.
One lane runs here: which lane does what is the GPU tier's business (tests/test_front2_joint_gpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "emu", "libfront2_joint_emu.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "emu", "front2_joint_emu.cpp")
        d = os.path.join(ROOT, "concentus_amd", "csrc")
        newest = max(os.path.getmtime(f) for f in [os.path.join(d, f) for f in os.listdir(d) if f.endswith(".h")] + [src])
        if not os.path.exists(PATH) or os.path.getmtime(PATH) < newest:
            subprocess.check_call(["g++", "-O2", "-fwrapv", "-std=c++17", "-shared", "-fPIC", "-w", "-o", PATH, src])
        _lib = C.CDLL(PATH)
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


SIG_SHIFT = 12          # the time signal is 16-bit PCM scale << 12 (celt_preemphasis)


def _frames():
    """name -> in_ws [2][1080] int32"""
    rng = np.random.default_rng(20)
    n = np.arange(1080)
    noise = rng.integers(-12000, 12000, size=(2, 1080)).astype(np.int64)
    attack = rng.integers(-300, 300, size=(2, 1080)).astype(np.int64)
    attack[:, 600:] = rng.integers(-30000, 30000, size=(2, 480))                      # mid-frame attack
    silent = noise.copy()
    silent[1] = 0                                                                     # one silent channel: "no energy" shifts
    full = np.empty((2, 1080), np.int64)
    full[0] = np.where(rng.integers(0, 2, 1080) == 1, 32767, -32768)                  # full-scale, random sign
    full[1] = np.round(32767 * np.sin(2 * np.pi * 997.0 * n / 48000.0))               # full-scale tone
    out = {"long": noise, "transient": attack, "silent_channel": silent, "full_scale": full}
    return {k: np.ascontiguousarray((v << SIG_SHIFT).astype(np.int32)) for k, v in out.items()}


FRAMES = _frames()
# the block size a frame of that kind is coded with, and the other one as well: both instantiations see every input
CASES = [("long", 0), ("transient", 8), ("silent_channel", 0), ("silent_channel", 8), ("full_scale", 0), ("full_scale", 8),
         ("long", 8), ("transient", 0)]


def _run(fn, sig, short):
    coef = np.zeros((2, 960), np.int32)
    bandE = np.zeros(42, np.int32)
    logE = np.zeros(42, np.int16)
    X = np.zeros((2, 960), np.int16)
    fn(_p(sig), short, _p(coef), _p(bandE), _p(logE), _p(X))
    return coef, bandE, logE, X


@pytest.mark.parametrize("name,short", CASES, ids=["%s-%s" % (n, "short" if s else "long") for n, s in CASES])
def test_joint_front2_equals_single_channel_routines(name, short):
    L = lib()
    sig = FRAMES[name]
    coef_j, bandE_j, logE_j, X_j = _run(L.emu_front2_joint, sig, short)
    coef_s, bandE_s, logE_s, X_s = _run(L.emu_front2_single, sig, short)
    assert np.any(coef_s[0] != 0)
    if name == "silent_channel":
        assert not coef_s[1].any() and (bandE_s[21:] == 1).all()                       # the "no energy" path was taken
    assert np.array_equal(coef_j, coef_s), "MDCT coefficients"
    assert np.array_equal(bandE_j, bandE_s), "bandE"
    assert np.array_equal(logE_j, logE_s), "bandLogE"
    assert np.array_equal(X_j[:, :800], X_s[:, :800]), "normalised bands X"


def test_joint_band_energies_on_extreme_coefficients():
    """values no transform produces: the largest magnitudes, -2^31 among them (its negation wraps), alone and next to others"""
    L = lib()
    rng = np.random.default_rng(21)
    coef = rng.integers(-2 ** 20, 2 ** 20, size=(2, 960)).astype(np.int32)
    lo, hi = np.int32(-2 ** 31), np.int32(2 ** 31 - 1)
    coef[0, 3] = lo                      # band 0: -2^31 next to small values
    coef[0, 8:16] = 0
    coef[0, 9] = lo                      # band 1: -2^31 alone: maximum 0
    coef[0, 17] = lo
    coef[0, 20] = hi                     # band 2: both extremes
    coef[1, 5] = -2 ** 31 + 1            # largest magnitude whose negation does not wrap
    coef[1, 700] = lo                    # a wide band, -2^31 in one chunk, a larger positive value in another
    coef[1, 650] = 2 ** 30
    coef[1, 100:104] = hi
    res = []
    for fn in (L.emu_band_energies_joint, L.emu_band_energies_single):
        bandE = np.zeros(42, np.int32)
        logE = np.zeros(42, np.int16)
        fn(_p(np.ascontiguousarray(coef)), _p(bandE), _p(logE))
        res.append((bandE, logE))
    assert np.array_equal(res[0][0], res[1][0]), "bandE"
    assert np.array_equal(res[0][1], res[1][1]), "bandLogE"


def test_front2_working_set_admits_16_wavefronts_per_cu():
    assert lib().emu_front2_lds_bytes() * 16 <= 160 * 1024
