"""GPU tier: the packed-pair (v_dot2c_i32_i16) pitch loops of celt_front1_kernel, bit-exact against the compiled reference
run live (oracle/_ref/librefdrv.so): packets, lengths and final ranges of pitched material whose candidates hit both
parities of the half-rate period, as first frames and as streams (history, prev_period / prev_gain, the shifted
autocorrelation), of full-scale squares and noise; and the primitive itself at chosen values through the pitch_xcorr hook
against the reference's own celt_pitch_xcorr -- all samples -32768 is the one input whose pair sum alone is 2^31, which
the non-clamping instruction must wrap as the reference's C does."""
import ctypes as C
import os

import numpy as np
import pytest

import encode_cases as ec
import pitch_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = (96000, 1, 0, 10)


@pytest.fixture(scope="module")
def ca():
    import torch
    assert torch.cuda.is_available()
    import concentus_amd
    concentus_amd.lib.load()
    return concentus_amd


def _need_ref():
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "librefdrv.so")):
        pytest.skip("oracle/_ref did not travel")
    return ec.golden_module()


def _gpu_encode(ca, pcm, fps):
    import torch
    n = pcm.shape[0]
    if fps == 1:
        out, lens, rng = ca.encode_independent(torch.from_numpy(np.ascontiguousarray(pcm)).cuda(),
                                               ca.CeltConfig(2, CFG[0], CFG[1], CFG[2], CFG[3], 16, 0, 1500))
        torch.cuda.synchronize()
        return out.cpu().numpy(), lens.cpu().numpy(), rng.cpu().numpy().view(np.uint32)
    ns = n // fps
    enc = ca.OpusEncoderBatch(ns).apply_opus_demo_ctls(*CFG)
    outs = np.zeros((n, 1280), np.uint8)
    lens = np.zeros(n, np.int32)
    rngs = np.zeros(n, np.uint32)
    p4 = pcm.reshape(ns, fps, 960, 2)
    for f in range(fps):
        o, l = enc.encode(torch.from_numpy(np.ascontiguousarray(p4[:, f])).cuda())
        torch.cuda.synchronize()
        idx = np.arange(ns) * fps + f
        o = o.cpu().numpy()
        outs[idx, :o.shape[1]] = o
        lens[idx] = l.cpu().numpy()
        rngs[idx] = enc.ctl(4031).cpu().numpy().view(np.uint32)
    return outs, lens, rngs


def _check(ca, pcm, fps, what):
    gm = _need_ref()
    pk, ln, rg = gm.ref_encode(gm._Cfg(2, CFG[0], CFG[1], CFG[2], CFG[3], 16, 0, 1500), pcm, fps, threads=8)
    out, lens, rng = _gpu_encode(ca, pcm, fps)
    ec.assert_packets_equal(out, lens, rng, pk, ln, rg, what)


def test_tones_independent_frames(ca):
    """(a) 64 first frames: harmonic tones, periods 31 ... 640 samples, half at full scale, half at amplitude <= 40"""
    _check(ca, pitch_cases.tones(64, 1, 60), 1, "tones, 64 independent frames")


def test_tones_streams(ca):
    """(b) 16 streams x 4 consecutive frames of the same material: non-zero history, prev_period / prev_gain"""
    _check(ca, pitch_cases.tones(16, 4, 61), 4, "tones, 16 streams x 4 frames")


def test_flat_envelope_streams(ca):
    """(b) the streams whose later frames take the shifted (sh != 0) autocorrelation (tests/test_pitch_dot2_emu_cpu.py
    counts that path on the same generator)"""
    _check(ca, pitch_cases.flat_envelope([32, 50, 100, 167, 31, 75, 240, 333], 4), 4, "flat envelope, 8 streams x 4 frames")


def test_squares_and_noise(ca):
    """(c) 64 frames: full-scale +32767 / -32768 square waves and uniform full-scale noise"""
    _check(ca, pitch_cases.squares_and_noise(64, 62), 1, "squares and noise, 64 independent frames")


def _xcorr(ca, x, y, len_, max_pitch):
    L = ca.lib.load()
    got = np.zeros(max_pitch, np.int32)
    mx = L.opusgpu_celt_pitch_xcorr(x.ctypes.data, y.ctypes.data, got.ctypes.data, len_, max_pitch, 0)
    assert L.opusgpu_get_last_error() == 0
    win = np.lib.stride_tricks.sliding_window_view(y.astype(np.int64), len_)[:max_pitch]
    exp = ((win * x.astype(np.int64)).sum(1) & 0xffffffff).astype(np.uint32).view(np.int32)
    assert np.array_equal(got, exp), (len_, max_pitch)
    assert mx == max(1, int(exp.max()))
    import reflib
    if reflib.available():
        ref = reflib.lib()
        want = np.zeros(max_pitch, np.int32)
        ref.celt_pitch_xcorr.restype = C.c_int32
        rmx = ref.celt_pitch_xcorr(C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data), C.c_void_p(want.ctypes.data), len_, max_pitch, 0)
        assert np.array_equal(got, want) and mx == rmx, (len_, max_pitch)


def test_hook_all_minus_32768(ca):
    """(d) x, y all -32768: every pair sum is 2^31. len 2: one pair, the sum wraps to INT32_MIN; len 3 / 241: the odd tail;
    len 8: four pairs wrap back to 0."""
    for len_ in (2, 3, 8, 241):
        for max_pitch in (1, 4, 7):
            x = np.full(len_, -32768, np.int16)
            y = np.full(len_ + max_pitch - 1, -32768, np.int16)
            _xcorr(ca, x, y, len_, max_pitch)


def test_hook_random_full_range(ca):
    rng = np.random.default_rng(63)
    for len_, max_pitch in ((2, 1), (3, 4), (8, 7), (241, 7), (240, 244), (480, 257)):
        x = rng.integers(-32768, 32768, size=len_, dtype=np.int16)
        y = rng.integers(-32768, 32768, size=len_ + max_pitch - 1, dtype=np.int16)
        x[:2] = (-32768, 32767)
        _xcorr(ca, x, y, len_, max_pitch)
