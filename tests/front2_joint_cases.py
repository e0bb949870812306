"""Inputs of tests/test_front2_joint_gpu.py and of the script that records its expected packets
(tests/golden/make_front2_joint_golden.py): 256 independent-or-streamed frame slots chosen for the paths of the second front
stage -- short blocks (noise, attack), the transient patch's second transform after long blocks (streams), the "no energy"
bands of a silent channel."""
import hashlib

import numpy as np

CFG = (96000, 1, 0, 10)            # bitrate, vbr, constrained vbr, complexity
STREAMS, STREAM_FRAMES = 64, 10


def noise():
    return np.random.default_rng(101).integers(-8192, 8192, size=(64, 960, 2), dtype=np.int16)


def _tri(t, period, amp):
    """triangle wave in integer arithmetic (the same samples on every machine)"""
    h = period // 2
    return amp * (2 * np.abs(t % period - h) - h) // h


def attack():
    """a mid-frame attack on a quiet floor, a hard step to noise (even frames) or a tone mix swelling over 400 samples (odd):
    the transient detector's case, short blocks at once"""
    rng = np.random.default_rng(102)
    pcm = rng.integers(-60, 60, size=(64, 960, 2)).astype(np.int64)
    t = np.arange(960, dtype=np.int64)
    for n in range(64):
        at = 300 + 6 * n
        if n % 2 == 0:
            pcm[n, at:] += rng.integers(-20000, 20000, size=(960 - at, 2))
        else:
            env = np.clip(t - at, 0, 400) ** 2                                   # / 160000
            x = env * (_tri(t, 240 - 3 * n, 9000) + _tri(t, 41 + n, 4000)) // 160000
            pcm[n] += np.stack([x, -(4 * x) // 5], -1)
    return np.clip(pcm, -32768, 32767).astype(np.int16)


def one_channel_zero():
    pcm = np.random.default_rng(103).integers(-8192, 8192, size=(64, 960, 2), dtype=np.int16)
    pcm[:32, :, 1] = 0
    pcm[32:, :, 0] = 0
    return pcm


def streams():
    """64 streams of 10 frames, stream-major [64 * 10][960][2]: broadband noise that swells by an octave every 500 to 700
    samples from frame 1 + s % 3 on -- too smooth for the transient detector, so those frames are transformed with long
    blocks first, and fast enough for the energy patch (patch_transient_decision) to order short blocks after all"""
    rng = np.random.default_rng(104)
    t = np.arange(STREAM_FRAMES * 960, dtype=np.int64)
    pcm = np.empty((STREAMS, STREAM_FRAMES * 960, 2), np.int64)
    for s in range(STREAMS):
        P = 500 + 50 * (s % 5)
        u = np.clip(t - (1 + s % 3) * 960, 0, 8 * P - 1)
        env = ((P + u % P) << (u // P)) * 100 // P                                # 100 .. 25 600, of 1000
        pcm[s] = env[:, None] * rng.integers(-1000, 1000, size=(STREAM_FRAMES * 960, 2)) // 1000
    return np.clip(pcm, -32768, 32767).astype(np.int16).reshape(STREAMS * STREAM_FRAMES, 960, 2)


INDEPENDENT = (("noise", noise), ("attack", attack), ("one_channel_zero", one_channel_zero))


def digest(pcm):
    return hashlib.sha256(np.ascontiguousarray(pcm).tobytes()).hexdigest()
