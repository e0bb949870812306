"""Pitched test signals for the packed-pair pitch loops of the front kernel (tests/test_pitch_dot2_*): stereo int16
frames [n][960][2] whose pitch candidates cover both parities of the half-rate period (the one-word and the two-word
reads of remove_doubling's inner products), at full scale and at an amplitude of at most 40; and the one shape that
reaches the shifted (sh != 0) path of the autocorrelation (flat_envelope)."""
import numpy as np


def harmonic(periods, nframes_each, amp, seed):
    """One stream per period: `nframes_each` consecutive frames of a tone with that period (in 48 kHz samples) and a few
    decaying harmonics, peak `amp`; the right channel is the left one a few samples late and a little weaker."""
    rng = np.random.default_rng(seed)
    t = np.arange(nframes_each * 960 + 8)
    out = np.zeros((len(periods), nframes_each * 960, 2), np.int16)
    for s, P in enumerate(periods):
        x = sum(np.sin(2 * np.pi * k * (t + rng.integers(0, P)) / P) / k for k in range(1, 6))
        x = x / np.abs(x).max() * amp
        out[s, :, 0] = np.clip(np.rint(x[8:]), -32768, 32767)
        out[s, :, 1] = np.clip(np.rint(0.8 * x[5:-3]), -32768, 32767)
    return out.reshape(len(periods) * nframes_each, 960, 2)


def periods(n):
    """n periods spread over 31 ... 640 samples, odd and even alternating"""
    p = np.linspace(31, 640, n).astype(int)
    p[1::2] |= 1
    p[0::2] &= ~1
    p[0], p[-1] = 31, 640
    return [int(v) for v in p]


def tones(n_streams, nframes_each, seed):
    """half the streams at full scale, half at amplitude <= 40 (alternating, so both halves see all period ranges)"""
    ps = periods(n_streams)
    loud = harmonic(ps[0::2], nframes_each, 32767, seed).reshape(-1, nframes_each, 960, 2)
    soft = harmonic(ps[1::2], nframes_each, 40, seed + 1).reshape(-1, nframes_each, 960, 2)
    out = np.zeros((n_streams, nframes_each, 960, 2), np.int16)
    out[0::2], out[1::2] = loud, soft
    return out.reshape(n_streams * nframes_each, 960, 2)


def squares_and_noise(n, seed):
    """n/2 frames of full-scale square waves (+32767 / -32768, half-periods 1 ... 400 samples, both channels, the right one
    inverted on odd frames) and n/2 frames of uniform full-scale noise"""
    rng = np.random.default_rng(seed)
    pcm = np.zeros((n, 960, 2), np.int16)
    half = np.unique(np.geomspace(1, 400, n // 2).astype(int))
    for f in range(n // 2):
        h = int(half[f % len(half)]) + (f // len(half))
        sq = np.where(((np.arange(960) + 3 * f) // h) % 2 == 0, 32767, -32768)
        pcm[f, :, 0] = sq
        pcm[f, :, 1] = sq if f % 2 == 0 else -1 - sq
    pcm[n // 2:] = rng.integers(-32768, 32768, size=(n - n // 2, 960, 2), dtype=np.int16)
    return pcm


def flat_envelope(half_periods, nframes_each, amps=(24000, 20000)):
    """One stream per half-period: a square wave run through the inverse of the encoder's pre-emphasis (y[n] = s[n] +
    0.85 y[n-1]), so that the pre-emphasised signal the pitch analysis sees is a square again, identical in both channels.
    The down-sampled buffer is scaled to |x_lp| < 2048, so _celt_autocorr's shift (ac0 >= 2^22, mean x_lp^2 above
    ~1450^2) needs an envelope flatter than a sine's over a buffer without a zero half: only frames after the first of
    such a stream get there, and only with the peak in the upper part of its octave (24000, 20000: not 32767, not 17000)."""
    n = nframes_each * 960
    out = np.zeros((len(half_periods), n, 2), np.int16)
    for s, h in enumerate(half_periods):
        sq = np.where((np.arange(n) // h) % 2 == 0, 1.0, -1.0)
        y = np.zeros(n)
        m = 0.0
        for i in range(n):
            m = sq[i] + 0.85 * m
            y[i] = m
        out[s, :, 0] = out[s, :, 1] = np.rint(y / np.abs(y).max() * amps[s % len(amps)])
    return out.reshape(len(half_periods) * nframes_each, 960, 2)
