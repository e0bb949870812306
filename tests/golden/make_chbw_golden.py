"""Golden vectors of the decoder's channel-count / bandwidth support: CELT-only 20 ms packets with the eight TOCs
0x98 0xB8 0xD8 0xF8 (mono) / 0x9C 0xBC 0xDC 0xFC (stereo), encoded by the compiled reference (opus_encoder_create(48000, ch,
OPUS_APPLICATION_RESTRICTED_LOWDELAY) with OPUS_SET_BANDWIDTH / OPUS_SET_FORCE_CHANNELS changed between frames), and the
reference's opus_decode() output on a (48000, 2) decoder: PCM, final range, return value. Writes tests/golden/chbw_golden.npz.

    python tests/golden/make_chbw_golden.py        (needs oracle/_ref/libopus_ref.so and librefdrv.so)
"""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "chbw_golden.npz")
sys.path.insert(0, os.path.dirname(HERE))
import reflib  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
gm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gm)

BANDWIDTH = {13: 1101, 17: 1103, 19: 1104, 21: 1105}           # end band -> OPUS_BANDWIDTH_{NARROW,WIDE,SUPERWIDE,FULL}BAND
TOCS = [0x98, 0xB8, 0xD8, 0xF8, 0x9C, 0xBC, 0xDC, 0xFC]


def toc_of(ch, end):
    return 0x98 | ([13, 17, 19, 21].index(end) << 5) | (4 if ch == 2 else 0)


def settings_of(toc):
    return (2 if toc & 4 else 1), [13, 17, 19, 21][(toc >> 5) & 3]


def encode_stream(pcm, settings, bitrate, vbr=1, cvbr=0, complexity=10, enc_channels=2):
    """One stream through the reference encoder. pcm int16 [n][960][2] (channel 0 alone for a 1-channel encoder); settings: per
    frame (channels, end band), set with OPUS_SET_FORCE_CHANNELS / OPUS_SET_BANDWIDTH before the frame, or None (OPUS_AUTO for
    both). Returns packets [n][1280], lengths [n]; asserts every packet's TOC against the intended one."""
    ref = reflib.lib()
    ref.opus_encoder_ctl.restype = C.c_int
    ref.opus_encoder_ctl.argtypes = [C.c_void_p, C.c_int, C.c_int]
    err = C.c_int(0)
    enc = C.c_void_p(ref.opus_encoder_create(48000, enc_channels, 2051, C.byref(err)))
    assert err.value == 0 and enc
    for req, v in ((4002, bitrate), (4006, vbr), (4020, cvbr), (4010, complexity), (4012, 0), (4016, 0), (4014, 0), (4036, 16),
                   (4040, 5000)):
        assert ref.opus_encoder_ctl(enc, req, v) == 0, req
    n = pcm.shape[0]
    out = np.zeros((n, 1280), np.uint8)
    lens = np.zeros(n, np.int32)
    for f in range(n):
        ch, end = settings[f] if settings[f] is not None else (None, None)
        assert ref.opus_encoder_ctl(enc, 4008, BANDWIDTH[end] if end else -1000) == 0
        assert ref.opus_encoder_ctl(enc, 4022, ch if ch and enc_channels == 2 else -1000) == 0
        fr = np.ascontiguousarray(pcm[f] if enc_channels == 2 else pcm[f, :, 0])
        r = ref.opus_encode(enc, fr.ctypes.data_as(C.c_void_p), 960, out[f].ctypes.data_as(C.c_void_p), 1276)
        assert r > 0, (f, r)
        lens[f] = r
        if settings[f] is not None:
            want = toc_of(ch if enc_channels == 2 else 1, end)
            assert out[f, 0] == want, "frame %d: TOC 0x%02X, intended 0x%02X" % (f, out[f, 0], want)
    ref.opus_encoder_destroy(enc)
    return out, lens


def _blocks(*per_block, each=4):
    s = []
    for b in per_block:
        s += [b] * each
    return s


def _pcm(kinds, n, seed):
    """n frames, the kinds in turn in runs of n / len(kinds) frames"""
    run = n // len(kinds)
    return np.concatenate([gm.synth_pcm(k, run, seed + i) for i, k in enumerate(kinds)])


S, M = 2, 1
SWITCH = _blocks((S, 21), (M, 21), (S, 19), (M, 13), (S, 21), (M, 17), (S, 13), (S, 21))
# stream 0: a loss right after an NB packet (6), right after a mono packet (14), seven in a row after a WB packet (20-26: noise-based
# from the sixth, over 17 bands). stream 1: a fullband stretch, a one-byte 0x98 packet (12) with two lost packets after it, a
# one-byte 0xF8 (20), then narrower settings again
SWITCH_LOSS = [
    (_blocks((S, 21), (S, 13), (S, 21), (M, 21), (S, 17), (S, 17), (S, 19), (S, 21)), [6, 14] + list(range(20, 27)), []),
    (_blocks((S, 21), (S, 21), (S, 21), (S, 21), (S, 21), (M, 21), (M, 17), (S, 19)), [13, 14], [(12, 0x98), (20, 0xF8)]),
]
STATIC_RATES = {0x98: 24000, 0xB8: 32000, 0xD8: 40000, 0xF8: 48000, 0x9C: 32000, 0xBC: 40000, 0xDC: 48000, 0xFC: 64000}


def chbw_cases():
    """name -> (packets [n][stride], lengths [n] (0: lost, 1: one-byte DTX packet), frames per stream)"""
    cases = {}
    for toc in TOCS:
        pcm = _pcm(["music", "edge"], 8, 100 + toc)
        pk, ln = encode_stream(pcm, [settings_of(toc)] * 8, STATIC_RATES[toc], vbr=int((toc & 0x20) == 0), cvbr=int((toc & 0x40) != 0))
        cases["static_%02x" % toc] = (pk, ln, 8)
    # a 1-channel encoder, with digital silence at frames 8 and 9. Zeros in the middle of an encoder's input do not give the silence
    # flag for a second or so (the Opus layer's dc_reject memory decays first), zeros at its start do: the decoder's stream is
    # eight frames of one encoder, then a second encoder's first eight, whose input starts with two frames of zeros.
    pcm = gm.synth_pcm("gmusic", 16, 13371337).copy()
    pcm[8:10] = 0
    pk, ln = encode_stream(pcm[:8], [None] * 8, 48000, enc_channels=1)
    pk2, ln2 = encode_stream(pcm[8:], [None] * 8, 48000, enc_channels=1)
    pk, ln = np.concatenate([pk, pk2]), np.concatenate([ln, ln2])
    assert (pk[:, 0] == 0xF8).all()
    assert (ln[8:10] == 3).all() and (ln[:8] > 3).all() and (ln[10:] > 3).all(), ln      # silence flag: TOC and two bytes
    cases["mono_input_stream"] = (pk, ln, 16)
    pk, ln = encode_stream(_pcm(["music", "gmusic", "noise", "edge"], 32, 200), SWITCH, 48000)
    cases["switch_stream"] = (pk, ln, 32)
    pks, lns = [], []
    for s, (settings, lost, dtx) in enumerate(SWITCH_LOSS):
        settings = list(settings)
        for f, toc in dtx:
            settings[f] = settings_of(toc)
        pk, ln = encode_stream(_pcm(["gmusic", "music"], 32, 300 + s), settings, 40000, cvbr=s)
        for f, toc in dtx:
            assert pk[f, 0] == toc
            ln[f] = 1
            pk[f, 1:] = 0
        ln[lost] = 0
        pk[lost] = 0
        pks.append(pk)
        lns.append(ln)
    cases["switch_loss_stream"] = (np.concatenate(pks), np.concatenate(lns), 32)
    # the encoder's own decisions (OPUS_AUTO) at rates below the GPU encoder's region
    pks, lns = [], []
    for kind, br, seed in (("gmusic", 24000, 400), ("noise", 16000, 401)):
        pk, ln, _rg = gm.ref_encode(gm._Cfg(2, br, 1, 1, 10, 16, 0, 1500), gm.synth_pcm(kind, 24, seed), 24)
        assert all(int(t) in TOCS for t in pk[:, 0]), [hex(t) for t in pk[:, 0]]
        assert (pk[:, 0] != 0xFC).any(), "%s %d: the encoder stayed in fullband stereo" % (kind, br)
        pks.append(pk)
        lns.append(ln.astype(np.int32))
    cases["auto_lowrate_stream"] = (np.concatenate(pks), np.concatenate(lns), 24)
    return cases


def is_loss_free(ln):
    return bool((ln > 1).all())


def chbw_vectors():
    out = {}
    for name, (pk, ln, fps) in chbw_cases().items():
        pk = np.ascontiguousarray(pk[:, :int(ln.max())])
        pcm, rng, ret = gm.ref_decode(pk, ln, fps)
        assert (ret == 960).all(), name
        assert (rng[ln <= 1] == 0).all() and (rng[ln > 1] != 0).all(), name
        out[name + "_packets"] = pk
        out[name + "_len"] = ln.astype(np.int32)
        out[name + "_fps"] = np.int32(fps)
        out[name + "_pcm"] = pcm
        out[name + "_rng"] = rng
        out[name + "_ret"] = ret
    return out


CASE_NAMES = ["static_%02x" % t for t in TOCS] + ["mono_input_stream", "switch_stream", "switch_loss_stream", "auto_lowrate_stream"]


def load_case(name):
    """packets, lengths, frames per stream, expected PCM / final range / return value of a stored case"""
    g = np.load(OUT)
    return (np.ascontiguousarray(g[name + "_packets"]), g[name + "_len"].astype(np.int32), int(g[name + "_fps"]), g[name + "_pcm"],
            g[name + "_rng"], g[name + "_ret"])


if __name__ == "__main__":
    if not reflib.available():
        sys.exit("oracle/_ref/libopus_ref.so missing: run `make -C oracle ref` where the reference exists")
    np.savez_compressed(OUT, **chbw_vectors())
    print("wrote chbw_golden.npz (%d bytes)" % os.path.getsize(OUT))
