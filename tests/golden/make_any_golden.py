"""Golden vectors of the decoder's short frames: CELT-only code-0 packets of 2.5, 5, 10 and 20 ms (TOC 0x80 | bw << 5 | fs << 3 |
stereo << 2), encoded by the compiled reference (opus_encoder_create(48000, 2, OPUS_APPLICATION_RESTRICTED_LOWDELAY) fed 120 << fs
samples per call, with OPUS_SET_FORCE_CHANNELS / OPUS_SET_BANDWIDTH before every frame and every TOC asserted), and the
reference's opus_decode(dec, data, len, pcm, 960, 0) on a (48000, 2) decoder: return value, the first `ret` sample pairs of PCM
(zero-padded to 960) and the final range. A packet of length 0 is lost: opus_decode(dec, NULL, 0, pcm, 960, 0).
Writes tests/golden/any_golden.npz.

    python tests/golden/make_any_golden.py        (needs oracle/_ref/libopus_ref.so)
"""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "any_golden.npz")
sys.path.insert(0, os.path.dirname(HERE))
import reflib  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_corrupt_golden", os.path.join(HERE, "make_corrupt_golden.py"))
mcg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mcg)
gm = mcg.gm

BANDWIDTH = [1101, 1103, 1104, 1105]                     # TOC bits 5-6 -> OPUS_BANDWIDTH_{NARROW,WIDE,SUPERWIDE,FULL}BAND
STATIC_TOCS = [0xE0, 0xE4, 0xE8, 0xEC, 0xF0, 0xF4]       # fullband, 2.5 / 5 / 10 ms, mono / stereo
NARROW_TOCS = [0x94, 0xA8, 0xC4]                         # NB 10 ms stereo, WB 5 ms mono, SWB 2.5 ms stereo
CASE_NAMES = ["static_%02x" % t for t in STATIC_TOCS + NARROW_TOCS] + ["fs_switch_stream", "fs_loss_stream", "fs_loss20_stream", "fs_corrupt"]
STRIDE = 400


def toc_lm(toc):
    return (toc >> 3) & 3


def toc_samples(toc):
    return 120 << toc_lm(toc)


def signal(nsamples, seed):
    """music and the edge signal in turn (2880 samples each), with a click every 331 samples in every other stretch of 1440: frames
    of every size meet clicks in their middle, which is what makes the encoder choose short blocks, and frames without any"""
    nfr = nsamples // 960 + 2
    a = gm.synth_pcm("music", nfr, seed).reshape(-1, 2).astype(np.int32)
    b = gm.synth_pcm("edge", nfr, seed).reshape(-1, 2).astype(np.int32)
    t = np.arange(a.shape[0])
    x = np.where(((t // 2880) % 2 == 0)[:, None], a, b // 2)
    x[((t % 331) == 200) & ((t // 1440) % 2 == 1)] += 20000
    x[(t % 1987) < 40] = 0
    return np.clip(x[:nsamples], -32768, 32767).astype(np.int16)


def _ref():
    ref = reflib.lib()
    ref.opus_encoder_create.restype = C.c_void_p
    ref.opus_decoder_create.restype = C.c_void_p
    ref.opus_encoder_ctl.restype = C.c_int
    ref.opus_encoder_ctl.argtypes = [C.c_void_p, C.c_int, C.c_int]
    ref.opus_decoder_ctl.restype = C.c_int
    ref.opus_decoder_ctl.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    ref.opus_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    ref.opus_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
    ref.opus_encoder_destroy.argtypes = [C.c_void_p]
    ref.opus_decoder_destroy.argtypes = [C.c_void_p]
    return ref


def encode_stream(pcm, tocs, bitrate, vbr=1, cvbr=0):
    """One stream through the reference encoder: pcm int16 [nsamples][2], consumed 120 << fs samples per packet; tocs: the TOC
    every packet is to have. Returns packets [n][STRIDE], lengths [n]."""
    ref = _ref()
    err = C.c_int(0)
    enc = C.c_void_p(ref.opus_encoder_create(48000, 2, 2051, C.byref(err)))
    assert err.value == 0 and enc
    for req, v in ((4002, bitrate), (4006, vbr), (4020, cvbr), (4010, 10), (4012, 0), (4016, 0), (4014, 0), (4036, 16)):
        assert ref.opus_encoder_ctl(enc, req, v) == 0, req
    out = np.zeros((len(tocs), STRIDE), np.uint8)
    lens = np.zeros(len(tocs), np.int32)
    pos = 0
    for f, toc in enumerate(tocs):
        fs = toc_samples(toc)
        assert ref.opus_encoder_ctl(enc, 4008, BANDWIDTH[(toc >> 5) & 3]) == 0
        assert ref.opus_encoder_ctl(enc, 4022, 2 if toc & 4 else 1) == 0
        fr = np.ascontiguousarray(pcm[pos:pos + fs])
        assert fr.shape[0] == fs
        pos += fs
        r = ref.opus_encode(enc, fr.ctypes.data_as(C.c_void_p), fs, out[f].ctypes.data_as(C.c_void_p), STRIDE)
        assert r > 2, (f, r)
        lens[f] = r
        assert out[f, 0] == toc, "packet %d: TOC 0x%02X, intended 0x%02X" % (f, out[f, 0], toc)
    ref.opus_encoder_destroy(enc)
    return out, lens


def ref_decode(pk, ln, fps):
    """opus_decode(dec, data, len, pcm, 960, 0) of every packet on (48000, 2) decoders, a fresh one every fps packets; length 0:
    data = NULL. Returns pcm [n][960][2] (zeros behind the first ret samples), final range [n], ret [n]."""
    ref = _ref()
    n = pk.shape[0]
    pcm = np.zeros((n, 960, 2), np.int16)
    rng = np.zeros(n, np.uint32)
    ret = np.zeros(n, np.int32)
    dec = None
    for f in range(n):
        if f % fps == 0:
            if dec:
                ref.opus_decoder_destroy(dec)
            err = C.c_int(0)
            dec = C.c_void_p(ref.opus_decoder_create(48000, 2, C.byref(err)))
            assert err.value == 0 and dec
        buf = np.zeros((960, 2), np.int16)
        data = np.ascontiguousarray(pk[f]).ctypes.data_as(C.c_void_p) if ln[f] > 0 else None
        ret[f] = ref.opus_decode(dec, data, int(ln[f]), buf.ctypes.data_as(C.c_void_p), 960, 0)
        if ret[f] > 0:
            pcm[f, :ret[f]] = buf[:ret[f]]
        r = C.c_uint32(0)
        assert ref.opus_decoder_ctl(dec, 4031, C.byref(r)) == 0
        rng[f] = r.value
    ref.opus_decoder_destroy(dec)
    return pcm, rng, ret


def _blocks(*per_block, each=4):
    s = []
    for b in per_block:
        s += [b] * each
    return s


STATIC_RATES = {0xE0: 96000, 0xE4: 128000, 0xE8: 64000, 0xEC: 96000, 0xF0: 48000, 0xF4: 64000, 0x94: 40000, 0xA8: 48000, 0xC4: 96000}
# frame size, channel count and bandwidth change between packets; 20 ms included
SWITCH = _blocks(0xFC, 0xF4, 0xEC, 0xE4, 0xE0, 0xF8, 0xA8, 0x94, each=2) + _blocks(0xC4, 0xF0, 0xFC, 0xE8, 0xB4, 0xEC, 0x9C, 0xE4, each=2)
# two streams of short packets with holes. Stream 0: the very first packet lost, a single loss right after a 2.5 ms packet (9),
# six in a row (16-21). Stream 1: a single loss after a 10 ms packet (5), six in a row after 5 ms packets (18-23).
LOSS = [
    (_blocks(0xE4, 0xE4, 0xE4, 0xEC, 0xEC, 0xEC, 0xF4, 0xE0), [0, 9] + list(range(16, 22))),
    (_blocks(0xF4, 0xF4, 0xEC, 0xEC, 0xEC, 0xEC, 0xE8, 0xF0), [5] + list(range(18, 24))),
]
# the losses the decoder conceals: right after 20 ms packets of a stream that otherwise changes its frame size -- a single one (5), six
# in a row (14-19: noise-based from the sixth), each followed by short packets
LOSS20 = (_blocks(0xE4, 0xFC, 0xEC, 0xFC, 0xFC, 0xF4, 0xE0, 0xFC, each=3) + _blocks(0xF4, 0xEC, each=4), [5, 14, 15, 16, 17, 18, 19])


def any_cases():
    """name -> (packets [n][STRIDE], lengths [n] (0: lost), packets per stream)"""
    cases = {}
    for toc in STATIC_TOCS + NARROW_TOCS:
        n = 16 if toc_lm(toc) < 2 else 8
        pk, ln = encode_stream(signal(n * toc_samples(toc), 500 + toc), [toc] * n, STATIC_RATES[toc], cvbr=int(toc & 0x08 != 0))
        cases["static_%02x" % toc] = (pk, ln, n)
    pk, ln = encode_stream(signal(32 * 960, 600), SWITCH, 64000)
    cases["fs_switch_stream"] = (pk, ln, 32)
    pks, lns = [], []
    for s, (tocs, lost) in enumerate(LOSS):
        pk, ln = encode_stream(signal(32 * 960, 700 + s), tocs, 96000, cvbr=s)
        ln[lost] = 0
        pk[lost] = 0
        pks.append(pk)
        lns.append(ln)
    cases["fs_loss_stream"] = (np.concatenate(pks), np.concatenate(lns), 32)
    tocs, lost = LOSS20
    assert all(tocs[f - 1] & 0x18 == 0x18 for f in lost if f - 1 not in lost)
    pk, ln = encode_stream(signal(32 * 960, 750), tocs, 96000)
    ln[lost] = 0
    pk[lost] = 0
    cases["fs_loss20_stream"] = (pk, ln, 32)
    # corrupt packets behind short-frame TOCs, each followed by a good packet of the same stream: random bytes, a truncated
    # packet, a 3-byte packet, and the silence flag (a payload of 0xFF bytes) at every LM
    rs = np.random.default_rng(9200)
    tocs = _blocks(0xE4, 0xEC, 0xF4, 0xE0, each=6)
    pk, ln = encode_stream(signal(24 * 480, 800), tocs, 96000)
    for k, base in enumerate(range(0, 24, 6)):
        toc = tocs[base]
        nrand = [9, 23, 60, 17][k]
        mcg._set_payload(pk, ln, base + 1, toc, rs.integers(0, 256, nrand, dtype=np.uint8))      # random bytes
        ln[base + 2] = max(4, int(ln[base + 2]) // 2)                                           # truncated
        pk[base + 2, ln[base + 2]:] = 0
        mcg._set_payload(pk, ln, base + 3, toc, rs.integers(0, 256, 2, dtype=np.uint8))         # 3-byte packet
        mcg._set_payload(pk, ln, base + 4, toc, np.full(6 + k, 0xFF, np.uint8))                 # silence flag, longer than it needs
    cases["fs_corrupt"] = (pk, ln, 24)
    return cases


def any_vectors():
    out = {}
    for name, (pk, ln, fps) in any_cases().items():
        pk = np.ascontiguousarray(pk[:, :int(ln.max())])
        pcm, rng, ret = ref_decode(pk, ln, fps)
        got = ln > 0
        want = np.array([toc_samples(int(t)) for t in pk[:, 0]])
        assert (ret[got] == want[got]).all(), (name, ret[got], want[got])
        assert (ret[~got] == 960).all(), name
        assert (rng[~got] == 0).all(), name
        out[name + "_packets"] = pk
        out[name + "_len"] = ln.astype(np.int32)
        out[name + "_fps"] = np.int32(fps)
        out[name + "_pcm"] = pcm
        out[name + "_rng"] = rng
        out[name + "_ret"] = ret
    return out


def load_case(name):
    """packets, lengths, packets per stream, expected PCM (zeros behind ret samples) / final range / return value"""
    g = np.load(OUT)
    return (np.ascontiguousarray(g[name + "_packets"]), g[name + "_len"].astype(np.int32), int(g[name + "_fps"]), g[name + "_pcm"],
            g[name + "_rng"], g[name + "_ret"])


if __name__ == "__main__":
    if not reflib.available():
        sys.exit("oracle/_ref/libopus_ref.so missing: run `make -C oracle ref` where the reference exists")
    mcg._savez_deterministic(OUT, any_vectors())
    print("wrote any_golden.npz (%d bytes)" % os.path.getsize(OUT))
