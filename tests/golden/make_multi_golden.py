"""Golden vectors of the decoder's packet layer: CELT-only packets with frame-count codes 1, 2 and 3, padding and DTX frames, as the
compiled reference makes them (opus_encode given 40 / 60 ms per call, opus_repacketizer_*, opus_packet_pad) or assembled by hand from
its code-0 packets where only the byte layout matters (DTX frames, malformed packets), and the reference's
opus_decode(dec, data, len, pcm, frame_size, 0) on a (48000, 2) decoder: return value, final range, and the PCM of the returned
samples, concatenated. A packet of length 0 is lost: opus_decode(dec, NULL, 0, pcm, 960, 0).
Writes tests/golden/multi_golden.npz.

    python tests/golden/make_multi_golden.py        (needs oracle/_ref/libopus_ref.so)
"""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "multi_golden.npz")
sys.path.insert(0, os.path.dirname(HERE))
import reflib  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_any_golden", os.path.join(HERE, "make_any_golden.py"))
mag = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mag)

INVALID, TOO_SMALL = -4, -2
CASE_NAMES = ["enc_40ms", "enc_60ms", "rp_code1", "rp_code2", "rp_code3_vbr", "rp_code3_cbr", "rp_6x20", "padded", "dtx_frames", "dtx_code0",
              "dtx_six", "loss_after_multi", "malformed", "too_small"]


def _ref():
    ref = mag._ref()
    ref.opus_repacketizer_create.restype = C.c_void_p
    ref.opus_repacketizer_init.restype = C.c_void_p
    ref.opus_repacketizer_init.argtypes = [C.c_void_p]
    ref.opus_repacketizer_cat.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    ref.opus_repacketizer_out.restype = C.c_int32
    ref.opus_repacketizer_out.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    ref.opus_repacketizer_destroy.argtypes = [C.c_void_p]
    ref.opus_packet_pad.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    ref.opus_packet_parse.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return ref


def ref_parse(data):
    """opus_packet_parse of bytes: (count or error, toc, sizes [count], frame offsets [count])"""
    ref = _ref()
    buf = (C.c_ubyte * max(1, len(data))).from_buffer_copy(bytes(data) or b"\0")
    toc = C.c_ubyte(0)
    frames = (C.c_void_p * 48)()
    size = (C.c_int16 * 48)()
    off = C.c_int(0)
    n = ref.opus_packet_parse(buf, len(data), C.byref(toc), frames, size, C.byref(off))
    if n < 0:
        return n, None, [], []
    base = C.addressof(buf)
    return n, toc.value, [size[i] for i in range(n)], [frames[i] - base for i in range(n)]


def frames_of(toc, n, bitrate, seed, vbr=1):
    """n code-0 packets of one TOC from the reference encoder, as bytes"""
    pk, ln = mag.encode_stream(mag.signal(n * mag.toc_samples(toc), seed), [toc] * n, bitrate, vbr=vbr)
    return [bytes(pk[i, :ln[i]]) for i in range(n)]


def repacketize(packets):
    """opus_repacketizer_cat of every packet, opus_repacketizer_out"""
    ref = _ref()
    rp = C.c_void_p(ref.opus_repacketizer_create())
    keep = [(C.c_ubyte * len(p)).from_buffer_copy(p) for p in packets]
    for b in keep:
        assert ref.opus_repacketizer_cat(rp, b, len(b)) == 0
    out = (C.c_ubyte * 8192)()
    n = ref.opus_repacketizer_out(rp, out, 8192)
    assert n > 0, n
    ref.opus_repacketizer_destroy(rp)
    return bytes(out[:n])


def pad(packet, extra):
    ref = _ref()
    buf = (C.c_ubyte * (len(packet) + extra)).from_buffer_copy(packet + bytes(extra))
    assert ref.opus_packet_pad(buf, len(packet), len(packet) + extra) == 0
    return bytes(buf)


def size_bytes(n):
    """the one- or two-byte frame length (src/opus.c: encode_size)"""
    return bytes([n]) if n < 252 else bytes([252 + (n & 3), (n - (252 + (n & 3))) >> 2])


def code2(toc, a, b):
    return bytes([toc | 2]) + size_bytes(len(a)) + a + b


def code3_vbr(toc, frames, padding=None):
    """VBR code 3; padding: the number of padding bytes behind the frames (its own length bytes not counted), or None"""
    head = bytes([toc | 3, 0x80 | (0x40 if padding is not None else 0) | len(frames)])
    if padding is not None:
        p = padding
        while p >= 255:
            head += b"\xff"
            p -= 254
        head += bytes([p])
    return head + b"".join(size_bytes(len(f)) for f in frames[:-1]) + b"".join(frames) + bytes(padding or 0)


def payload(p):
    return p[1:]


def ref_decode(stream):
    """stream: [(bytes, frame_size)] through one fresh decoder -> [(ret, final range, pcm [max(ret, 0)][2])]"""
    ref = _ref()
    err = C.c_int(0)
    dec = C.c_void_p(ref.opus_decoder_create(48000, 2, C.byref(err)))
    assert err.value == 0 and dec
    out = []
    for data, frame_size in stream:
        buf = np.zeros((5760, 2), np.int16)
        b = (C.c_ubyte * len(data)).from_buffer_copy(data) if data else None
        ret = ref.opus_decode(dec, b, len(data), buf.ctypes.data_as(C.c_void_p), frame_size, 0)
        r = C.c_uint32(0)
        assert ref.opus_decoder_ctl(dec, 4031, C.byref(r)) == 0
        out.append((ret, r.value, buf[:max(ret, 0)].copy()))
    ref.opus_decoder_destroy(dec)
    return out


def multi_cases():
    """name -> (streams: [[(bytes, frame_size)]] all of one length, want: [[check]] where check(ret, rng, parse) asserts what the
    packet is meant to provoke in the reference)"""
    cases = {}

    def good(count, fs, code=None, rng0=False):
        def check(ret, rng, data):
            assert ret == count * fs, (ret, count, fs)
            n, toc, _sizes, _offs = ref_parse(data)
            assert n == count and (code is None or toc & 3 == code), (n, toc, code)
            assert (rng == 0) == rng0, rng
        return check

    def bad(err):
        def check(ret, rng, data):
            assert ret == err, (ret, err)
            if err == INVALID:
                assert ref_parse(data)[0] == INVALID
        return check

    def lost(ret, rng, data):
        assert ret == 960 and rng == 0

    FS = 5760
    # the encoder itself, fed 40 and 60 ms per call (RESTRICTED_LOWDELAY, 20 ms frames inside)
    ref = _ref()
    for name, per_call, count, seed in (("enc_40ms", 1920, 2, 901), ("enc_60ms", 2880, 3, 902)):
        err = C.c_int(0)
        enc = C.c_void_p(ref.opus_encoder_create(48000, 2, 2051, C.byref(err)))
        assert err.value == 0 and enc
        for req, v in ((4002, 64000), (4006, 1), (4020, 0), (4010, 10), (4012, 0), (4016, 0), (4014, 0), (4036, 16)):
            assert ref.opus_encoder_ctl(enc, req, v) == 0, req
        pcm = mag.signal(3 * per_call, seed)
        stream, checks = [], []
        for f in range(3):
            fr = np.ascontiguousarray(pcm[f * per_call:(f + 1) * per_call])
            out = np.zeros(4000, np.uint8)
            r = ref.opus_encode(enc, fr.ctypes.data_as(C.c_void_p), per_call, out.ctypes.data_as(C.c_void_p), 4000)
            assert r > 0, r
            data = bytes(out[:r])
            # what the reference's encoder produced (VBR): 40 ms is code 2 (0xFE), 60 ms code 3 with count byte 0x83 (0xFF, VBR, 3 frames)
            assert data[0] == (0xFF if count == 3 else 0xFE) and (count != 3 or data[1] == 0x83), (hex(data[0]), hex(data[1]))
            stream.append((data, FS))
            checks.append(good(count, 960))
        ref.opus_encoder_destroy(enc)
        cases[name] = ([stream], [checks])

    # repacketized from code-0 packets of one TOC
    fr = frames_of(0xFC, 6, 64000, 910, vbr=0)
    assert len({len(f) for f in fr}) == 1
    cases["rp_code1"] = ([[(repacketize(fr[0:2]), FS), (repacketize(fr[2:4]), FS), (repacketize(fr[4:6]), FS)]], [[good(2, 960, 1)] * 3])
    fr = frames_of(0xFC, 8, 112000, 911)
    # two pairs of neighbours that differ in size, the FIRST of each (the coded length) of at least 252 bytes
    pairs = [i for i in range(7) if len(fr[i]) != len(fr[i + 1]) and len(payload(fr[i])) >= 252]
    pairs = [pairs[0]] + [i for i in pairs if i > pairs[0] + 1][:1]
    assert len(pairs) == 2, [len(f) for f in fr]
    p2 = [repacketize(fr[i:i + 2]) for i in pairs]
    assert all(p[1] >= 252 for p in p2)
    cases["rp_code2"] = ([[(p2[0], FS), (p2[1], FS)]], [[good(2, 960, 2)] * 2])
    streams, checks = [], []
    for toc, count, rate, seed in ((0xF4, 3, 64000, 920), (0xE8, 8, 48000, 921), (0xE4, 48, 96000, 922), (0x94, 3, 40000, 923)):
        fr = frames_of(toc, 2 * count, rate, seed)
        assert len({len(f) for f in fr[:count]}) > 1
        streams.append([(repacketize(fr[:count]), FS), (repacketize(fr[count:]), FS)])
        checks.append([good(count, mag.toc_samples(toc), 3)] * 2)
        assert streams[-1][0][0][1] & 0x80                                                    # VBR
    cases["rp_code3_vbr"] = (streams, checks)
    streams, checks = [], []
    for toc, count, rate, seed in ((0x94, 3, 40000, 930), (0xC4, 8, 96000, 931), (0xE0, 48, 96000, 932), (0xEC, 8, 64000, 933)):
        fr = frames_of(toc, 2 * count, rate, seed, vbr=0)
        assert len({len(f) for f in fr}) == 1
        streams.append([(repacketize(fr[:count]), FS), (repacketize(fr[count:]), FS)])
        checks.append([good(count, mag.toc_samples(toc), 3)] * 2)
        assert not streams[-1][0][0][1] & 0x80                                                # CBR
    cases["rp_code3_cbr"] = (streams, checks)
    fr = frames_of(0xFC, 7, 48000, 940)
    cases["rp_6x20"] = ([[(repacketize(fr[:6]), FS), (fr[6], FS)]], [[good(6, 960, 3), good(1, 960, 0)]])

    # padded with opus_packet_pad: a code-0 packet (by at most 254 bytes), a code-1 packet (by more, so that the length chains), a
    # code-3 packet; and a padded packet whose every frame is DTX
    fr = frames_of(0xFC, 5, 48000, 950, vbr=0)
    sh = frames_of(0xEC, 5, 64000, 951)
    p0, p1, p3 = pad(fr[0], 100), pad(repacketize(fr[1:3]), 300), pad(repacketize(sh[0:4]), 9)
    assert p0[1] & 0x40 and p0[2] == 98 and p1[1] & 0x40 and p1[2] == 255 and p3[1] & 0x40, (p0[:3], p1[:4])
    alldtx = code3_vbr(0xEC, [b"", b"\x55", b""], padding=7)
    cases["padded"] = ([[(p0, FS), (p1, FS), (p3, FS), (alldtx, FS), (sh[4], FS)]],
                       [[good(1, 960, 3), good(2, 960, 3), good(4, 240, 3), good(3, 240, 3, rng0=True), good(1, 240, 0)]])

    # DTX frames (no or one payload byte) between real ones, first and last place included, at every frame size; the stream's very
    # first frame is one (zeros)
    streams, checks = [], []
    for toc, rate, seed in ((0xE4, 96000, 960), (0xEC, 64000, 961), (0xF0, 64000, 962), (0xFC, 48000, 963)):
        f = [payload(p) for p in frames_of(toc, 6, rate, seed)]
        N = mag.toc_samples(toc)
        streams.append([(code2(toc, b"", f[0]), FS), (code3_vbr(toc, [f[1], b"", b"\xAA", f[2]]), FS),
                        (code3_vbr(toc, [b"\x01", f[3], b""]), FS), (code2(toc, f[4], b"\x7F"), FS), (bytes([toc]) + f[5], FS)])
        checks.append([good(2, N, 2), good(4, N, 3), good(3, N, 3, rng0=True), good(2, N, 2, rng0=True), good(1, N, 0)])
    cases["dtx_frames"] = (streams, checks)
    # one- and two-byte code-0 packets under short-frame TOCs: before any packet (zeros), after history, changing the frame size
    a, b, c = frames_of(0xE4, 2, 96000, 970), frames_of(0xF4, 2, 64000, 971), frames_of(0xE0, 1, 96000, 972)
    stream = [(b"\xE4", FS), (a[0], FS), (b"\xE4\x33", FS), (b"\xEC", FS), (a[1], FS), (b[0], FS), (b"\xF4", FS), (b"\xE0\x00", FS),
              (c[0], FS), (b"\xC8", FS), (b[1], FS)]
    want = [120, 120, 120, 240, 120, 480, 480, 120, 120, 240, 480]
    cases["dtx_code0"] = ([stream], [[good(1, w, 0, rng0=len(p) <= 2) for (p, _fs), w in zip(stream, want)]])
    # six DTX frames in a row (the sixth is concealed from noise): 5 ms frames inside one packet, and 20 ms frames
    f5, f20 = [payload(p) for p in frames_of(0xEC, 3, 64000, 980)], frames_of(0xFC, 2, 48000, 981)
    cases["dtx_six"] = ([[(code3_vbr(0xEC, [f5[0], f5[1]] + [b""] * 6), FS), (bytes([0xEC]) + f5[2], FS)],
                         [(f20[0], FS), (code3_vbr(0xFC, [b""] * 6), FS)]],
                        [[good(8, 240, 3, rng0=True), good(1, 240, 0)], [good(1, 960, 0), good(6, 960, 3, rng0=True)]])

    # a lost packet after multi-frame packets of short frames: concealed for 960 samples in steps of the frame size
    fr = frames_of(0xEC, 16, 64000, 990)
    cases["loss_after_multi"] = ([[(repacketize(fr[0:8]), FS), (b"", 960), (repacketize(fr[8:16]), FS), (b"", 960), (b"", 960)]],
                                 [[good(8, 240, 3), lost, good(8, 240, 3), lost, lost]])

    # malformed packets, each followed by a good packet of the same stream
    g = frames_of(0xFC, 10, 48000, 1000)
    f = [payload(p) for p in frames_of(0xF4, 4, 64000, 1001)]
    malformed = [
        bytes([0xFD]) + f[0][:21],                                            # code 1, odd payload
        bytes([0xFE, 200]) + f[0][:50],                                       # code 2, size[0] past the end
        bytes([0xFE, 252]),                                                   # code 2, the two-byte length cut off
        bytes([0xFF]),                                                        # code 3 of one byte
        bytes([0xFF, 0x80]) + f[0],                                           # code 3, count 0
        bytes([0xFF, 0x80 | 7]) + bytes(6) + f[0],                            # code 3, 7 * 960 > 5760
        bytes([0xF7, 0x40 | 2, 255, 255, 10]) + f[0] + f[0],                  # padding longer than the packet
        bytes([0xF7, 3]) + f[0][:31],                                         # CBR payload not divisible by the count
        bytes([0xF7, 0x80 | 3, 20, 200]) + f[0][:60],                         # VBR sizes overrunning
        bytes([0xFC]) + bytes(range(256)) * 4 + bytes(252),                   # a last frame of 1276 bytes
    ]
    assert len(malformed[-1]) == 1277
    stream, checks = [], []
    for k, m in enumerate(malformed):
        stream += [(m, FS), (g[k], FS)]
        checks += [bad(INVALID), good(1, 960, 0)]
    cases["malformed"] = ([stream], [checks])

    # opus_decode's frame_size too small for the packet: refused whole, and the next packet decodes
    fr = frames_of(0xFC, 4, 48000, 1010)
    cases["too_small"] = ([[(repacketize(fr[0:3]), 1920), (fr[3], 960), (repacketize(fr[0:2]), 1920)]],
                          [[bad(TOO_SMALL), good(1, 960, 0), good(2, 960)]])
    assert list(cases) == CASE_NAMES
    return cases


def multi_vectors():
    out = {}
    for name, (streams, checks) in multi_cases().items():
        fps = len(streams[0])
        assert all(len(s) == fps for s in streams)
        flat = [p for s in streams for p in s]
        stride = max(4, max(len(d) for d, _fs in flat) + 3 & ~3)
        pk = np.zeros((len(flat), stride), np.uint8)
        ln = np.zeros(len(flat), np.int32)
        fsz = np.zeros(len(flat), np.int32)
        ret = np.zeros(len(flat), np.int32)
        rng = np.zeros(len(flat), np.uint32)
        pcm = []
        for s, stream in enumerate(streams):
            for f, ((data, frame_size), (r, g, x)) in enumerate(zip(stream, ref_decode(stream))):
                k = s * fps + f
                checks[s][f](r, g, data)
                pk[k, :len(data)] = np.frombuffer(data, np.uint8)
                ln[k], fsz[k], ret[k], rng[k] = len(data), frame_size, r, g
                pcm.append(x)
        out[name + "_packets"] = pk
        out[name + "_len"] = ln
        out[name + "_frame_size"] = fsz
        out[name + "_fps"] = np.int32(fps)
        out[name + "_ret"] = ret
        out[name + "_rng"] = rng
        out[name + "_pcm"] = np.concatenate(pcm)
    return out


def load_case(name):
    """packets [n][stride], lengths [n], frame_size [n], packets per stream, expected ret [n], final range [n], PCM (the returned
    samples of all packets, concatenated) [sum(max(ret, 0))][2]"""
    g = np.load(OUT)
    return (np.ascontiguousarray(g[name + "_packets"]), g[name + "_len"].astype(np.int32), g[name + "_frame_size"].astype(np.int32),
            int(g[name + "_fps"]), g[name + "_ret"], g[name + "_rng"], g[name + "_pcm"])


if __name__ == "__main__":
    if not reflib.available():
        sys.exit("oracle/_ref/libopus_ref.so missing: run `make -C oracle ref` where the reference exists")
    mag.mcg._savez_deterministic(OUT, multi_vectors())
    size = os.path.getsize(OUT)
    assert size <= max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz") and f != "multi_golden.npz")
    print("wrote multi_golden.npz (%d bytes)" % size)
