"""Golden vectors of the decoder on CORRUPT and TRUNCATED packets: valid CELT-only 20 ms packets of the committed fixtures
(chbw_golden.npz: switch_stream, auto_lowrate_stream, static_fc, static_98; decode_golden.npz: dec_music_32k_stream) with bits
flipped, bytes cut off, bytes appended or the whole payload replaced, always behind one of the eight accepted TOCs, and the
compiled reference's opus_decode() output on a (48000, 2) decoder per stream: PCM, final range, return value. The mutations come
from seeded numpy generators, so the packets need no reference; the expected outputs do. Writes tests/golden/corrupt_golden.npz.

    python tests/golden/make_corrupt_golden.py        (needs oracle/_ref/libopus_ref.so and librefdrv.so)

Streams of 16 frames, stride 1280; the first two frames of every stream are valid (history). Per case, stored next to the
packets: <case>_corrupt, 1 where the packet was mutated (a loss or a DTX packet is not "corrupt").
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "corrupt_golden.npz")
sys.path.insert(0, os.path.dirname(HERE))
import reflib  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
gm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gm)

TOCS = [0x98, 0xB8, 0xD8, 0xF8, 0x9C, 0xBC, 0xDC, 0xFC]
FPS, STRIDE = 16, 1280
MAX_FRAMES = 320
CASE_NAMES = ["flip1", "flip_many", "truncate", "extend", "random", "const", "corrupt_then_lost", "switch_corrupt"]
RANDOM_LENGTHS = [2, 3, 4, 8, 16, 64, 160, 400, 1276]
INVALID_PACKET = -4


def _sources():
    """name -> list of streams (packets [n][1280], lengths [n]) of the committed valid fixtures"""
    src = {}
    g = np.load(os.path.join(HERE, "chbw_golden.npz"))
    for name in ("switch_stream", "auto_lowrate_stream", "static_fc", "static_98"):
        pk, ln, fps = g[name + "_packets"], g[name + "_len"].astype(np.int32), int(g[name + "_fps"])
        pk = np.pad(pk, ((0, 0), (0, STRIDE - pk.shape[1])))
        src[name] = [(pk[s:s + fps], ln[s:s + fps]) for s in range(0, len(ln), fps)]
    g = np.load(os.path.join(HERE, "decode_golden.npz"))
    pk, ln = g["dec_music_32k_stream_packets"], g["dec_music_32k_stream_len"].astype(np.int32)
    pk = np.pad(pk, ((0, 0), (0, STRIDE - pk.shape[1])))
    src["dec_music_32k_stream"] = [(pk[s:s + 16], ln[s:s + 16]) for s in range(0, len(ln), 16)]
    return src


def _take(stream, start=0, n=FPS):
    """n frames of a valid stream from frame `start` on, around its end if it is shorter"""
    pk, ln = stream
    idx = (start + np.arange(n)) % len(ln)
    return pk[idx].copy(), ln[idx].copy()


def _flip(rs, pk, ln, f, nbits):
    """nbits distinct random payload bits of packet f flipped (byte 0, the TOC, stays)"""
    nb = (int(ln[f]) - 1) * 8
    for b in rs.choice(nb, size=min(nbits, nb), replace=False):
        pk[f, 1 + b // 8] ^= 1 << (b % 8)


def _set_payload(pk, ln, f, toc, payload):
    pk[f] = 0
    pk[f, 0] = toc
    pk[f, 1:1 + len(payload)] = payload
    ln[f] = 1 + len(payload)


def corrupt_cases():
    """name -> (packets [n][1280], lengths [n] (0: lost, 1: one-byte DTX packet), corrupt [n], frames per stream)"""
    src = _sources()
    cases = {}

    def put(name, streams):
        pk = np.concatenate([s[0] for s in streams])
        ln = np.concatenate([s[1] for s in streams]).astype(np.int32)
        co = np.concatenate([s[2] for s in streams]).astype(np.uint8)
        for f in range(len(ln)):
            pk[f, max(int(ln[f]), 0):] = 0
        assert all(int(t) in TOCS for t in pk[ln > 0, 0]) and (ln <= STRIDE).all()
        assert not co.reshape(-1, FPS)[:, :2].any(), "the first two frames of a stream stay valid"
        cases[name] = (pk, ln, co, FPS)

    # flip1: one payload bit of every packet from frame 2 on
    rs = np.random.default_rng(9101)
    streams = []
    for stream in (src["dec_music_32k_stream"][0], _take(src["switch_stream"][0], 0)):
        pk, ln = _take(stream)
        co = np.zeros(FPS, bool)
        for f in range(2, FPS):
            _flip(rs, pk, ln, f, 1)
            co[f] = True
        streams.append((pk, ln, co))
    put("flip1", streams)

    # flip_many: about 1 % of the payload bits
    rs = np.random.default_rng(9102)
    streams = []
    for stream in (src["dec_music_32k_stream"][1], src["auto_lowrate_stream"][0]):
        pk, ln = _take(stream)
        co = np.zeros(FPS, bool)
        for f in range(2, FPS):
            _flip(rs, pk, ln, f, max(1, (int(ln[f]) - 1) * 8 // 100))
            co[f] = True
        streams.append((pk, ln, co))
    put("flip_many", streams)

    # truncate: a random shorter length, three packets forced to 2, 3 and 4 bytes. Stream 1 keeps every payload above one byte
    # (a payload of one byte is DTX), so that it can go through the entry points without concealment
    rs = np.random.default_rng(9103)
    streams = []
    for s, stream in enumerate((src["static_fc"][0], _take(src["switch_stream"][0], 16))):
        pk, ln = _take(stream)
        co = np.zeros(FPS, bool)
        for f in range(2, FPS):
            ln[f] = int(rs.integers(2 if s == 0 else 3, int(ln[f])))
            co[f] = True
        for f, n in ((4, 2), (7, 3), (11, 4)) if s == 0 else ((5, 3), (9, 4)):
            ln[f] = n
        streams.append((pk, ln, co))
    put("truncate", streams)

    # extend: random bytes appended; one packet of exactly 1276 bytes, one of 1277 (the only OPUS_INVALID_PACKET of the corpus)
    rs = np.random.default_rng(9104)
    streams = []
    for s, stream in enumerate((_take(src["auto_lowrate_stream"][1], 0), src["static_98"][0])):
        pk, ln = _take(stream)
        co = np.zeros(FPS, bool)
        for f in range(2, FPS, 2):                                  # every second packet: valid ones follow the long ones
            n = min(1276, int(ln[f]) + int(rs.integers(1, 600)))
            if f == 6:
                n = 1276 if s == 0 else 1277
            pk[f, ln[f]:n] = rs.integers(0, 256, n - int(ln[f]), dtype=np.uint8)
            ln[f] = n
            co[f] = True
        streams.append((pk, ln, co))
    put("extend", streams)

    # random: uniform payloads, the lengths and the eight TOCs in turn
    rs = np.random.default_rng(9105)
    streams = []
    k = 0
    for stream in (src["dec_music_32k_stream"][0], _take(src["switch_stream"][0], 8)):
        pk, ln = _take(stream)
        co = np.zeros(FPS, bool)
        for f in range(2, FPS):
            n = RANDOM_LENGTHS[k % len(RANDOM_LENGTHS)]
            _set_payload(pk, ln, f, TOCS[k % 8], rs.integers(0, 256, n - 1, dtype=np.uint8))
            co[f] = True
            k += 1
        streams.append((pk, ln, co))
    put("random", streams)

    # const: all-0x00, all-0xFF, all-0x80 payloads at 2, 40 and 1276 bytes under 0x98, 0xF8 and 0xFC: 27 packets. The nine of two
    # bytes (DTX) are all in stream 0
    combos = [(n, toc, v) for n in (2, 40, 1276) for toc in (0x98, 0xF8, 0xFC) for v in (0x00, 0xFF, 0x80)]
    order = [c for c in combos if c[0] == 2] + [c for c in combos if c[0] != 2]
    streams = []
    for s, stream in enumerate((src["static_fc"][0], src["dec_music_32k_stream"][1])):
        pk, ln = _take(stream)
        co = np.zeros(FPS, bool)
        for f in range(2, FPS):
            i = s * (FPS - 2) + f - 2
            if i >= len(order):
                break
            n, toc, v = order[i]
            _set_payload(pk, ln, f, toc, np.full(n - 1, v, np.uint8))
            co[f] = True
        streams.append((pk, ln, co))
    put("const", streams)

    # corrupt_then_lost: corrupt / lost / valid; corrupt / one-byte DTX; corrupt, then seven losses (noise from the sixth on)
    rs = np.random.default_rng(9107)
    streams = []
    for s, stream in enumerate((src["dec_music_32k_stream"][0], src["auto_lowrate_stream"][0])):
        pk, ln = _take(stream)
        co = np.zeros(FPS, bool)
        for f in (2, 5, 8):
            if s == 0:
                _flip(rs, pk, ln, f, max(1, (int(ln[f]) - 1) * 8 // 50))
            else:
                _set_payload(pk, ln, f, int(pk[f, 0]), rs.integers(0, 256, int(ln[f]) - 1, dtype=np.uint8))
            co[f] = True
        ln[3] = 0
        ln[6] = 1
        ln[9:16] = 0
        streams.append((pk, ln, co))
    put("corrupt_then_lost", streams)

    # switch_corrupt: every third packet of switch_stream, so that channel count and bandwidth change on corrupt frames
    rs = np.random.default_rng(9108)
    streams = []
    for start in (0, 16):
        pk, ln = _take(src["switch_stream"][0], start)
        co = np.zeros(FPS, bool)
        for f in range(2, FPS, 3):
            _flip(rs, pk, ln, f, max(1, (int(ln[f]) - 1) * 8 // 100))
            co[f] = True
        streams.append((pk, ln, co))
    put("switch_corrupt", streams)
    assert list(cases) == CASE_NAMES
    return cases


def is_loss_free(ln):
    """every packet has a payload of two bytes or more: nothing for the concealment (0: lost, 1 and 2: DTX)"""
    return bool((ln > 2).all())


def corrupt_vectors():
    out = {}
    total = odd = 0
    for name, (pk, ln, co, fps) in corrupt_cases().items():
        pcm, rng, ret = gm.ref_decode(pk, ln, fps)
        # what the reference did is part of the expectation: 960 everywhere but on the 1277-byte packets
        expect = np.where(ln == 1277, INVALID_PACKET, 960)
        odd += int((ret != expect).sum())
        total += len(ln)
        assert (ret[ln == 1277] == INVALID_PACKET).all(), (name, ret[ln == 1277])
        pcm[ret < 0] = 0                                   # (the reference leaves its output buffer alone there: not compared)
        out[name + "_packets"] = pk
        out[name + "_len"] = ln.astype(np.int32)
        out[name + "_corrupt"] = co
        out[name + "_fps"] = np.int32(fps)
        out[name + "_pcm"] = pcm
        out[name + "_rng"] = rng
        out[name + "_ret"] = ret
    assert total <= MAX_FRAMES, total
    assert odd * 20 <= total, "%d of %d frames with a return value other than 960 / -4: choose other seeds" % (odd, total)
    return out


def load_case(name):
    """packets, lengths, frames per stream, expected PCM / final range / return value, corrupt mask of a stored case"""
    g = np.load(OUT)
    return (np.ascontiguousarray(g[name + "_packets"]), g[name + "_len"].astype(np.int32), int(g[name + "_fps"]), g[name + "_pcm"],
            g[name + "_rng"], g[name + "_ret"], g[name + "_corrupt"].astype(bool))


def _savez_deterministic(path, arrays):
    """np.savez_compressed with fixed member timestamps, so that the same arrays give the same file"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


if __name__ == "__main__":
    if not reflib.available():
        sys.exit("oracle/_ref/libopus_ref.so missing: run `make -C oracle ref` where the reference exists")
    _savez_deterministic(OUT, corrupt_vectors())
    print("wrote corrupt_golden.npz (%d bytes)" % os.path.getsize(OUT))
