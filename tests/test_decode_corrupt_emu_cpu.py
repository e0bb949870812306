"""CPU tier of the decoder on CORRUPT and TRUNCATED packets: the decoder sources compiled for the host (tests/emu/celt_plc_emu.cpp,
the wave-per-stream build with concealment; tests/emu/celt_lane_emu.cpp, the lane build) against the compiled reference's
opus_decode() on the same bytes (tests/golden/corrupt_golden.npz, made by tests/golden/make_corrupt_golden.py; live where
oracle/_ref is present): return value, final range and PCM equal on EVERY frame, the valid, lost and DTX frames after a corrupt
one included. A frame the reference rejects (the 1277-byte packets: OPUS_INVALID_PACKET) is compared by return value and final
range -- the reference leaves its output buffer alone there -- and must leave the stream's state as it was.

Branch counters (CA_COUNT "corrupt_*" in celt_dec.h / celt_plc.h), read per frame, prove that the corpus's corrupt frames reach:
dec.error, the silence flag in front of a long payload, post-filter octave 5, the header running out of bits before intra_ener /
the spread decision / the trim, anti-collapse, a payload of one byte (DTX), and the concealment's explosion guards right after a
corrupt frame. NOT reached by this corpus, and not asserted: the ec_tell(dec) > 8 * len exit of celt_decode_front_as
("corrupt_tell_past_end" stays 0; every reader checks its budget first, so it may be unreachable).

The same packets go through a stand-alone AddressSanitizer + UBSan build of the emulation (tests/emu/decode_corpus_main.cpp), run
as a child process; nothing instrumented is loaded into this interpreter."""
import ctypes as C
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import emulib
import plc_emulib
from test_decode_chbw_emu_cpu import assert_frames_equal as _assert_all_equal
from test_decode_chbw_emu_cpu import mcg, random_settings_streams
from test_plc_emu_cpu import random_loss_mask

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HAVE_REF = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "librefdrv.so"))

_spec = importlib.util.spec_from_file_location("make_corrupt_golden", os.path.join(HERE, "golden", "make_corrupt_golden.py"))
mco = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mco)

p = lambda a: a.ctypes.data_as(C.c_void_p)
NEW_COUNTERS = ("corrupt_dec_error", "corrupt_silence_long", "corrupt_pf_octave5", "corrupt_intra_skipped", "corrupt_spread_skipped",
                "corrupt_trim_default", "corrupt_anti_collapse", "corrupt_payload_one_byte", "corrupt_tell_past_end")
EXPLOSION = ("plc_explosion_zeroed", "plc_explosion_attenuated")
REJECTED_INSERTS = [(0xFD, 40, -5), (0x78, 40, -5), (0xF0, 40, -5), (0xFC, 1277, -4)]       # TOC, length, opus_decode()'s answer


def assert_frames_equal(pcm, rng, ret, want, wrng, wret, ln, what):
    """ret and final range on every frame; PCM on every frame the reference did not reject"""
    ok = wret >= 0
    pcm, want = pcm.copy(), want.copy()
    pcm[~ok] = 0
    want[~ok] = 0
    _assert_all_equal(pcm, rng, ret, want, wrng, wret, ln, what)


def streams_of(name):
    """the streams of a stored case: (packets, lengths, expected pcm, rng, ret, corrupt mask) each"""
    pk, ln, fps, want, wrng, wret, co = mco.load_case(name)
    return [tuple(a[s:s + fps] for a in (pk, ln, want, wrng, wret, co)) for s in range(0, len(ln), fps)]


def test_fixture_is_what_the_issue_describes():
    total = odd = 0
    for name in mco.CASE_NAMES:
        pk, ln, fps, want, wrng, wret, co = mco.load_case(name)
        assert fps == 16 and pk.shape[1] == 1280 and len(ln) % fps == 0
        assert all(int(t) in mco.TOCS for t in pk[ln > 0, 0])
        assert not co.reshape(-1, fps)[:, :2].any() and (ln.reshape(-1, fps)[:, :2] > 2).all()
        assert (wret[ln == 1277] == -4).all() and (wret[ln != 1277] != -4).all()
        odd += int((wret[ln != 1277] != 960).sum())
        total += len(ln)
    assert total <= mco.MAX_FRAMES and odd * 20 <= total
    ln = mco.load_case("truncate")[1]
    assert {2, 3, 4}.issubset(ln.tolist())
    ln, _f, _w, _r, wret = mco.load_case("extend")[1:6]
    assert (ln == 1276).sum() == 1 and (ln == 1277).sum() == 1
    k = int(np.nonzero(ln == 1277)[0][0])
    assert (wret[k + 1:(k // 16 + 1) * 16] == 960).all()                      # the valid packets after it still decode
    pk, ln = mco.load_case("random")[:2]
    assert set(ln.tolist()) >= set(mco.RANDOM_LENGTHS) and set(pk[:, 0].tolist()) == set(mco.TOCS)
    ln = mco.load_case("corrupt_then_lost")[1].reshape(-1, 16)
    assert (ln[:, 3] == 0).all() and (ln[:, 6] == 1).all() and (ln[:, 9:] == 0).all()


@pytest.mark.parametrize("name", mco.CASE_NAMES)
def test_emulated_decode_of_corrupt_packets_matches_reference(name):
    pk, ln, fps, want, wrng, wret, _co = mco.load_case(name)
    pcm, rng, ret = plc_emulib.decode(pk, ln, fps)
    assert_frames_equal(pcm, rng, ret, want, wrng, wret, ln, name)


def lane_decode(pk, ln, fps, slot):
    emu = emulib.lane_lib()
    pk, ln = np.ascontiguousarray(pk), np.ascontiguousarray(ln.astype(np.int32))
    n = pk.shape[0]
    pcm = np.zeros((n, 960, 2), np.int16)
    rng = np.zeros(n, np.uint32)
    ret = np.zeros(n, np.int32)
    emu.emu_lane_set_slot(slot)
    clean = emu.emu_lane_celt_decode_frames(p(pk), pk.shape[1], p(ln), n, fps, p(pcm), p(rng), p(ret))
    return pcm, rng, ret, clean


LANE_SLOTS = dict(zip(mco.CASE_NAMES, (0, 63, 1, 62, 31, 32, 17, 46)))


@pytest.mark.skipif(not os.path.exists(emulib.HOST_CLANG), reason="host clang of the ROCm image not present")
@pytest.mark.parametrize("name", mco.CASE_NAMES)
def test_lane_build_decodes_corrupt_packets_inside_its_own_lds_column(name):
    """The lane build (per-stream PVQ scratch in one column of a 64-column LDS image) on the corpus, in a column of its own per
    case: before every frame the other 63 columns hold a sentinel pattern, and they must hold it afterwards (the library's return
    value). A loss-free stream must equal the fixture. The lane emulation has no concealment, so from a stream with lost or DTX
    packets (payload under two bytes) those packets are dropped, and what remains must equal the wave-per-stream emulation of
    the same packets, which the test above pins to the reference."""
    slot = LANE_SLOTS[name]
    for s, (pk, ln, want, wrng, wret, _co) in enumerate(streams_of(name)):
        if not mco.is_loss_free(ln):
            keep = ln > 2
            pk, ln = pk[keep], ln[keep]
            want, wrng, wret = plc_emulib.decode(pk, ln, len(ln))
        pcm, rng, ret, clean = lane_decode(pk, ln, len(ln), slot ^ s)
        assert clean == 0, "%s stream %d: the lane wrote outside LDS column %d" % (name, s, slot ^ s)
        assert_frames_equal(pcm, rng, ret, want, wrng, wret, ln, "%s stream %d (lane build)" % (name, s))


def rejected_insert_cases():
    """A valid stream, and the same stream with one packet that opus_decode() rejects inserted before frame 5: (name, packets,
    lengths, index of the insert, its return value). Garbage behind an unaccepted TOC; 1277 bytes behind 0xFC."""
    pk, ln = mcg.load_case("switch_stream")[:2]
    pk = np.pad(pk[:16], ((0, 0), (0, 1280 - pk.shape[1])))
    ln = ln[:16]
    rs = np.random.default_rng(4405)
    out = []
    for toc, n, want in REJECTED_INSERTS:
        row = rs.integers(0, 256, 1280, dtype=np.uint8)
        row[0] = toc
        row[n:] = 0
        out.append(("toc 0x%02X, %d bytes" % (toc, n), np.concatenate([pk[:5], row[None], pk[5:]]),
                    np.concatenate([ln[:5], [n], ln[5:]]).astype(np.int32), 5, want))
    return (pk, ln), out


def test_a_rejected_packet_leaves_the_state_alone():
    (pk, ln), inserts = rejected_insert_cases()
    want, wrng, wret = plc_emulib.decode(pk, ln, len(ln))
    assert (wret == 960).all()
    for what, ipk, iln, k, code in inserts:
        pcm, rng, ret = plc_emulib.decode(ipk, iln, len(iln))
        assert ret[k] == code, (what, ret[k])
        assert rng[k] == wrng[k - 1], "%s: OPUS_GET_FINAL_RANGE moved on a rejected packet" % what
        rest = np.arange(len(iln)) != k
        _assert_all_equal(pcm[rest], rng[rest], ret[rest], want, wrng, wret, ln, what)


def per_frame_counts(pk, ln, fps, names):
    """events of the named counters per frame of one emulated decode: int64 [n][len(names)]"""
    lib = plc_emulib.lib()
    arr = (C.c_char_p * len(names))(*[k.encode() for k in names])
    out = np.zeros((len(ln), len(names)), np.int64)
    plc_emulib.counts_reset()
    lib.emu_plc_trace_counts(arr, len(names), p(out))
    try:
        plc_emulib.decode(pk, ln, fps)
    finally:
        lib.emu_plc_trace_counts(None, 0, None)
    return np.diff(out, axis=0, prepend=0)


def corpus_counts():
    """case -> events per counter on the CORRUPT frames of the case (the explosion guards: on concealed frames whose last
    received frame was corrupt)"""
    names = NEW_COUNTERS + EXPLOSION
    res = {}
    for name in mco.CASE_NAMES:
        pk, ln, fps, _w, _r, _ret, co = mco.load_case(name)
        per = per_frame_counts(pk, ln, fps, names)
        after_corrupt = np.zeros(len(ln), bool)
        for s in range(0, len(ln), fps):
            last = False
            for f in range(s, s + fps):
                if ln[f] > 2:
                    last = bool(co[f])
                else:
                    after_corrupt[f] = last
        c = {k: int(per[co, i].sum()) for i, k in enumerate(NEW_COUNTERS)}
        for k in EXPLOSION:
            c[k] = int(per[after_corrupt, names.index(k)].sum())
        res[name] = c
    return res


def test_corrupt_frames_reach_the_branches():
    counts = corpus_counts()
    total = {k: sum(c[k] for c in counts.values()) for k in NEW_COUNTERS + EXPLOSION}
    print(counts)
    for k in NEW_COUNTERS:
        if k != "corrupt_tell_past_end":                          # (may be unreachable: see the docstring)
            assert total[k] >= 1, (k, total)
    assert total["plc_explosion_zeroed"] + total["plc_explosion_attenuated"] >= 1, total
    assert counts["const"]["corrupt_silence_long"] >= 1 and counts["const"]["corrupt_payload_one_byte"] == 9


# ---- live reference -------------------------------------------------------------------------------------------------------------
LIVE = [(16000, 1), (32000, 2), (64000, 3), (96000, 4)]          # bit rate, seed


def live_corrupt_streams(seed, nstreams, fps, bitrate):
    """random_settings_streams under random loss, 30 % of the received packets corrupted -- by a flip of 1 % of the payload bits,
    a truncation or a random payload, the seed chooses which: packets [n][1280], lengths [n]"""
    pk, ln = random_settings_streams(seed, nstreams, fps, bitrate)
    pk = np.pad(pk, ((0, 0), (0, 1280 - pk.shape[1])))
    rs = np.random.default_rng(1000 + seed)
    ln[random_loss_mask(rs, nstreams, fps).reshape(-1)] = 0
    kind = seed % 3
    for k in np.nonzero((ln > 0) & (rs.random(len(ln)) < 0.3))[0]:
        n = int(ln[k])
        if kind == 0:
            nb = (n - 1) * 8
            for b in rs.choice(nb, size=max(1, nb // 100), replace=False):
                pk[k, 1 + b // 8] ^= 1 << (b % 8)
        elif kind == 1:
            ln[k] = int(rs.integers(2, n))
            pk[k, ln[k]:] = 0
        else:
            pk[k, 1:n] = rs.integers(0, 256, n - 1, dtype=np.uint8)
    return pk, ln


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref is absent")
@pytest.mark.parametrize("bitrate,seed", LIVE)
def test_emulated_decode_of_corrupt_packets_matches_live_reference(bitrate, seed):
    nstreams, fps = 4, 24
    pk, ln = live_corrupt_streams(seed, nstreams, fps, bitrate)
    want, wrng, wret = mco.gm.ref_decode(pk, ln, fps)
    pcm, rng, ret = plc_emulib.decode(pk, ln, fps)
    assert_frames_equal(pcm, rng, ret, want, wrng, wret, ln, "%d b/s seed %d" % (bitrate, seed))


# ---- the stand-alone sanitizer program ----------------------------------------------------------------------------------------
def garbage_sample(seed=768):
    """48 streams of 16 frames of garbage: random, all-0xFF and all-0x00 payloads, ten lengths, all eight TOCs"""
    rs = np.random.default_rng(seed)
    lengths = [2, 3, 4, 8, 16, 64, 160, 400, 1276, 0]
    n = 48 * 16
    pk = np.zeros((n, 1280), np.uint8)
    ln = np.zeros(n, np.int32)
    for k in range(n):
        ln[k] = lengths[int(rs.integers(0, len(lengths)))]
        fill = k % 3
        pk[k, :1276] = rs.integers(0, 256, 1276, dtype=np.uint8) if fill == 0 else (0xFF if fill == 1 else 0x00)
        pk[k, 0] = mco.TOCS[int(rs.integers(0, 8))]
        pk[k, ln[k]:] = 0
    return pk, ln


def write_corpus(path, pk, ln, fps):
    with open(path, "wb") as f:
        f.write(np.array([len(ln), fps, pk.shape[1]], np.int32).tobytes())
        f.write(np.ascontiguousarray(ln.astype(np.int32)).tobytes())
        f.write(np.ascontiguousarray(pk).tobytes())


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_sanitizer_build_decodes_the_corpus_clean(tmp_path):
    exe = str(tmp_path / "decode_corpus")
    src = os.path.join(HERE, "emu", "decode_corpus_main.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-fwrapv", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-w", "-o", exe, src])
    parts = [mco.load_case(name)[:2] for name in mco.CASE_NAMES] + [garbage_sample()]
    pk = np.concatenate([a for a, _b in parts])
    ln = np.concatenate([b for _a, b in parts])
    write_corpus(str(tmp_path / "corpus.bin"), pk, ln, 16)
    r = subprocess.run([exe, str(tmp_path / "corpus.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    done = [int(w) for w in r.stdout.replace(",", " ").split() if w.isdigit()]
    assert sum(done) == len(ln) and done[2] == int((ln == 1277).sum()), r.stdout
