"""CPU tier of the decoder's packet layer (opusgpu_packet_parse_batch / opusgpu_decode_batch_packets): the host build of the same
parser and frame loop (tests/emu/celt_dec_multi_emu.cpp) against the compiled reference's committed opus_decode() outputs
(tests/golden/multi_golden.npz: frame-count codes 0-3, padding, DTX frames, malformed packets), the parser against the live
reference's opus_packet_parse on a drawn corpus, and the parser as a stand-alone program under the address and undefined-behaviour
sanitizers."""
import importlib.util
import os
import struct
import subprocess

import numpy as np
import pytest

import multi_emulib
import reflib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_multi_golden", os.path.join(ROOT, "tests", "golden", "make_multi_golden.py"))
mmg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mmg)

SENT = multi_emulib.SENTINEL
SENT16 = np.int16(SENT)


def assert_multi_equal(pcm, rng, ret, wret, wrng, wpcm, what):
    """pcm [n][rows][2] pre-filled with the sentinel; wpcm: the expected samples of all packets, concatenated"""
    assert np.array_equal(ret, wret), "%s: return values %s, expected %s" % (what, ret.tolist(), wret.tolist())
    assert np.array_equal(rng, wrng), "%s: final range differs at packets %s" % (what, np.nonzero(rng != wrng)[0].tolist())
    pos = 0
    for k in range(len(ret)):
        r = max(int(wret[k]), 0)
        bad = np.nonzero((pcm[k, :r] != wpcm[pos:pos + r]).any(axis=1))[0]
        assert bad.size == 0, "%s: packet %d differs from sample %d on (%d of %d)" % (what, k, bad[0], bad.size, r)
        assert (pcm[k, r:] == SENT16).all(), "%s: packet %d wrote behind its %d samples" % (what, k, r)
        pos += r
    assert pos == len(wpcm)


@pytest.fixture(scope="module")
def golden_runs():
    """every golden case through the emulation once, with the branch counters of the whole run"""
    multi_emulib.counts_reset()
    runs = {}
    for name in mmg.CASE_NAMES:
        pk, ln, fsz, fps, wret, wrng, wpcm = mmg.load_case(name)
        runs[name] = (multi_emulib.decode(pk, ln, fps, frame_size=fsz), (wret, wrng, wpcm))
    return runs, multi_emulib.counts()


@pytest.mark.parametrize("name", mmg.CASE_NAMES)
def test_emulation_matches_golden(golden_runs, name):
    (pcm, rng, ret, _fr), (wret, wrng, wpcm) = golden_runs[0][name]
    assert_multi_equal(pcm, rng, ret, wret, wrng, wpcm, name)


def test_golden_reaches_every_branch(golden_runs):
    c = golden_runs[1]
    for k in ("pkt_code0", "pkt_code1", "pkt_code2", "pkt_code3", "pkt_code3_vbr", "pkt_code3_cbr", "pkt_padding", "pkt_padding_chained",
              "pkt_size_two_bytes", "multi_dtx_lm0", "multi_dtx_lm1", "multi_dtx_lm2", "multi_dtx_lm3", "multi_dtx_short",
              "fs_loss_after_short", "fs_short_step_pitch", "fs_short_step_noise", "plc_no_history", "plc_pitch_first", "plc_pitch_repeat",
              "plc_noise", "multi_frame_decoded"):
        assert c[k] > 0, (k, c)


def test_rejections_of_our_own(golden_runs):
    """count > max_frames and a SILK / hybrid TOC give OPUSGPU_UNIMPLEMENTED and leave the stream alone: the packet after them decodes
    as it does when they are left out"""
    pk, ln, fsz, fps, wret, wrng, wpcm = mmg.load_case("rp_code3_vbr")
    first = slice(0, fps)                                  # stream 0: two packets of three 10 ms frames
    pcm, rng, ret, _fr = multi_emulib.decode(pk[first], ln[first], fps, max_frames=2)
    assert ret.tolist() == [-5] * fps and (pcm == SENT16).all() and (rng == 0).all()
    silk = pk[first].copy()
    silk[0, 0] = 0x4B                                      # the first packet under a hybrid TOC: parsed, refused
    pcm, rng, ret, fr = multi_emulib.decode(silk, ln[first], fps)
    assert ret[0] == -5 and fr["ret"][0] == 3 and (pcm[0] == SENT16).all()
    alone = multi_emulib.decode(pk[1:2], ln[1:2], 1)
    assert ret[1] == alone[2][0] == 1440 and rng[1] == alone[1][0] and np.array_equal(pcm[1], alone[0][0])


# ---- the corpus of the parser tests: drawn packets, well-formed ones of every code, mutated ones and plain random bytes ----
FUZZ_STRIDE = 1600


def toc_frame_samples(toc):
    if toc & 0x80:
        return 120 << ((toc >> 3) & 3)
    if toc & 0x60 == 0x60:
        return 960 if toc & 8 else 480
    a = (toc >> 3) & 3
    return 2880 if a == 3 else 480 << a


def _draw_size(rs):
    k = rs.integers(0, 10)
    return int(rs.integers(252, 400)) if k == 0 else int(rs.integers(0, 2)) if k == 1 else int(rs.integers(2, 60))


def _draw_packet(rs):
    kind = rs.integers(0, 8)
    if kind == 0:
        return rs.integers(0, 256, int(rs.integers(1, 40)), dtype=np.uint8).tobytes()
    toc = int(rs.integers(0, 256))
    code = toc & 3
    body = lambda n: rs.integers(0, 256, n, dtype=np.uint8).tobytes()
    if code == 0:
        n = int(rs.integers(1270, 1290)) if rs.integers(0, 12) == 0 else _draw_size(rs)
        p = bytes([toc]) + body(n)
    elif code == 1:
        p = bytes([toc]) + body(2 * _draw_size(rs) + int(rs.integers(0, 8) == 0))
    elif code == 2:
        a = _draw_size(rs)
        p = bytes([toc]) + mmg.size_bytes(a) + body(a + (int(rs.integers(1270, 1290)) if rs.integers(0, 12) == 0 else _draw_size(rs)))
    else:
        count = int(rs.integers(0, 5760 // toc_frame_samples(toc) + 2)) if rs.integers(0, 6) == 0 else int(rs.integers(1, 5760 // toc_frame_samples(toc) + 1))
        count = min(count, 63)
        vbr, padded = bool(rs.integers(0, 2)), rs.integers(0, 3) == 0
        head = bytes([toc, (0x80 if vbr else 0) | (0x40 if padded else 0) | count])
        npad = 0
        if padded:
            npad = int(rs.integers(254, 600)) if rs.integers(0, 3) == 0 else int(rs.integers(0, 40))
            q = npad
            while q >= 255:
                head += b"\xff"
                q -= 254
            head += bytes([q])
        if vbr:
            sizes = [_draw_size(rs) if count < 10 else int(rs.integers(0, 12)) for _ in range(max(count, 1))]
            head += b"".join(mmg.size_bytes(s) for s in sizes[:-1])
            p = head + body(sum(sizes)) + bytes(npad)
        else:
            s = _draw_size(rs) if count < 10 else int(rs.integers(0, 12))
            p = head + body(s * count + int(rs.integers(0, 6) == 0)) + bytes(npad)
    if kind >= 6:                                          # mutated: cut short, or a header byte replaced
        if rs.integers(0, 2):
            p = p[:int(rs.integers(1, len(p) + 1))]
        else:
            i = int(rs.integers(0, min(len(p), 6)))
            p = p[:i] + bytes([int(rs.integers(0, 256))]) + p[i + 1:]
    return p[:FUZZ_STRIDE]


def fuzz_batches(n_batches, batch=256, seed=77001):
    """packets uint8 [n_batches * batch][FUZZ_STRIDE], lengths; batch b is the same whatever n_batches is"""
    pk = np.zeros((n_batches * batch, FUZZ_STRIDE), np.uint8)
    ln = np.zeros(n_batches * batch, np.int32)
    for b in range(n_batches):
        rs = np.random.default_rng(seed + b)
        for k in range(b * batch, (b + 1) * batch):
            p = _draw_packet(rs)
            pk[k, :len(p)] = np.frombuffer(p, np.uint8)
            ln[k] = len(p)
    return pk, ln


@pytest.mark.skipif(not reflib.available(), reason="oracle/_ref/libopus_ref.so missing (make -C oracle ref)")
def test_parser_matches_the_live_reference():
    """count, every size, every frame offset and the error code against opus_packet_parse, on as many batches as it takes for the
    reference alone to accept and to reject every code and to see padding and a two-byte length"""
    need = {("ok", c) for c in range(4)} | {("bad", c) for c in range(4)} | {"padding", "two_bytes", "chained"}
    seen, done = set(), 0
    for n_batches in range(4, 44, 4):
        pk, ln = fuzz_batches(n_batches)
        fr = multi_emulib.parse(pk[done:], ln[done:])
        for k in range(done, len(ln)):
            data = pk[k, :ln[k]].tobytes()
            n, toc, sizes, offs = mmg.ref_parse(data)
            code = data[0] & 3
            seen.add(("ok" if n > 0 else "bad", code))
            if n > 0 and code == 3 and data[1] & 0x40:
                seen.add("padding")
                if data[2] == 255:
                    seen.add("chained")
            if n > 0 and ((code == 2 and data[1] >= 252) or (code == 3 and data[1] & 0x80 and any(s >= 252 for s in sizes[:-1]))):
                seen.add("two_bytes")
            g = fr[k - done]
            assert g["ret"] == n, (k, data[:8].hex(), int(g["ret"]), n)
            assert g["toc"] == data[0] and g["frame_samples"] == toc_frame_samples(data[0])
            if n > 0:
                assert g["size"][:n].tolist() == sizes and g["offset"][:n].tolist() == offs, (k, data[:8].hex())
            assert not g["size"][max(n, 0):].any() and not g["offset"][max(n, 0):].any()
        done = len(ln)
        if need <= seen:
            break
    assert need <= seen, need - seen


def test_parser_answers_for_lengths_it_must_not_read():
    pk = np.full((3, 8), 0xFF, np.uint8)
    fr = multi_emulib.parse(pk, np.array([0, 9, -1], np.int32))
    assert fr["ret"].tolist() == [0, -1, -1] and not fr["size"].any() and not fr["offset"].any()


def long_packets():
    """48 CBR frames of 2.5 ms: 700 bytes each (33 602 bytes: frame offsets past 32 767, which the record's int16 cannot hold) and
    682 bytes each (32 738 bytes, the last offset 32 056); rows of 33 604 bytes"""
    pk = np.zeros((2, 33604), np.uint8)
    ln = np.array([2 + 48 * 700, 2 + 48 * 682], np.int32)
    rs = np.random.default_rng(5)
    for k in range(2):
        pk[k, :ln[k]] = rs.integers(0, 256, ln[k], dtype=np.uint8)
        pk[k, :2] = 0xE7, 48
    return pk, ln


def test_packets_longer_than_the_offsets_can_address_are_refused():
    """no offset may wrap: the reference parses both packets; ours refuses the one past 32 767 bytes with OPUSGPU_BAD_ARG, tables
    zero, and the decoder leaves the stream and its row alone"""
    pk, ln = long_packets()
    fr = multi_emulib.parse(pk, ln)
    assert fr["ret"].tolist() == [-1, 48] and not fr["offset"][0].any() and not fr["size"][0].any()
    assert fr["size"][1].tolist() == [682] * 48 and fr["offset"][1].tolist() == [2 + 682 * i for i in range(48)]
    if reflib.available():
        assert [mmg.ref_parse(pk[k, :ln[k]].tobytes())[0] for k in range(2)] == [48, 48]
        assert mmg.ref_parse(pk[1, :ln[1]].tobytes())[3] == fr["offset"][1].tolist()
    pcm, rng, ret, _fr = multi_emulib.decode(pk, ln, 1)
    assert ret.tolist() == [-1, 5760] and (pcm[0] == SENT16).all() and rng[0] == 0


def test_parser_alone_under_the_sanitizers(tmp_path):
    """tests/emu/packet_parse_main.cpp, a plain executable built with -fsanitize=address,undefined: its own packets, the golden
    malformed ones and the drawn corpus, each in a heap block of exactly its length"""
    exe = str(tmp_path / "packet_parse_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-w", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "packet_parse_main.cpp")])
    corpus = str(tmp_path / "corpus.bin")
    with open(corpus, "wb") as f:
        pk, ln = mmg.load_case("malformed")[:2]
        fpk, fln = fuzz_batches(4)
        for p, l in list(zip(pk, ln)) + list(zip(fpk, fln)):
            f.write(struct.pack("<I", int(l)) + p[:l].tobytes())
    r = subprocess.run([exe, corpus], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
