"""GPU tests of the decoder's packet layer (opusgpu_packet_parse_batch, opusgpu_decode_batch_packets through
OpusDecoderBatch.decode_packets): CELT-only packets of 1..48 frames (frame-count codes 0-3), padding, DTX frames and malformed
packets, bit-exact against the compiled reference's committed opus_decode() outputs (tests/golden/multi_golden.npz) and against the
host emulation of the same sources; the samples behind `ret` must keep what the caller put there."""
import numpy as np
import pytest

import multi_emulib
from test_decode_multi_emu_cpu import assert_multi_equal, fuzz_batches, long_packets, mmg

pytestmark = pytest.mark.gpu
SENT = multi_emulib.SENTINEL
mag = mmg.mag


@pytest.fixture(scope="module")
def ca():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import concentus_amd
    concentus_amd.lib.load()
    return concentus_amd


def _gpu_decode_packets(ca, pk, ln, fsz, fps, max_frames=48):
    """Streams of fps packets, every stream through its own decoder, packet f of all streams in one call; pcm [n][rows][2]
    pre-filled with the sentinel, rng [n], ret [n]"""
    import torch
    n = pk.shape[0]
    ns = n // fps
    rows = int(np.max(fsz))
    dec = ca.OpusDecoderBatch(ns)
    d_pk = torch.from_numpy(np.ascontiguousarray(pk.reshape(ns, fps, pk.shape[1]).transpose(1, 0, 2))).cuda()
    d_ln = torch.from_numpy(np.ascontiguousarray(ln.reshape(ns, fps).T.astype(np.int32))).cuda()
    fs = np.broadcast_to(np.asarray(fsz, np.int32), (n,)).reshape(ns, fps)
    assert (fs == fs[0]).all(), "the streams of one call share its frame_size"
    outs = []
    for f in range(fps):
        buf = torch.full((ns, int(fs[0, f]), 2), SENT, dtype=torch.int16, device="cuda")
        o, r = dec.decode_packets(d_pk[f], d_ln[f], frame_size=int(fs[0, f]), max_frames=max_frames, out=buf)
        outs.append((o, r, dec.ctl(4031)))
    torch.cuda.synchronize()
    pcm = np.full((ns, fps, rows, 2), SENT, np.int16)
    for f, (o, _r, _g) in enumerate(outs):
        pcm[:, f, :o.shape[1]] = o.cpu().numpy()
    ret = np.stack([r.cpu().numpy() for _o, r, _g in outs], 1).reshape(n)
    rng = np.stack([g.cpu().numpy().view(np.uint32) for _o, _r, g in outs], 1).reshape(n)
    return pcm.reshape(n, rows, 2), rng, ret


@pytest.mark.parametrize("name", mmg.CASE_NAMES)
def test_gpu_decode_matches_golden(ca, name):
    pk, ln, fsz, fps, wret, wrng, wpcm = mmg.load_case(name)
    pcm, rng, ret = _gpu_decode_packets(ca, pk, ln, fsz, fps)
    assert_multi_equal(pcm, rng, ret, wret, wrng, wpcm, name)


def _assert_equals_emulation(got, want, what):
    pcm, rng, ret = got
    wpcm, wrng, wret, _fr = want
    assert np.array_equal(ret, wret), "%s: return values differ at %s" % (what, np.nonzero(ret != wret)[0].tolist())
    assert np.array_equal(rng, wrng), "%s: final range differs at %s" % (what, np.nonzero(rng != wrng)[0].tolist())
    bad = np.nonzero((pcm != wpcm).any(axis=(1, 2)))[0]
    assert bad.size == 0, "%s: PCM differs from the emulation's at packets %s" % (what, bad.tolist())


@pytest.fixture(scope="module")
def mixed_batch():
    """65 streams of 2 packets (a 64-lane workgroup and one more, three 32-lane wavefronts): the fixture's streams in turn, every
    further round starting one packet later in its source. Expected: the host emulation, stream by stream."""
    ns, fps = 65, 2
    src = []
    for name in mmg.CASE_NAMES:
        if name == "too_small":
            continue
        pk, ln, _fsz, sfps = mmg.load_case(name)[:4]
        for s in range(pk.shape[0] // sfps):
            src.append((pk[s * sfps:(s + 1) * sfps], ln[s * sfps:(s + 1) * sfps]))
    stride = max(p.shape[1] for p, _l in src)
    pk = np.zeros((ns * fps, stride), np.uint8)
    ln = np.zeros(ns * fps, np.int32)
    for s in range(ns):
        p, l = src[s % len(src)]
        idx = (s // len(src) + np.arange(fps)) % len(l)
        pk[s * fps:(s + 1) * fps, :p.shape[1]] = p[idx]
        ln[s * fps:(s + 1) * fps] = l[idx]
    return pk, ln, fps


@pytest.fixture(scope="module")
def mixed_emulated(mixed_batch):
    pk, ln, fps = mixed_batch
    return multi_emulib.decode(pk, ln, fps)


def test_mixed_batch_holds_every_configuration(mixed_batch, mixed_emulated):
    pk, ln, fps = mixed_batch
    _pcm, rng, ret, fr = mixed_emulated
    for f in range(fps):
        ok = ret[f::fps] > 0
        assert {1, 2, 3, 8, 48} <= set(fr["ret"][f::fps][ok].tolist()), f
        assert {120, 240, 480, 960} <= set(fr["frame_samples"][f::fps][ok].tolist())
        tocs = fr["toc"][f::fps][ok & (ln[f::fps] > 0)]
        assert set((tocs & 4).tolist()) == {0, 4} and len(set((tocs >> 5).tolist())) >= 3
    assert (ret[ln == 0] == 960).all() and (ln == 0).any() and (ret == -4).any()
    dtx = [(fr["size"][k, :fr["ret"][k]] <= 1).any() for k in range(len(ret)) if ret[k] > 0 and ln[k] > 0]
    assert any(dtx)


@pytest.mark.parametrize("lane_frames", [32, 64])
def test_mixed_batch_matches_the_host_emulation(ca, mixed_batch, mixed_emulated, monkeypatch, lane_frames):
    pk, ln, fps = mixed_batch
    monkeypatch.setenv("OPUSGPU_LANE_FRAMES", str(lane_frames))
    got = _gpu_decode_packets(ca, pk, ln, 5760, fps)
    _assert_equals_emulation(got, mixed_emulated, "65 streams, %d per wavefront" % lane_frames)
    assert (got[0][got[2] < 0] == np.int16(SENT)).all()                  # a rejected stream's whole row is left alone


def test_more_frames_than_max_frames_is_refused_whole(ca):
    """three frames against max_frames = 2: OPUSGPU_UNIMPLEMENTED, nothing written, and the stream's next packet decodes as it does
    when the refused one is left out"""
    import torch
    pk, ln, _fsz, fps = mmg.load_case("rp_code3_vbr")[:4]
    pk, ln = pk[:fps], ln[:fps]                                          # stream 0: two packets of three 10 ms frames
    dec = ca.OpusDecoderBatch(1)
    d_pk, d_ln = torch.from_numpy(pk).cuda(), torch.from_numpy(ln).cuda()
    buf = torch.full((1, 5760, 2), SENT, dtype=torch.int16, device="cuda")
    _o, r0 = dec.decode_packets(d_pk[0:1], d_ln[0:1], max_frames=2, out=buf)
    g0 = dec.ctl(4031).cpu().numpy()
    assert r0.cpu().numpy().tolist() == [-5] and (buf.cpu().numpy() == np.int16(SENT)).all() and g0.tolist() == [0]
    o, r1 = dec.decode_packets(d_pk[1:2], d_ln[1:2], max_frames=3, out=buf)
    wpcm, wrng, wret, _fr = multi_emulib.decode(pk[1:2], ln[1:2], 1)
    assert r1.cpu().numpy().tolist() == wret.tolist() == [1440]
    assert np.array_equal(dec.ctl(4031).cpu().numpy().view(np.uint32), wrng) and np.array_equal(o.cpu().numpy(), wpcm)


def test_code0_packets_equal_decode_any(ca):
    """streams of three code-0 packets under each of the 32 TOCs (the fixture's packets of the TOC's frame size and channel count,
    the bandwidth bits rewritten: both paths take the bytes as they are): decode_packets(max_frames=1, frame_size=960) against
    decode(any_frame_size=True), PCM, ret and final range"""
    import torch
    by = {}
    for name in ("static_e0", "static_e4", "static_e8", "static_ec", "static_f0", "static_f4", "fs_switch_stream"):
        pk, ln = mag.load_case(name)[:2]
        for p, l in zip(pk, ln):
            if l > 2:
                by.setdefault(int(p[0]) & 0x1C, []).append((p, int(l)))
    assert len(by) == 8, sorted(by)
    tocs = [0x80 | bw << 5 | fs << 3 | st << 2 for bw in range(4) for fs in range(4) for st in range(2)]
    stride = max(p.shape[0] for v in by.values() for p, _l in v)
    pk = np.zeros((3, 32, stride), np.uint8)
    ln = np.zeros((3, 32), np.int32)
    for s, toc in enumerate(tocs):
        for f in range(3):
            p, l = by[toc & 0x1C][(s + f) % len(by[toc & 0x1C])]
            pk[f, s, :p.shape[0]] = p
            pk[f, s, 0] = toc
            ln[f, s] = l
    a, b = ca.OpusDecoderBatch(32), ca.OpusDecoderBatch(32)
    for f in range(3):
        d_pk, d_ln = torch.from_numpy(pk[f]).cuda(), torch.from_numpy(ln[f]).cuda()
        o1 = torch.full((32, 960, 2), SENT, dtype=torch.int16, device="cuda")
        o2 = torch.full((32, 960, 2), SENT, dtype=torch.int16, device="cuda")
        _p, r1 = a.decode_packets(d_pk, d_ln, frame_size=960, max_frames=1, out=o1)
        _p, r2 = b.decode(d_pk, d_ln, any_frame_size=True, out=o2)
        assert np.array_equal(r1.cpu().numpy(), r2.cpu().numpy()) and (r2.cpu().numpy() == [120 << ((t >> 3) & 3) for t in tocs]).all()
        assert np.array_equal(a.ctl(4031).cpu().numpy(), b.ctl(4031).cpu().numpy())
        assert np.array_equal(o1.cpu().numpy(), o2.cpu().numpy()), f


def test_parser_matches_the_emulation(ca):
    """packet_parse_batch on the drawn corpus of the CPU tier (1024 packets) and on lengths it must not read"""
    import torch
    pk, ln = fuzz_batches(4)
    ln = ln.copy()
    ln[[5, 600]] = 0
    ln[[9, 700]] = pk.shape[1] + 1
    ln[11] = -3
    want = multi_emulib.parse(pk, ln)
    got = ca.packet_parse_batch(torch.from_numpy(pk).cuda(), torch.from_numpy(ln).cuda())
    torch.cuda.synchronize()
    for k in ("ret", "frame_samples", "toc", "offset", "size"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert {0, -1, -4} <= set(want["ret"].tolist()) and (want["ret"] > 1).any()


def test_packets_longer_than_the_offsets_can_address_are_refused(ca):
    """48 x 700 bytes (offsets past 32 767) is refused unread with -1 and its row left alone; 48 x 682 bytes decodes as in the emulation"""
    import torch
    pk, ln = long_packets()
    d_pk, d_ln = torch.from_numpy(pk).cuda(), torch.from_numpy(ln).cuda()
    got = ca.packet_parse_batch(d_pk, d_ln)
    want = multi_emulib.parse(pk, ln)
    for k in ("ret", "frame_samples", "toc", "offset", "size"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert want["ret"].tolist() == [-1, 48]
    pcm, rng, ret = _gpu_decode_packets(ca, pk, ln, 5760, 1)
    _assert_equals_emulation((pcm, rng, ret), multi_emulib.decode(pk, ln, 1), "long packets")
    assert ret.tolist() == [-1, 5760] and (pcm[0] == np.int16(SENT)).all()


def test_one_call_replays_from_a_graph(ca):
    """one call with max_frames = 3, captured on a side stream and replayed, equals the direct call"""
    import torch
    pk, ln, _fps = _first_packets()
    ns = pk.shape[0]
    d_pk, d_ln = torch.from_numpy(pk).cuda(), torch.from_numpy(ln).cuda()
    direct = ca.OpusDecoderBatch(ns)
    buf = torch.full((ns, 1920, 2), SENT, dtype=torch.int16, device="cuda")
    want, wret = direct.decode_packets(d_pk, d_ln, frame_size=1920, max_frames=3, out=buf)
    wrng = direct.ctl(4031).clone()
    torch.cuda.synchronize()
    L = ca.lib.load()
    dec = ca.OpusDecoderBatch(ns)
    frames = torch.zeros((ns, 200), dtype=torch.uint8, device="cuda")
    out = torch.full((ns, 1920, 2), SENT, dtype=torch.int16, device="cuda")
    ret = torch.zeros(ns, dtype=torch.int32, device="cuda")
    rng = torch.zeros(ns, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            rc = L.opusgpu_decode_batch_packets(dec._states.data_ptr(), d_pk.data_ptr(), d_pk.shape[1], d_ln.data_ptr(), out.data_ptr(), 1920, 3,
                                                frames.data_ptr(), ret.data_ptr(), rng.data_ptr(), ns, ca.lib.current_stream_handle())
    assert rc == 0
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(ret.cpu().numpy(), wret.cpu().numpy()) and np.array_equal(rng.cpu().numpy(), wrng.cpu().numpy())
    assert np.array_equal(out.cpu().numpy(), want.cpu().numpy())
    assert {-5, -2, 1440, 1920} <= set(ret.cpu().numpy().tolist())


def _first_packets():
    """the first packet of every fixture stream: decoded, refused for its frame count (-5) and for its duration (-2) side by side"""
    rows = []
    for name in mmg.CASE_NAMES:
        pk, ln, _fsz, sfps = mmg.load_case(name)[:4]
        rows += [(pk[s], ln[s]) for s in range(0, pk.shape[0], sfps)]
    stride = max(p.shape[0] for p, _l in rows)
    pk = np.zeros((len(rows), stride), np.uint8)
    for k, (p, _l) in enumerate(rows):
        pk[k, :p.shape[0]] = p
    return pk, np.array([l for _p, l in rows], np.int32), 1
