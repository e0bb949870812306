"""GPU tests of the decoder on CORRUPT and TRUNCATED packets (opusgpu_decode_batch, opusgpu_decode_batch_plc, the single-stream
shim, compat/libopus.so): return value, final range and PCM bit-exact against the compiled reference's opus_decode() on the same
bytes -- committed (tests/golden/corrupt_golden.npz), live when oracle/_ref travelled -- and against the host emulation. Streams
whose neighbours in the wavefront hold corrupt packets must decode as they do alone. Every packet fed here went through the CPU
tier first (tests/test_decode_corrupt_emu_cpu.py): the committed corpus and that tier's live seeds; nothing is drawn afresh."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import plc_emulib
from test_decode_chbw_emu_cpu import mcg
from test_decode_corrupt_emu_cpu import (LIVE, assert_frames_equal, live_corrupt_streams, mco, rejected_insert_cases, streams_of)
from test_decode_gpu import _gpu_decode
from test_plc_gpu import _gpu_decode_plc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_REF = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "librefdrv.so"))
BAD_ARG = -1


@pytest.fixture(scope="module")
def ca():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import concentus_amd
    concentus_amd.lib.load()
    return concentus_amd


@pytest.mark.parametrize("name", mco.CASE_NAMES)
def test_gpu_decode_with_concealment_matches_golden(ca, name):
    pk, ln, fps, want, wrng, wret, _co = mco.load_case(name)
    pcm, rng, ret = _gpu_decode_plc(ca, pk, ln, fps)
    assert_frames_equal(pcm, rng, ret, want, wrng, wret, ln, name)


@pytest.mark.parametrize("name", mco.CASE_NAMES)
def test_gpu_plain_decode_matches_golden(ca, name):
    """the loss-free streams of the case (no packet with a payload under two bytes) through the entry point without concealment"""
    free = [s for s in streams_of(name) if mco.is_loss_free(s[1])]
    if name not in ("random", "corrupt_then_lost"):
        assert free, name
    for pk, ln, want, wrng, wret, _co in free:
        pcm, rng, ret = _gpu_decode(ca, pk, ln, len(ln))
        assert_frames_equal(pcm, rng, ret, want, wrng, wret, ln, name)


@pytest.fixture(scope="module")
def mixed_batch():
    """200 streams of 16 frames (three full 64-stream workgroups and a ragged fourth): the corrupt streams and static_fc, static_98
    and switch_loss_stream tiled, stream s starting s frames into its source. Returns packets, lengths, corrupt mask, fps."""
    ns, fps = 200, 16
    src = []
    for name in mco.CASE_NAMES:
        for pk, ln, _w, _r, _ret, co in streams_of(name):
            src.append((pk, ln, co))
    for name in ("static_fc", "static_98", "switch_loss_stream"):
        pk, ln, sfps = mcg.load_case(name)[:3]
        pk = np.pad(pk, ((0, 0), (0, 1280 - pk.shape[1])))
        for s in range(0, len(ln), sfps):
            src.append((pk[s:s + sfps], ln[s:s + sfps], np.zeros(sfps, bool)))
    pk = np.zeros((ns * fps, 1280), np.uint8)
    ln = np.zeros(ns * fps, np.int32)
    co = np.zeros(ns * fps, bool)
    for s in range(ns):
        q, l, c = src[s % len(src)]
        idx = (s // len(src) * 5 + s + np.arange(fps)) % len(l)
        pk[s * fps:(s + 1) * fps], ln[s * fps:(s + 1) * fps], co[s * fps:(s + 1) * fps] = q[idx], l[idx], c[idx]
    return pk, ln, co, fps


def test_mixed_batch_holds_every_kind_of_stream(mixed_batch):
    pk, ln, co, fps = mixed_batch
    for f in (0, 7, 15):
        l, c, toc = ln[f::fps], co[f::fps], pk[f::fps, 0]
        assert c.any(), f
        assert ((toc == 0xFC) & ~c & (l > 2)).any(), f
        assert (((toc & 4) == 0) & (l > 2)).any(), f
        assert (l == 0).any(), f


@pytest.fixture(scope="module")
def mixed_alone(ca, mixed_batch):
    """every stream of the mixed batch decoded alone, a batch of one each (computed once)"""
    pk, ln, _co, fps = mixed_batch
    parts = [_gpu_decode_plc(ca, pk[s * fps:(s + 1) * fps], ln[s * fps:(s + 1) * fps], fps) for s in range(len(ln) // fps)]
    return tuple(np.concatenate([q[i] for q in parts]) for i in range(3))


@pytest.mark.parametrize("lane_frames", [32, 64])
def test_streams_of_a_mixed_corrupt_wavefront_decode_as_alone(ca, mixed_batch, mixed_alone, monkeypatch, lane_frames):
    pk, ln, _co, fps = mixed_batch
    a_pcm, a_rng, a_ret = mixed_alone
    monkeypatch.setenv("OPUSGPU_LANE_FRAMES", str(lane_frames))
    pcm, rng, ret = _gpu_decode_plc(ca, pk, ln, fps)
    assert_frames_equal(pcm, rng, ret, a_pcm, a_rng, a_ret, ln, "200 streams, %d per wavefront" % lane_frames)


def test_mixed_corrupt_batch_matches_the_host_emulation(ca, mixed_batch):
    pk, ln, _co, fps = mixed_batch
    want, wrng, wret = plc_emulib.decode(pk, ln, fps)
    pcm, rng, ret = _gpu_decode_plc(ca, pk, ln, fps)
    assert_frames_equal(pcm, rng, ret, want, wrng, wret, ln, "200 mixed streams")


def test_all_fullband_stereo_corrupt_wavefront_matches_the_host_emulation(ca):
    """64 streams, every packet 0xFC and every stream corrupt: the wavefront runs celt_decode_front_as<true>, the instantiation
    with channel count and end band fixed, which a mixed batch never reaches"""
    ns, fps = 64, 16
    src = []
    for name in mco.CASE_NAMES:
        for pk, ln, _w, _r, _ret, co in streams_of(name):
            keep = (pk[:, 0] == 0xFC) & (ln > 2) & (ln <= 1276)
            if (keep & co).any():
                src.append((pk[keep], ln[keep]))
    assert len(src) >= 4
    pk = np.zeros((ns * fps, 1280), np.uint8)
    ln = np.zeros(ns * fps, np.int32)
    for s in range(ns):
        q, l = src[s % len(src)]
        idx = (s // len(src) + s + np.arange(fps)) % len(l)
        pk[s * fps:(s + 1) * fps], ln[s * fps:(s + 1) * fps] = q[idx], l[idx]
    assert (pk[:, 0] == 0xFC).all()
    want, wrng, wret = plc_emulib.decode(pk, ln, fps)
    assert (wret == 960).all()
    for decode in (_gpu_decode, _gpu_decode_plc):
        pcm, rng, ret = decode(ca, pk, ln, fps)
        assert_frames_equal(pcm, rng, ret, want, wrng, wret, ln, "64 corrupt 0xFC streams")


def test_a_rejected_packet_leaves_the_gpu_state_alone(ca):
    (pk, ln), inserts = rejected_insert_cases()
    want, wrng, wret = _gpu_decode(ca, pk, ln, len(ln))
    assert (wret == 960).all()
    for what, ipk, iln, k, code in inserts:
        for decode in (_gpu_decode, _gpu_decode_plc):
            pcm, rng, ret = decode(ca, ipk, iln, len(iln))
            assert ret[k] == code, (what, ret[k])
            assert rng[k] == wrng[k - 1], what
            rest = np.arange(len(iln)) != k
            assert_frames_equal(pcm[rest], rng[rest], ret[rest], want, wrng, wret, ln, what)


def test_a_length_past_the_stride_is_a_bad_argument_for_that_stream_only(ca):
    import torch
    streams = [s for name in ("flip1", "flip_many") for s in streams_of(name)][:3]
    pk = np.stack([s[0][2] for s in streams])                               # frame 2 of three streams, on fresh decoders
    ln = np.array([int(s[1][2]) for s in streams], np.int32)
    alone = [ca.decode_independent(torch.from_numpy(pk[i:i + 1]).cuda(), torch.from_numpy(ln[i:i + 1]).cuda()) for i in range(3)]
    bad = ln.copy()
    bad[1] = 1281
    pcm, ret, rng = ca.decode_independent(torch.from_numpy(pk).cuda(), torch.from_numpy(bad).cuda())
    torch.cuda.synchronize()
    assert ret.cpu().numpy().tolist() == [960, BAD_ARG, 960]
    for i in (0, 2):
        assert torch.equal(pcm[i], alone[i][0][0]) and torch.equal(rng[i], alone[i][2][0])


@pytest.mark.parametrize("name,stream", [("flip_many", 0), ("extend", 1)])
def test_single_stream_shim_on_corrupt_packets(ca, name, stream):
    pk, ln, want, wrng, wret, _co = streams_of(name)[stream]
    L = ca.lib.load()
    err = C.c_int(0)
    d = C.c_void_p(L.opusgpu_decoder_create(48000, 2, C.byref(err)))
    assert d and err.value == 0
    out = np.zeros((960, 2), np.int16)
    for f in range(len(ln)):
        data = (C.c_ubyte * 1500).from_buffer_copy(pk[f].tobytes().ljust(1500, b"\0"))
        assert L.opusgpu_decode(d, data, int(ln[f]), out.ctypes.data_as(C.c_void_p), 960, 0) == wret[f], f
        fr = C.c_uint32(0)
        assert L.opusgpu_decoder_ctl(d, 4031, C.byref(fr)) == 0 and fr.value == wrng[f], f
        if wret[f] >= 0:
            assert np.array_equal(out, want[f]), f
    L.opusgpu_decoder_destroy(d)


def test_reference_cli_and_compat_library_agree_on_a_corrupt_file(ca, tmp_path):
    demo, demo_gpu = os.path.join(ROOT, "oracle", "_ref", "opus_demo"), os.path.join(ROOT, "oracle", "_ref", "opus_demo_gpu")
    if not (os.path.exists(demo) and os.path.exists(demo_gpu)):
        pytest.skip("oracle/_ref/opus_demo and opus_demo_gpu did not travel")
    from concentus_amd import bitstream
    pk, ln, _w, wrng, _ret, _co = streams_of("flip_many")[0]
    bit = tmp_path / "corrupt.bit"
    bitstream.write_opus_demo_bit(str(bit), pk, ln, wrng)
    res = []
    for exe, out in ((demo, tmp_path / "ref.pcm"), (demo_gpu, tmp_path / "gpu.pcm")):
        r = subprocess.run([exe, "-d", "48000", "2", str(bit), str(out)], capture_output=True, text=True, timeout=120)
        res.append((r.returncode, out.read_bytes() if out.exists() else None, r.stderr))
    assert res[0][0] == res[1][0], (res[0][2], res[1][2])
    assert res[0][1] is not None and res[0][1] == res[1][1]


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref did not travel")
def test_gpu_decode_of_corrupt_packets_matches_live_reference(ca):
    fps = 24
    parts = [live_corrupt_streams(seed, 4, fps, bitrate) for bitrate, seed in LIVE]
    pk = np.concatenate([np.tile(q.reshape(4, fps, -1), (4, 1, 1)).reshape(-1, q.shape[1]) for q, _l in parts])
    ln = np.concatenate([np.tile(l.reshape(4, fps), (4, 1)).reshape(-1) for _q, l in parts])
    assert len(ln) == 64 * fps
    want, wrng, wret = mco.gm.ref_decode(pk, ln, fps, threads=8)
    pcm, rng, ret = _gpu_decode_plc(ca, pk, ln, fps)
    assert_frames_equal(pcm, rng, ret, want, wrng, wret, ln, "64 streams, live seeds")
