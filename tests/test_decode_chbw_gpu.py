"""GPU tests of the decoder's mono and NB / WB / SWB support (the eight CELT-only 20 ms TOCs 0x98 0xB8 0xD8 0xF8 / 0x9C 0xBC 0xDC
0xFC through opusgpu_decode_batch, opusgpu_decode_batch_plc and the single-stream shim): PCM, return value and final range
bit-exact against the compiled reference's opus_decode() on a (48000, 2) decoder -- committed (tests/golden/chbw_golden.npz),
live when oracle/_ref travelled. Streams whose neighbours in the wavefront differ in channel count and bandwidth must decode as
they do alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import encode_cases as ec
from test_decode_chbw_emu_cpu import assert_frames_equal, mcg, random_settings_streams
from test_decode_gpu import _gpu_decode
from test_plc_emu_cpu import random_loss_mask
from test_plc_gpu import _gpu_decode_plc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_REF = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "librefdrv.so"))
LOSS_FREE = [n for n in mcg.CASE_NAMES if n != "switch_loss_stream"]


@pytest.fixture(scope="module")
def ca():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import concentus_amd
    concentus_amd.lib.load()
    return concentus_amd


@pytest.mark.parametrize("name", mcg.CASE_NAMES)
def test_gpu_decode_with_concealment_matches_golden(ca, name):
    pk, ln, fps, want, wrng, wret = mcg.load_case(name)
    pcm, rng, ret = _gpu_decode_plc(ca, pk, ln, fps)
    assert_frames_equal(pcm, rng, ret, want, wrng, wret, ln, name)


@pytest.mark.parametrize("name", LOSS_FREE)
def test_gpu_plain_decode_matches_golden(ca, name):
    pk, ln, fps, want, wrng, wret = mcg.load_case(name)
    assert mcg.is_loss_free(ln)
    pcm, rng, ret = _gpu_decode(ca, pk, ln, fps)
    assert_frames_equal(pcm, rng, ret, want, wrng, wret, ln, name)


@pytest.fixture(scope="module")
def mixed_batch():
    """200 streams of 24 frames (three full 64-stream workgroups and a ragged fourth): the golden streams tiled, stream s starting
    s frames into its source, so that the lanes of a wavefront hold mono and stereo packets of all four bandwidths next to 0xFC
    streams and lost ones. Expected: each DISTINCT stream decoded alone by the same library."""
    ns, fps = 200, 24
    src = []
    for name in ("switch_stream", "switch_loss_stream", "auto_lowrate_stream", "mono_input_stream", "static_fc", "static_98"):
        pk, ln, sfps = mcg.load_case(name)[:3]
        for s in range(pk.shape[0] // sfps):
            src.append((pk[s * sfps:(s + 1) * sfps], ln[s * sfps:(s + 1) * sfps]))
    stride = max(p.shape[1] for p, _l in src) + 3 & ~3
    pk = np.zeros((ns * fps, stride), np.uint8)
    ln = np.zeros(ns * fps, np.int32)
    for s in range(ns):
        p, l = src[s % len(src)]
        idx = (s // len(src) * 5 + s + np.arange(fps)) % len(l)
        pk[s * fps:(s + 1) * fps, :p.shape[1]] = p[idx]
        ln[s * fps:(s + 1) * fps] = l[idx]
    return pk, ln, fps


def test_mixed_batch_holds_every_configuration(mixed_batch):
    pk, ln, fps = mixed_batch
    for f in (0, 7, 23):
        tocs = set(pk[f::fps, 0][ln[f::fps] > 1].tolist())
        assert {0xFC, 0xF8, 0x98}.issubset(tocs) and len(tocs) >= 5, (f, sorted(hex(t) for t in tocs))
    assert (ln == 0).any() and (ln == 1).any()


@pytest.fixture(scope="module")
def mixed_alone(ca, mixed_batch):
    """every stream of the mixed batch decoded alone, a batch of one each (computed once)"""
    pk, ln, fps = mixed_batch
    parts = [_gpu_decode_plc(ca, pk[s * fps:(s + 1) * fps], ln[s * fps:(s + 1) * fps], fps) for s in range(len(ln) // fps)]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


@pytest.mark.parametrize("lane_frames", [32, 64])
def test_streams_of_a_mixed_wavefront_decode_as_alone(ca, mixed_batch, mixed_alone, monkeypatch, lane_frames):
    pk, ln, fps = mixed_batch
    a_pcm, a_rng, a_ret = mixed_alone
    assert (a_ret == 960).all()
    monkeypatch.setenv("OPUSGPU_LANE_FRAMES", str(lane_frames))
    pcm, rng, ret = _gpu_decode_plc(ca, pk, ln, fps)
    assert_frames_equal(pcm, rng, ret, a_pcm, a_rng, a_ret, ln, "200 streams, %d per wavefront" % lane_frames)


def test_mixed_batch_matches_the_host_emulation(ca, mixed_batch):
    import plc_emulib
    pk, ln, fps = mixed_batch
    want, wrng, wret = plc_emulib.decode(pk, ln, fps)
    pcm, rng, ret = _gpu_decode_plc(ca, pk, ln, fps)
    assert_frames_equal(pcm, rng, ret, want, wrng, wret, ln, "200 mixed streams")


def test_single_stream_shim_follows_the_switches(ca):
    """switch_stream through opusgpu_decode: PCM, OPUS_GET_FINAL_RANGE and OPUS_GET_BANDWIDTH after every packet."""
    pk, ln, fps, want, wrng, _wret = mcg.load_case("switch_stream")
    L = ca.lib.load()
    err = C.c_int(0)
    d = C.c_void_p(L.opusgpu_decoder_create(48000, 2, C.byref(err)))
    assert d and err.value == 0
    bw = C.c_int32(0)
    assert L.opusgpu_decoder_ctl(d, 4009, C.byref(bw)) == 0 and bw.value == 1105          # nothing decoded yet
    out = np.zeros((960, 2), np.int16)
    for f in range(fps):
        data = (C.c_ubyte * 1500).from_buffer_copy(pk[f].tobytes().ljust(1500, b"\0"))
        assert L.opusgpu_decode(d, data, int(ln[f]), out.ctypes.data_as(C.c_void_p), 960, 0) == 960
        assert np.array_equal(out, want[f]), f
        fr = C.c_uint32(0)
        assert L.opusgpu_decoder_ctl(d, 4031, C.byref(fr)) == 0 and fr.value == wrng[f]
        assert L.opusgpu_decoder_ctl(d, 4009, C.byref(bw)) == 0
        assert bw.value == mcg.BANDWIDTH[mcg.SWITCH[f][1]], f
    assert L.opusgpu_decoder_ctl(d, 4028) == 0
    assert L.opusgpu_decoder_ctl(d, 4009, C.byref(bw)) == 0 and bw.value == 1105          # OPUS_RESET_STATE forgets it
    L.opusgpu_decoder_destroy(d)


def test_gpu_still_rejects_other_tocs(ca):
    import torch
    pk = np.full((4, 8), 0x55, np.uint8)
    pk[:, 0] = [0xFD, 0x78, 0xF0, 0x98]
    ln = np.array([8, 8, 8, 1], np.int32)          # code 1; SILK-only; CELT FB 10 ms; a one-byte packet in opusgpu_decode_batch
    _pcm, ret, _r = ca.decode_independent(torch.from_numpy(pk).cuda(), torch.from_numpy(ln).cuda())
    assert ret.cpu().numpy().tolist() == [-5, -5, -5, -5]
    dec = ca.OpusDecoderBatch(1)
    one = np.zeros((1, 8), np.uint8)
    one[0, 0] = 0x78
    _o, r = dec.decode(torch.from_numpy(one).cuda(), torch.from_numpy(np.array([1], np.int32)).cuda(), conceal=True)
    assert r.cpu().numpy().tolist() == [-5]


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref did not travel")
def test_gpu_decode_matches_live_reference(ca):
    nstreams, fps = 64, 24
    pks, lns = [], []
    for i, br in enumerate((16000, 24000, 48000, 96000)):
        pk, ln = random_settings_streams(20 + i, nstreams // 4, fps, br)
        pks.append(pk)
        lns.append(ln)
    stride = max(p.shape[1] for p in pks) + 3 & ~3
    pk = np.concatenate([np.pad(p, ((0, 0), (0, stride - p.shape[1]))) for p in pks])
    ln = np.concatenate(lns)
    ln[random_loss_mask(np.random.default_rng(5), nstreams, fps).reshape(-1)] = 0
    want, wrng, wret = mcg.gm.ref_decode(pk, ln, fps, threads=8)
    assert (wret == 960).all()
    pcm, rng, ret = _gpu_decode_plc(ca, pk, ln, fps)
    assert_frames_equal(pcm, rng, ret, want, wrng, wret, ln, "64 streams, random settings and loss")


def test_reference_cli_mono_swb_file_decodes_on_the_compat_library(ca, tmp_path):
    """The reference's opus_demo encodes with -forcemono -bandwidth SWB (TOC 0xD8); the same unedited CLI linked against
    compat/libopus.so (opus_demo_gpu) decodes the .bit file to the PCM the reference's own decode gives; the batched decoder,
    fed the file through concentus_amd.bitstream, gives it too."""
    import torch
    demo, demo_gpu = os.path.join(ROOT, "oracle", "_ref", "opus_demo"), os.path.join(ROOT, "oracle", "_ref", "opus_demo_gpu")
    if not (os.path.exists(demo) and os.path.exists(demo_gpu)):
        pytest.skip("oracle/_ref/opus_demo and opus_demo_gpu did not travel")
    from concentus_amd import bitstream
    gm = ec.golden_module()
    raw, bit = tmp_path / "in.pcm", tmp_path / "x.bit"
    gm.synth_pcm("music", 30, 4244).astype("<i2").tofile(str(raw))
    r = subprocess.run([demo, "-e", "restricted-lowdelay", "48000", "2", "40000", "-forcemono", "-bandwidth", "SWB", str(raw), str(bit)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    pk, ln, rg = bitstream.read_opus_demo_bit(str(bit), stride=1500)
    assert (pk[:, 0] == 0xD8).all()
    res = []
    for exe, out in ((demo, tmp_path / "ref.pcm"), (demo_gpu, tmp_path / "gpu.pcm")):
        r = subprocess.run([exe, "-d", "48000", "2", str(bit), str(out)], capture_output=True, text=True, timeout=120)
        res.append((r.returncode, out.read_bytes() if out.exists() else None, r.stderr))
    assert res[0][0] == res[1][0] == 0, res[1][2]
    assert res[0][1] is not None and len(res[0][1]) >= 30 * 3840 and res[0][1] == res[1][1]
    want = np.frombuffer(res[0][1], np.int16).reshape(-1, 960, 2)
    dec = ca.OpusDecoderBatch(1)
    for k in range(len(ln)):
        o, r = dec.decode(torch.from_numpy(pk[k:k + 1]).cuda(), torch.from_numpy(ln[k:k + 1]).cuda())
        torch.cuda.synchronize()
        assert int(r.item()) == 960
        assert np.uint32(dec.ctl(4031).cpu().numpy().view(np.uint32)[0]) == rg[k]
        assert np.array_equal(o.cpu().numpy()[0], want[k]), k
