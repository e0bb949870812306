"""GPU tests of the packet loss concealment (opusgpu_decode_batch_plc, opusgpu_decode_lost): PCM, return value and final range
bit-exact against the compiled reference's opus_decode() with lost packets -- committed (tests/golden/plc_golden.npz), live when
oracle/_ref travelled -- and against the host emulation of the same sources. Only valid packets and the lengths 0 and 1 are fed
here; corrupt and truncated packets, and losses right after them, are in tests/test_decode_corrupt_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import encode_cases as ec
import plc_emulib
from test_plc_emu_cpu import CASES, GOLD, assert_frames_equal, load_plc_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_REF = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "librefdrv.so"))


@pytest.fixture(scope="module")
def ca():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import concentus_amd
    concentus_amd.lib.load()
    return concentus_amd


def _gpu_decode_plc(ca, pk, ln, fps):
    """Streams of fps packets, every stream through its own decoder, with concealment; pcm [n][960][2], rng [n], ret [n]."""
    import torch
    n = pk.shape[0]
    ns = n // fps
    dec = ca.OpusDecoderBatch(ns)
    d_pk = torch.from_numpy(np.ascontiguousarray(pk.reshape(ns, fps, pk.shape[1]).transpose(1, 0, 2))).cuda()
    d_ln = torch.from_numpy(np.ascontiguousarray(ln.reshape(ns, fps).T.astype(np.int32))).cuda()
    outs = []
    for f in range(fps):
        o, r = dec.decode(d_pk[f], d_ln[f], conceal=True)
        outs.append((o, r, dec.ctl(4031)))
    torch.cuda.synchronize()
    pcm = np.stack([o.cpu().numpy() for o, _r, _g in outs], 1).reshape(n, 960, 2)
    ret = np.stack([r.cpu().numpy() for _o, r, _g in outs], 1).reshape(n)
    rng = np.stack([g.cpu().numpy().view(np.uint32) for _o, _r, g in outs], 1).reshape(n)
    return pcm, rng, ret


@pytest.mark.parametrize("name", CASES)
def test_gpu_concealment_matches_golden_pcm(ca, name):
    pk, ln, fps, want, wrng = load_plc_case(name)
    pcm, rng, ret = _gpu_decode_plc(ca, pk, ln, fps)
    assert_frames_equal(pcm, rng, ret, want, wrng, ln, name)


@pytest.fixture(scope="module")
def mixed_batch():
    """130 streams of 24 frames (two full 64-stream workgroups and a ragged third), every stream with its own rotation of one loss
    pattern, so that lost and received streams share wavefronts: packets, lengths, expected PCM / final range."""
    ns, fps = 130, 24
    pattern = np.zeros(fps, bool)
    pattern[[3, 6, 7, 10, 11, 12, 13, 14, 15, 16, 20]] = True          # runs of 1, 2, 7 (noise-based from its sixth) and 1
    if HAVE_REF:
        gm = ec.golden_module()
        pk, ln, _rg = gm.ref_encode(gm._Cfg(2, 64000, 1, 0, 10, 16, 0, 1500), gm.synth_pcm("music", ns * fps, 77), fps, threads=8)
        pk = np.ascontiguousarray(pk[:, :(int(ln.max()) + 3) & ~3])
        ln = ln.astype(np.int32)
    else:
        _pcm, gpk, gln, _grg = ec.load_case("gmusic_cvbr_stream")
        pk = np.ascontiguousarray(np.tile(gpk[:fps], (ns, 1)))
        ln = np.tile(gln[:fps].astype(np.int32), ns)
    for s in range(ns):
        ln[s * fps:(s + 1) * fps][np.roll(pattern, s)] = 0
    if HAVE_REF:
        want, wrng, wret = gm.ref_decode(pk, ln, fps, threads=8)
    else:
        want, wrng, wret = plc_emulib.decode(pk, ln, fps)
    assert (wret == 960).all()
    return pk, ln, fps, want, wrng


@pytest.mark.parametrize("lane_frames", [32, 64])
def test_lost_and_received_streams_share_wavefronts(ca, mixed_batch, monkeypatch, lane_frames):
    pk, ln, fps, want, wrng = mixed_batch
    monkeypatch.setenv("OPUSGPU_LANE_FRAMES", str(lane_frames))
    pcm, rng, ret = _gpu_decode_plc(ca, pk, ln, fps)
    assert_frames_equal(pcm, rng, ret, want, wrng, ln, "130 streams, %d per wavefront" % lane_frames)


def test_null_lengths_conceal_every_stream(ca):
    """d_len == NULL: all streams lost. Twice in a row on streams with history: the first loss, then a repeated one."""
    import torch
    pk, ln, fps, _w, _r = load_plc_case("music_vbr_stream")
    ns = pk.shape[0] // fps
    ln = ec.load_case("music_vbr_stream")[2].astype(np.int32).copy()          # nothing lost in the first eight frames ...
    for s in range(ns):
        ln[s * fps + 8:s * fps + 10] = 0                                      # ... then two losses, and nothing after them
    want, _wrng, _wret = plc_emulib.decode(pk, ln, fps)
    dec = ca.OpusDecoderBatch(ns)
    p3 = pk.reshape(ns, fps, -1)
    for f in range(8):
        dec.decode(torch.from_numpy(np.ascontiguousarray(p3[:, f])).cuda(), torch.from_numpy(np.ascontiguousarray(ln.reshape(ns, fps)[:, f])).cuda())
    for f in (8, 9):
        o, r = dec.decode_lost()
        torch.cuda.synchronize()
        assert (r.cpu().numpy() == 960).all() and (dec.ctl(4031).cpu().numpy() == 0).all()
        assert np.array_equal(o.cpu().numpy(), want.reshape(ns, fps, 960, 2)[:, f]), f
    o, r = dec.decode(torch.from_numpy(np.ascontiguousarray(p3[:, 10])).cuda(), torch.from_numpy(np.ascontiguousarray(ln.reshape(ns, fps)[:, 10])).cuda(),
                      conceal=True)
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), want.reshape(ns, fps, 960, 2)[:, 10])


def test_single_stream_decode_lost(ca):
    name = "music_vbr_stream"
    pk, ln, fps, want, _wrng = load_plc_case(name)
    ln_all = ec.load_case(name)[2]
    L = ca.lib.load()
    err = C.c_int(0)
    dec = L.opusgpu_decoder_create(48000, 2, C.byref(err))
    assert dec and err.value == 0
    d = C.c_void_p(dec)
    out = np.full((960, 2), 77, np.int16)
    po = out.ctypes.data_as(C.c_void_p)
    # a fresh decoder has nothing to extrapolate: zeros
    assert L.opusgpu_decode_lost(d, po, 960) == 960 and not out.any()
    assert L.opusgpu_decode_lost(d, po, 480) == -5 and L.opusgpu_decode_lost(d, po, 961) == -1 and L.opusgpu_decode_lost(d, po, 0) == -1
    # stream 1 of the golden case: frame 0 received, frames 1..6 lost
    s1 = fps
    data = (C.c_ubyte * 1500).from_buffer_copy(pk[s1].tobytes().ljust(1500, b"\0"))
    assert L.opusgpu_decode(d, data, int(ln_all[s1]), po, 960, 0) == 960 and np.array_equal(out, want[s1])
    for f in range(1, 7):
        assert L.opusgpu_decode_lost(d, po, 960) == 960
        assert np.array_equal(out, want[s1 + f]), f
        fr, dur = C.c_uint32(1), C.c_int32(0)
        L.opusgpu_decoder_ctl(d, 4031, C.byref(fr))
        L.opusgpu_decoder_ctl(d, 4039, C.byref(dur))
        assert fr.value == 0 and dur.value == 960
    # ... and after the 16 packets of stream 0, the golden concealed frame
    assert L.opusgpu_decoder_ctl(d, 4028) == 0
    for f in range(fps):
        data = (C.c_ubyte * 1500).from_buffer_copy(pk[f].tobytes().ljust(1500, b"\0"))
        assert L.opusgpu_decode(d, data, int(ln_all[f]), po, 960, 0) == 960
    assert L.opusgpu_decode_lost(d, po, 960) == 960
    assert np.array_equal(out, np.load(GOLD)["music_vbr_stream_after16_pcm"])
    fr, dur = C.c_uint32(1), C.c_int32(0)
    L.opusgpu_decoder_ctl(d, 4031, C.byref(fr))
    L.opusgpu_decoder_ctl(d, 4039, C.byref(dur))
    assert fr.value == 0 and dur.value == 960
    # OPUS_RESET_STATE clears the concealment's state with the rest: zeros again
    assert L.opusgpu_decoder_ctl(d, 4028) == 0
    out[:] = 77
    assert L.opusgpu_decode_lost(d, po, 960) == 960 and not out.any()
    L.opusgpu_decoder_destroy(d)


def test_received_only_batch_is_identical_through_both_entry_points(ca):
    import torch
    name = "noise_cvbr_stream"
    _pcm, pk, ln, rg = ec.load_case(name)
    fps = 16
    ns = pk.shape[0] // fps
    a, b = ca.OpusDecoderBatch(ns), ca.OpusDecoderBatch(ns)
    p3, l2 = pk.reshape(ns, fps, -1), ln.astype(np.int32).reshape(ns, fps)
    for f in range(fps):
        d_pk, d_ln = torch.from_numpy(np.ascontiguousarray(p3[:, f])).cuda(), torch.from_numpy(np.ascontiguousarray(l2[:, f])).cuda()
        o1, r1 = a.decode(d_pk, d_ln)
        o2, r2 = b.decode(d_pk, d_ln, conceal=True)
        torch.cuda.synchronize()
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(a.ctl(4031), b.ctl(4031)), f
        assert (r2.cpu().numpy() == 960).all()


def test_reference_cli_with_loss_runs_on_the_compat_library(ca, tmp_path):
    """The reference's unedited opus_demo, linked against libopus_ref.so and against compat/libopus.so (opus_demo_gpu): decoding a
    50-frame .bit file with -loss 20 gives the same output file and exit status. Both draw the same rand() sequence: the compat
    library keeps the caller's generator state out of the GPU runtime's reach (compat/opus_compat.c)."""
    demo, demo_gpu = os.path.join(ROOT, "oracle", "_ref", "opus_demo"), os.path.join(ROOT, "oracle", "_ref", "opus_demo_gpu")
    if not (os.path.exists(demo) and os.path.exists(demo_gpu)):
        pytest.skip("oracle/_ref/opus_demo and opus_demo_gpu did not travel")
    gm = ec.golden_module()
    raw, bit = tmp_path / "in.pcm", tmp_path / "x.bit"
    gm.synth_pcm("music", 50, 4243).astype("<i2").tofile(str(raw))
    r = subprocess.run([demo, "-e", "restricted-lowdelay", "48000", "2", "64000", str(raw), str(bit)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = []
    for exe, out in ((demo, tmp_path / "ref.pcm"), (demo_gpu, tmp_path / "gpu.pcm")):
        r = subprocess.run([exe, "-d", "48000", "2", "-loss", "20", str(bit), str(out)], capture_output=True, text=True, timeout=120)
        res.append((r.returncode, out.read_bytes() if out.exists() else None))
    assert res[0][0] == res[1][0] == 0
    assert res[0][1] is not None and len(res[0][1]) > 40 * 3840 and res[0][1] == res[1][1]
