"""GPU tests of the decoder's short frames (opusgpu_decode_batch_any through OpusDecoderBatch.decode(..., any_frame_size=True)):
CELT-only code-0 packets of 2.5, 5, 10 and 20 ms, return value, the first `ret` sample pairs of PCM and the final range bit-exact
against the compiled reference's committed opus_decode() outputs (tests/golden/any_golden.npz) and against the host emulation of
the same sources; the samples behind `ret` must keep what the caller put there.

A loss after a packet shorter than 20 ms is concealed in steps of that packet's duration, as the reference does
(fs_loss_stream)."""
import numpy as np
import pytest

import any_emulib
from test_decode_any_emu_cpu import assert_any_equal, mag

pytestmark = pytest.mark.gpu
SENT = any_emulib.SENTINEL


@pytest.fixture(scope="module")
def ca():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import concentus_amd
    concentus_amd.lib.load()
    return concentus_amd


def _gpu_decode_any(ca, pk, ln, fps, **kw):
    """Streams of fps packets, every stream through its own decoder; pcm [n][960][2] pre-filled with the sentinel, rng [n], ret [n]."""
    import torch
    n = pk.shape[0]
    ns = n // fps
    dec = ca.OpusDecoderBatch(ns)
    d_pk = torch.from_numpy(np.ascontiguousarray(pk.reshape(ns, fps, pk.shape[1]).transpose(1, 0, 2))).cuda()
    d_ln = torch.from_numpy(np.ascontiguousarray(ln.reshape(ns, fps).T.astype(np.int32))).cuda()
    kw = kw or {"any_frame_size": True}
    outs = []
    for f in range(fps):
        buf = torch.full((ns, 960, 2), SENT, dtype=torch.int16, device="cuda") if "any_frame_size" in kw else None
        o, r = dec.decode(d_pk[f], d_ln[f], out=buf, **kw)
        outs.append((o, r, dec.ctl(4031)))
    torch.cuda.synchronize()
    pcm = np.stack([o.cpu().numpy() for o, _r, _g in outs], 1).reshape(n, 960, 2)
    ret = np.stack([r.cpu().numpy() for _o, r, _g in outs], 1).reshape(n)
    rng = np.stack([g.cpu().numpy().view(np.uint32) for _o, _r, g in outs], 1).reshape(n)
    return pcm, rng, ret


@pytest.mark.parametrize("name", mag.CASE_NAMES)
def test_gpu_decode_matches_golden(ca, name):
    pk, ln, fps, want, wrng, wret = mag.load_case(name)
    pcm, rng, ret = _gpu_decode_any(ca, pk, ln, fps)
    assert_any_equal(pcm, rng, ret, want, wrng, wret, name)


@pytest.fixture(scope="module")
def mixed_batch():
    """200 streams of 16 packets (three full 64-stream workgroups and a ragged fourth): the fixture's streams tiled, stream s
    starting s packets into its source, so that the lanes of a wavefront hold all four frame sizes, both channel counts, lost
    streams (after 20 ms and after shorter packets) and rejected ones next to each other; two streams of plain 0xFC packets among them. Expected: the host emulation."""
    ns, fps = 200, 16
    src = []
    for name in ("fs_switch_stream", "fs_loss20_stream", "fs_loss_stream", "fs_corrupt", "static_e0", "static_ec", "static_f4",
                 "static_94", "static_a8", "static_c4"):
        pk, ln, sfps = mag.load_case(name)[:3]
        for s in range(pk.shape[0] // sfps):
            src.append((pk[s * sfps:(s + 1) * sfps], ln[s * sfps:(s + 1) * sfps]))
    p, l = src[0]
    fc = p[:, 0] == 0xFC
    src.append((p[fc], l[fc]))
    stride = max(p.shape[1] for p, _l in src) + 3 & ~3
    pk = np.zeros((ns * fps, stride), np.uint8)
    ln = np.zeros(ns * fps, np.int32)
    for s in range(ns):
        p, l = src[s % len(src)]
        idx = (s // len(src) * 5 + s + np.arange(fps)) % len(l)
        pk[s * fps:(s + 1) * fps, :p.shape[1]] = p[idx]
        ln[s * fps:(s + 1) * fps] = l[idx]
    # rejected streams: a one-byte packet with a short-frame TOC, a code-1 packet, a length past the stride
    pk[5 * fps + 3, 0], ln[5 * fps + 3] = 0xF0, 1
    pk[70 * fps + 2, 0] = 0xE5
    ln[133 * fps + 7] = stride + 1
    return pk, ln, fps


@pytest.fixture(scope="module")
def mixed_emulated(mixed_batch):
    pk, ln, fps = mixed_batch
    return any_emulib.decode(pk, ln, fps)


def test_mixed_batch_holds_every_configuration(mixed_batch, mixed_emulated):
    pk, ln, fps = mixed_batch
    _pcm, _rng, ret = mixed_emulated
    for f in (0, 5, 15):
        for w in range(0, 192, 64):                      # (the ragged fourth workgroup holds eight streams)
            tocs = pk[f::fps, 0][w:w + 64][ln[f::fps][w:w + 64] > 2]
            assert set(((tocs >> 3) & 3).tolist()) == {0, 1, 2, 3} and set((tocs & 4).tolist()) == {0, 4}, (f, w)
    assert set(np.unique(ret).tolist()) >= {-5, -1, 120, 240, 480, 960}
    lost = np.nonzero(ln == 0)[0]
    assert (ret[lost] == 960).all() and ((pk[lost - 1, 0] & 0x18) != 0x18)[lost % fps != 0].any()      # losses after short packets too


@pytest.mark.parametrize("lane_frames", [32, 64])
def test_mixed_batch_matches_the_host_emulation(ca, mixed_batch, mixed_emulated, monkeypatch, lane_frames):
    pk, ln, fps = mixed_batch
    want, wrng, wret = mixed_emulated
    monkeypatch.setenv("OPUSGPU_LANE_FRAMES", str(lane_frames))
    pcm, rng, ret = _gpu_decode_any(ca, pk, ln, fps)
    assert_any_equal(pcm, rng, ret, want, wrng, wret, "200 streams, %d per wavefront" % lane_frames)
    assert (pcm[ret < 0] == SENT).all()                   # a rejected stream's whole row is left alone


def test_without_the_flag_short_tocs_are_still_refused(ca):
    pk, ln, fps = mag.load_case("fs_switch_stream")[:3]
    short = (pk[:, 0] & 0x18) != 0x18
    _pcm, _rng, ret = _gpu_decode_any(ca, pk, ln, fps, conceal=True)
    assert (ret[short] == -5).all() and (ret[~short] == 960).all()
    import torch
    _p, r, _g = ca.decode_independent(torch.from_numpy(pk).cuda(), torch.from_numpy(ln).cuda())
    assert (r.cpu().numpy()[short] == -5).all()
    _p, r, _g = ca.decode_independent(torch.from_numpy(pk).cuda(), torch.from_numpy(ln).cuda(), any_frame_size=True)
    assert (r.cpu().numpy() == [mag.toc_samples(int(t)) for t in pk[:, 0]]).all()


def test_one_call_replays_from_a_graph(ca):
    """the 200-stream batch's first packets: one call captured on a side stream and replayed equals the direct call"""
    import torch
    pk, ln, fps = mag.load_case("fs_switch_stream")[:3]
    ns = 64
    idx = (np.arange(ns) * 3) % fps
    d_pk = torch.from_numpy(np.ascontiguousarray(pk[idx])).cuda()
    d_ln = torch.from_numpy(np.ascontiguousarray(ln[idx])).cuda()
    direct = ca.OpusDecoderBatch(ns)
    buf = torch.full((ns, 960, 2), SENT, dtype=torch.int16, device="cuda")
    want, wret = direct.decode(d_pk, d_ln, any_frame_size=True, out=buf)
    wrng = direct.ctl(4031).clone()
    torch.cuda.synchronize()
    L = ca.lib.load()
    dec = ca.OpusDecoderBatch(ns)
    out = torch.full((ns, 960, 2), SENT, dtype=torch.int16, device="cuda")
    ret = torch.zeros(ns, dtype=torch.int32, device="cuda")
    rng = torch.zeros(ns, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            rc = L.opusgpu_decode_batch_any(dec._states.data_ptr(), d_pk.data_ptr(), d_pk.shape[1], d_ln.data_ptr(), out.data_ptr(),
                                            ret.data_ptr(), rng.data_ptr(), ns, ca.lib.current_stream_handle())
    assert rc == 0
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(ret.cpu().numpy(), wret.cpu().numpy()) and np.array_equal(rng.cpu().numpy(), wrng.cpu().numpy())
    assert np.array_equal(out.cpu().numpy(), want.cpu().numpy())
    assert set(ret.cpu().numpy().tolist()) == {120, 240, 480, 960}
