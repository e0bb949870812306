"""GPU tier of the two-channel second front stage (celt_front2_kernel: both channels through every lane loop together, the
transform in place): packets, lengths and final ranges of the inputs of tests/front2_joint_cases.py, bit for bit against what
the compiled reference encoded from them (tests/golden/front2_joint_golden.npz, tests/golden/make_front2_joint_golden.py).
Three sets of 64 independent frames -- noise, a mid-frame attack, one channel zero -- through encode_independent, and 64
streams, one frame of each per call for ten calls, through the streams entry; the recorder checked on the host build that the
sets reach the short-block transform, the transient patch's second transform and plain long blocks."""
import os

import numpy as np
import pytest

import encode_cases as ec
import front2_joint_cases as fj

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "front2_joint_golden.npz")


@pytest.fixture(scope="module")
def ca():
    import torch
    assert torch.cuda.is_available()
    import concentus_amd
    concentus_amd.lib.load()
    return concentus_amd


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _expected(gold, name, pcm):
    assert str(gold[name + "_pcm_sha256"]) == fj.digest(pcm), "%s: the input is not the one the golden was recorded from" % name
    return gold[name + "_packets"], gold[name + "_len"], gold[name + "_rng"]


@pytest.mark.parametrize("name,make", fj.INDEPENDENT, ids=[n for n, _ in fj.INDEPENDENT])
def test_independent_frames_match_the_reference(ca, gold, name, make):
    import torch
    pcm = make()
    pk, ln, rg = _expected(gold, name, pcm)
    cfg = ca.CeltConfig(2, fj.CFG[0], fj.CFG[1], fj.CFG[2], fj.CFG[3], 16, 0, 1500)
    out, lens, rng = ca.encode_independent(torch.from_numpy(np.ascontiguousarray(pcm)).cuda(), cfg)
    torch.cuda.synchronize()
    ec.assert_packets_equal(out.cpu().numpy(), lens.cpu().numpy(), rng.cpu().numpy().view(np.uint32), pk, ln, rg, name)


def test_streams_match_the_reference(ca, gold):
    import torch
    pcm = fj.streams()
    pk, ln, rg = _expected(gold, "streams", pcm)
    ns, fps = fj.STREAMS, fj.STREAM_FRAMES
    enc = ca.OpusEncoderBatch(ns).apply_opus_demo_ctls(*fj.CFG)
    p4 = pcm.reshape(ns, fps, 960, 2)
    for f in range(fps):
        o, l = enc.encode(torch.from_numpy(np.ascontiguousarray(p4[:, f])).cuda())
        torch.cuda.synchronize()
        idx = np.arange(ns) * fps + f
        ec.assert_packets_equal(o.cpu().numpy(), l.cpu().numpy(), enc.ctl(4031).cpu().numpy().view(np.uint32),
                                pk[idx], ln[idx], rg[idx], "streams, frame %d" % f)
