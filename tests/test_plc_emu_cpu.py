"""CPU tier of the packet loss concealment: the decoder SOURCES with celt_decode_lost (concentus_amd/csrc/celt_plc.h), compiled
for the host with CA_HOST_EMU (tests/emu/celt_plc_emu.cpp), against committed opus_decode() outputs of the compiled reference for
golden streams with lost packets and DTX packets (tests/golden/plc_golden.npz, made by tests/golden/make_plc_golden.py): PCM,
return value and final range bit-exact on EVERY frame -- the received frames after a loss pin the TDAC hand-off and the
loss_count reset -- and, when oracle/_ref is present, against the live reference on fresh packets under random loss.

Which branches the golden cases reach (counter block of the emulation, asserted below): no history, pitch first loss, pitch
repeated loss, noise-based, non-zero post-filter gain during a pitch loss, explosion check zeroed (edge case), explosion check
attenuated (music and edge cases). NOT reached by the golden cases: a good non-transient frame arriving with loss_count >= 10
(the frames after the 12- and 11-loss runs of gmusic are transient); it is data-dependent and not asserted."""
import importlib.util
import os

import numpy as np
import pytest

import encode_cases as ec
import plc_emulib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "plc_golden.npz")
HAVE_REF = os.path.exists(os.path.join(os.path.dirname(HERE), "oracle", "_ref", "librefdrv.so"))

_spec = importlib.util.spec_from_file_location("make_plc_golden", os.path.join(HERE, "golden", "make_plc_golden.py"))
mpg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mpg)

CASES = list(mpg.PLC_CASES)


def load_plc_case(name):
    """packets, lengths with the losses applied, frames per stream, expected PCM / final range."""
    g = np.load(GOLD)
    pk, ln, fps = mpg.case_packets(name)
    assert np.array_equal(ln, g[name + "_len"]), "plc_golden.npz was made with another loss mask: rerun make_plc_golden.py"
    return pk, ln, fps, g[name + "_pcm"], g[name + "_rng"]


def assert_frames_equal(pcm, rng, ret, want, wrng, ln, what):
    assert (ret == 960).all(), "%s: ret %s" % (what, ret[ret != 960][:8])
    assert np.array_equal(rng, wrng), "%s: final range differs at %s" % (what, np.nonzero(rng != wrng)[0][:8])
    bad = np.nonzero((pcm != want).reshape(len(ln), -1).any(1))[0]
    assert bad.size == 0, "%s: PCM differs at frames %s (lengths %s)" % (what, bad[:8], ln[bad[:8]])


@pytest.mark.parametrize("name", CASES)
def test_emulated_concealment_matches_reference_pcm(name):
    pk, ln, fps, want, wrng = load_plc_case(name)
    assert (ln <= 1).sum() >= 9 and (wrng[ln <= 1] == 0).all() and (wrng[ln > 1] != 0).all()
    pcm, rng, ret = plc_emulib.decode(pk, ln, fps)
    assert_frames_equal(pcm, rng, ret, want, wrng, ln, name)


def test_emulated_loss_after_a_whole_stream_matches_reference_pcm():
    pk, ln, fps = mpg.after16_packets()
    pcm, rng, ret = plc_emulib.decode(pk, ln, fps)
    assert ret[-1] == 960 and rng[-1] == 0
    assert np.array_equal(pcm[-1], np.load(GOLD)["music_vbr_stream_after16_pcm"])


def _counts_of(name):
    pk, ln, fps, _w, _r = load_plc_case(name)
    plc_emulib.counts_reset()
    plc_emulib.decode(pk, ln, fps)
    return plc_emulib.counts(), ln


def test_golden_cases_reach_the_branches():
    c, ln = _counts_of("gmusic_cvbr_stream")
    # stream 0: runs of 1, 2, 7, 12 and DTX; stream 1: frame 0 (no history), runs of 2, 6, 1, 11 and DTX
    assert c["plc_no_history"] == 1
    assert c["plc_pitch_first"] == 10
    assert c["plc_pitch_repeat"] == 1 + 4 + 4 + 1 + 4 + 4
    assert c["plc_noise"] == 2 + 7 + 1 + 6
    assert c["plc_no_history"] + c["plc_pitch_first"] + c["plc_pitch_repeat"] + c["plc_noise"] == int((ln <= 1).sum())
    assert c["plc_pitch_postfilter_gain"] > 0
    c, ln = _counts_of("music_vbr_stream")
    assert c["plc_pitch_first"] == 6 and c["plc_pitch_repeat"] == 10 and c["plc_noise"] == 2
    assert c["plc_pitch_postfilter_gain"] > 0
    assert c["plc_explosion_attenuated"] > 0
    c, ln = _counts_of("noise_cvbr_stream")
    assert c["plc_pitch_first"] == 6 and c["plc_pitch_repeat"] == 10 and c["plc_noise"] == 2
    c, ln = _counts_of("dec_edge_40k_cbr_stream")
    assert c["plc_pitch_first"] == 4 and c["plc_pitch_repeat"] == 5 and c["plc_noise"] == 1
    assert c["plc_explosion_zeroed"] > 0 and c["plc_explosion_attenuated"] > 0


def test_one_byte_packets_other_than_dtx_of_this_configuration_are_not_concealed():
    pk = np.zeros((2, 8), np.uint8)
    pk[0, 0] = 0x78          # SILK-only TOC
    pk[1, 0] = 0xFD          # CELT FB 20 ms stereo, code 1
    pcm, rng, ret = plc_emulib.decode(pk, np.array([1, 1], np.int32), 1)
    assert ret.tolist() == [-5, -5]


def random_loss_mask(rs, nstreams, fps):
    """20 % single losses plus bursts of up to 12, per stream; True = lost."""
    m = rs.random((nstreams, fps)) < 0.2
    for s in range(nstreams):
        for _ in range(max(1, fps // 24)):
            a = int(rs.integers(0, fps))
            m[s, a:a + int(rs.integers(2, 13))] = True
    return m


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref is absent")
@pytest.mark.parametrize("kind,cfgvals,seed", [
    ("music", (32000, 1, 0, 10), 1), ("music", (64000, 1, 0, 10), 2), ("music", (96000, 0, 0, 10), 3),
    ("noise", (32000, 1, 1, 10), 4), ("noise", (64000, 1, 0, 10), 5), ("noise", (96000, 1, 0, 5), 6),
    ("edge", (32000, 0, 0, 5), 7), ("edge", (64000, 1, 0, 10), 8), ("edge", (96000, 1, 0, 10), 9),
    ("gmusic", (32000, 1, 1, 10), 10), ("gmusic", (64000, 1, 0, 10), 11), ("gmusic", (96000, 1, 0, 10), 12),
])
def test_emulated_concealment_matches_live_reference(kind, cfgvals, seed):
    gm = ec.golden_module()
    br, vbr, cvbr, cx = cfgvals
    nstreams, fps = 4, 48
    pk, ln, _rg = gm.ref_encode(gm._Cfg(2, br, vbr, cvbr, cx, 16, 0, 1500), gm.synth_pcm(kind, nstreams * fps, 9000 + seed), fps)
    pk = np.ascontiguousarray(pk[:, :int(ln.max())])
    ln = ln.astype(np.int32)
    ln[random_loss_mask(np.random.default_rng(seed), nstreams, fps).reshape(-1)] = 0
    want, wrng, wret = gm.ref_decode(pk, ln, fps)
    assert (wret == 960).all()
    pcm, rng, ret = plc_emulib.decode(pk, ln, fps)
    assert_frames_equal(pcm, rng, ret, want, wrng, ln, "%s %d" % (kind, br))
