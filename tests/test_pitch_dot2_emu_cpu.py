"""CPU tier: the packed-pair pitch loops of the front half (celt_enc_front.h: the coarse search, remove_doubling's inner
products, the five-lag autocorrelation) in the host build of the sources (CA_HOST_EMU, LANES == 1) on pitched tones.
The CA_COUNT counters prove that the case set reaches what it is meant to reach -- inner products at odd half-rate
periods (two words + align) as well as even ones (one word), and the shifted (sh != 0) path of the autocorrelation --
and the packets are compared with the compiled reference where it is built."""
import ctypes as C

import numpy as np
import pytest

import emulib
import encode_cases as ec
import pitch_cases

CFG = (96000, 1, 0, 10)


def _counts(emu):
    buf = C.create_string_buffer(1 << 16)
    n = emu.emu_counts_dump(buf, len(buf))
    assert n >= 0
    return {l.split()[0]: (int(l.split()[1]), int(l.split()[2])) for l in buf.value.decode().splitlines()}


def _run_emu(pcm, fps, split):
    emu = emulib.lib()
    cfg = emulib.Config(2, CFG[0], CFG[1], CFG[2], CFG[3], 16, 0, 1500)
    n = pcm.shape[0]
    out = np.zeros((n, 1280), np.uint8)
    lens = np.zeros(n, np.int32)
    rng = np.zeros(n, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    st = emulib.fresh_states(n // fps) if fps > 1 else None
    fn = emu.emu_celt_encode_frames_split if split else emu.emu_celt_encode_frames
    emu.emu_counts_reset()
    fn(C.byref(cfg), p(st) if st is not None else None, p(np.ascontiguousarray(pcm)), n, fps, p(out), 1280, p(lens), p(rng))
    return (out, lens, rng), _counts(emu)


# name -> (pcm, frames per stream): independent first frames (zero history) and short streams (history, prev_period / prev_gain)
CASES = {
    "tones_indep": (pitch_cases.tones(16, 1, 50), 1),
    "tones_stream": (pitch_cases.tones(8, 3, 51), 3),
    "loud_indep": (pitch_cases.harmonic(pitch_cases.periods(8), 1, 32767, 52), 1),
    "soft_indep": (pitch_cases.harmonic(pitch_cases.periods(8), 1, 40, 53), 1),
    "flat_stream": (pitch_cases.flat_envelope([32, 50, 100, 167], 3), 3),
}


@pytest.fixture(scope="module")
def runs():
    return {(name, split): _run_emu(pcm, fps, split) for name, (pcm, fps) in CASES.items() for split in (False, True)}


@pytest.mark.parametrize("name", list(CASES))
def test_inner_products_run_at_odd_and_even_periods(runs, name):
    for split in (False, True):
        cnt = runs[(name, split)][1]
        odd, even = cnt.get("pitch.lag_odd", (0, 0))[0], cnt.get("pitch.lag_even", (0, 0))[0]
        assert odd > 0 and even > 0, (name, split, odd, even)
        assert odd + even >= 4 * CASES[name][0].shape[0]      # at least T0 and the three xc[] lags of every frame


def test_shifted_autocorrelation_is_reached(runs):
    """sh != 0 in _celt_autocorr: every stream of flat_stream gets there in its later frames (pitch_cases.flat_envelope
    says why nothing else does); amplitude <= 40 never does."""
    for split in (False, True):
        assert runs[("flat_stream", split)][1].get("pitch.autocorr_shifted", (0, 0))[0] >= 4
        assert "pitch.autocorr_shifted" not in runs[("soft_indep", split)][1]


@pytest.mark.parametrize("name", list(CASES))
def test_whole_front_and_split_pipeline_agree(runs, name):
    a, b = runs[(name, False)][0], runs[(name, True)][0]
    ec.assert_packets_equal(a[0], a[1], a[2], b[0], b[1], b[2], name)


@pytest.mark.ref
@pytest.mark.parametrize("name", list(CASES))
def test_emulated_pitch_loops_match_live_reference(runs, name):
    gm = ec.golden_module()
    pcm, fps = CASES[name]
    pk, ln, rg = gm.ref_encode(gm._Cfg(2, CFG[0], CFG[1], CFG[2], CFG[3], 16, 0, 1500), pcm, fps, threads=2)
    for split in (False, True):
        out, lens, rng = runs[(name, split)][0]
        ec.assert_packets_equal(out, lens, rng, pk, ln, rg, "%s split=%s" % (name, split))
