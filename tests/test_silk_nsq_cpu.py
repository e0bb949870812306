"""CPU tier for silk_NSQ: the device source of the plain noise-shaping quantiser (concentus_amd/csrc/silk_nsq_dev.h:
silk_nsq_record_dev, the one call silk_nsq_kernel makes per record) compiled for the host (tests/emu, emu_silk_nsq) against
  a. the 80 records captured from the compiled reference (tests/golden/silk_golden.npz): pulses and every byte of silk_nsq_state;
  b. the short-lag / ragged-subframe corpus of tests/nsq_cases.py (the general path and its single-sample mode, which no captured
     record reaches) against the restatement in oracle/;
  c. the same corpus against silk_NSQ_c of the compiled reference, where oracle/_ref is built: the restatement had only been
     pinned on lags >= 36, so for the short lags the reference is the authority."""
import ctypes as C

import numpy as np
import pytest

import emulib
import nsq_cases
import oraclelib
import reflib

p = lambda a: a.ctypes.data_as(C.c_void_p)


def _run_emu(nsq_in, state_in):
    st = state_in.copy()
    out = np.zeros((nsq_in.shape[0], 320), np.uint8)
    emulib.lib().emu_silk_nsq(p(np.ascontiguousarray(nsq_in)), p(st), p(out), C.c_long(nsq_in.shape[0]))
    return out, st


def _assert_same(out, st, want_out, want_st, cls=None):
    bad = np.nonzero((out != want_out).any(1))[0]
    assert bad.size == 0, ("pulses differ", bad[:8], None if cls is None else [nsq_cases.CLASSES[c] for c in cls[bad[:8]]])
    bad = np.nonzero((st != want_st).any(1))[0]
    assert bad.size == 0, ("NSQ state differs", bad[:8], None if cls is None else [nsq_cases.CLASSES[c] for c in cls[bad[:8]]],
                           [np.nonzero(st[b] != want_st[b])[0][:6] for b in bad[:3]])


def test_nsq_source_matches_golden_records():
    g = np.load(nsq_cases.GOLD)
    out, st = _run_emu(g["silk_nsq_in"], g["silk_nsq_state_in"])
    _assert_same(out, st, g["silk_nsq_out"], g["silk_nsq_state_out"])


@pytest.fixture(scope="module")
def corpus():
    nsq_in, st_in, cls = nsq_cases.nsq_short_lag_corpus()
    assert nsq_cases.record_ok(nsq_in, st_in).all(), "a record that fails nsq_record_ok is skipped by the kernel and by emu_silk_nsq"
    out, st = _run_emu(nsq_in, st_in)
    return nsq_in, st_in, cls, out, st


def test_nsq_source_matches_the_oracle_on_short_lags_and_ragged_subframes(corpus):
    nsq_in, st_in, cls, out, st = corpus
    nsq_cases.check_nsq_corpus_reaches_every_path(nsq_in, st_in, cls)
    want_st = st_in.copy()
    want = np.zeros_like(out)
    oraclelib.lib().orc_silk_nsq_batch(p(nsq_in), p(want_st), p(want), nsq_in.shape[0])
    _assert_same(out, st, want, want_st, cls)


@pytest.mark.ref
def test_nsq_source_matches_the_reference_on_short_lags_and_ragged_subframes(corpus):
    if not reflib.available():
        pytest.skip("oracle/_ref/libopus_ref.so not built")
    nsq_in, st_in, cls, out, st = corpus
    fn = reflib.lib().silk_NSQ_c
    want_st = st_in.copy()
    want = np.zeros((nsq_in.shape[0], 320), np.int8)
    for k in range(nsq_in.shape[0]):
        x_Q3, pred, ltp, ar2, harm, tilt, lf, gains, pitch = reflib.nsq_arrays(nsq_in[k])
        enc, idx, lam, ltps = reflib.nsq_ref_structs(nsq_in[k], None)
        fn(p(enc), p(want_st[k]), p(idx), p(x_Q3), p(want[k]), p(pred), p(ltp), p(ar2), p(harm), p(tilt), p(lf), p(gains), p(pitch),
           C.c_int(lam), C.c_int(ltps))
    _assert_same(out, st, want.view(np.uint8), want_st, cls)
