"""Short-lag / ragged-subframe records for the two noise-shaping quantisers -- TEST INFRASTRUCTURE shared by the CPU tier
(tests/test_silk_nsq_cpu.py) and the GPU tier (tests/test_silk_gpu.py).

The captured records (tests/golden/silk_golden.npz, silk_dd_golden.npz) all have subframes of 80 samples and voiced lags of
42 .. 276, so they only reach the plain quantiser's four-sample fast path and del_dec's full decision delay of 32. The records
here are the captured ones with HEADER fields overwritten (pitchL, subfr_length / frame_length, the state's lagPrev); the signals,
filters and gains stay as captured. No capture of the reference has such headers (its pitch analysis yields lags >= 2 ms), so
the expected outputs come from the quantisers' restatement in oracle/ and, where it is built, the compiled reference itself.

Which path of silk_nsq_record_dev (concentus_amd/csrc/silk_nsq_dev.h) a subframe takes is a pure function of its lag (pitchL[k]
when voiced, else lagPrev) and subfr_length: paths() restates that rule so the tests can assert that every path is reached."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "silk_golden.npz")
GOLD_DD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "silk_dd_golden.npz")
LAGPREV = 4356                      # byte offset of opusgpu_nsq_state.lagPrev
CLASSES = ("voiced_lag_3_7", "voiced_lag_8_11", "voiced_subfr_78", "voiced_subfr_79", "unvoiced_lagprev_5", "unvoiced_lagprev_0", "captured")
PER_CLASS = 10


def header(nsq_in):
    """int32 view of the scalar fields: nb_subfr, subfr_length, frame_length, ltp_mem_length, predictLPCOrder, shapingLPCOrder,
    signalType, quantOffsetType, NLSFInterpCoef_Q2, Seed, Lambda_Q10, LTP_scale_Q14, then five arrays of four (pitchL = [28:32])."""
    return nsq_in[:, :128].view(np.int32)


def lag_prev(state):
    return state[:, LAGPREV:LAGPREV + 4].view(np.int32)[:, 0]


def record_ok(nsq_in, state):
    """nsq_record_ok of concentus_amd/csrc/silk_validate.h, per record."""
    h, lp = header(nsq_in), lag_prev(state)
    n, L, fl, ltp, po, so, sig, qo = (h[:, j] for j in range(8))
    ok = (n >= 1) & (n <= 4) & (L >= 1) & (L <= 80) & (fl == n * L) & (ltp >= 1) & (ltp <= 320) & (po >= 2) & (po <= 16)
    ok &= (so >= 2) & (so <= 16) & (so % 2 == 0) & (sig >= 0) & (sig <= 2) & (qo >= 0) & (qo <= 1) & (lp >= 0) & (lp <= ltp)
    for k in range(4):
        lag = h[:, 28 + k]
        ok &= ~((sig == 2) & (k < n)) | ((lag >= 3) & (ltp - lag - po - 2 > 0))
    return ok


def paths(nsq_in, state):
    """Per record, the set of paths its subframes take: 'fast' (groups of four, compile-time windows), 'general4' (shifting
    histories, groups of four, ragged tail), 'single' (one sample per group, taps re-read behind the fences)."""
    h, lp = header(nsq_in), lag_prev(state)
    out = []
    for r in range(h.shape[0]):
        L, got = int(h[r, 1]), set()
        for k in range(int(h[r, 0])):
            lag = int(h[r, 28 + k]) if h[r, 6] == 2 else int(lp[r])
            if (lag <= 0 or lag >= 12) and L % 4 == 0:
                got.add("fast")
            else:
                got.add("general4" if (lag >= 8 or lag <= 0) else "single")
        out.append(got)
    return out


def nsq_short_lag_corpus():
    """(nsq_in, state_in, class index per record): PER_CLASS derived records per class of CLASSES, then the 80 captured ones."""
    g = np.load(GOLD)
    gin, gst = g["silk_nsq_in"], g["silk_nsq_state_in"]
    sig = header(gin)[:, 6]
    voiced, unvoiced = np.nonzero(sig == 2)[0], np.nonzero(sig != 2)[0]
    assert voiced.size >= PER_CLASS and unvoiced.size >= PER_CLASS
    rng = np.random.default_rng(11)
    ins, sts, cls = [], [], []
    for c, name in enumerate(CLASSES[:-1]):
        pool = voiced if name.startswith("voiced") else unvoiced
        src = pool[np.linspace(0, pool.size - 1, PER_CLASS).astype(int)]
        a, s = gin[src].copy(), gst[src].copy()
        h = header(a)
        if name == "voiced_lag_3_7":
            h[:, 28:32] = rng.integers(3, 8, size=(PER_CLASS, 4))
            h[0, 28:32] = 3                                     # both ends of the range in every subframe
            h[1, 28:32] = 7
        elif name == "voiced_lag_8_11":
            h[:, 28:32] = rng.integers(8, 12, size=(PER_CLASS, 4))
            h[0, 28:32] = 8
            h[1, 28:32] = 11
        elif name in ("voiced_subfr_78", "voiced_subfr_79"):
            h[:, 1] = int(name[-2:])
            h[:, 2] = h[:, 0] * h[:, 1]
        elif name == "unvoiced_lagprev_5":
            lag_prev(s)[:] = 5
        else:
            lag_prev(s)[:] = 0
        ins.append(a); sts.append(s); cls += [c] * PER_CLASS
    ins.append(gin); sts.append(gst); cls += [len(CLASSES) - 1] * gin.shape[0]
    return np.ascontiguousarray(np.concatenate(ins)), np.ascontiguousarray(np.concatenate(sts)), np.array(cls)


def check_nsq_corpus_reaches_every_path(nsq_in, state, cls):
    """Every class is present and takes the path it is there for (computed from the headers alone)."""
    p = paths(nsq_in, state)
    want = {"voiced_lag_3_7": {"single"}, "voiced_lag_8_11": {"general4"}, "voiced_subfr_78": {"general4"}, "voiced_subfr_79": {"general4"},
            "unvoiced_lagprev_5": {"single"}, "unvoiced_lagprev_0": {"fast"}, "captured": {"fast"}}
    for c, name in enumerate(CLASSES):
        rows = np.nonzero(cls == c)[0]
        assert rows.size >= PER_CLASS, name
        assert all(p[r] == want[name] for r in rows), (name, [p[r] for r in rows[:4]])
    h = header(nsq_in)
    assert {78, 79, 80} <= set(h[:, 1].tolist()) and (h[h[:, 1] == 78, 2] == 312).all()


def dd_short_delay_corpus(n=133):
    """(dd_in, state_in): the 84 captured del_dec records with the voiced lags overwritten to 4 .. 11 (decision delay = lag - 3 = 1 .. 8
    instead of 32), tiled to n records (n = 133: a ragged last workgroup of 16)."""
    g = np.load(GOLD_DD)
    din, st = g["silk_dd_in"].copy(), g["silk_dd_state_in"].copy()
    h = header(din)
    v = np.nonzero(h[:, 6] == 2)[0]
    assert v.size >= 8
    rng = np.random.default_rng(12)
    h[v, 28:32] = rng.integers(4, 12, size=(v.size, 4))
    for j in range(8):                                         # every delay 1 .. 8 as the frame's minimum
        h[v[j], 28:32] = np.maximum(h[v[j], 28:32], 4 + j)
        h[v[j], 28 + j % 4] = 4 + j
    delays = set((h[v, 28:32].min(1) - 3).tolist())
    assert delays == set(range(1, 9)), delays
    reps = n // din.shape[0] + 1
    return np.ascontiguousarray(np.tile(din, (reps, 1))[:n]), np.ascontiguousarray(np.tile(st, (reps, 1))[:n])
