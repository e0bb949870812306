"""CPU tier: every per-call hook (include/opusgpu_hooks.h, and the five older ones of opusgpu.h / opusgpu_silk.h) rejects a bad
call on the host, before its first HIP call: the documented code in opusgpu_get_last_error(), the documented return value, and
every caller-owned buffer byte-for-byte as it was. One table row = one call; no row reaches a device allocation, so the file
needs no GPU."""
import ctypes as C
import os
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BAD_ARG, UNIMPLEMENTED = -1, -5

# include/opusgpu_hooks.h (pinned against the reference's headers by tests/test_hooks_layout.py)
SIZEOF_STATE_FIX, SIZEOF_CTRL_FIX, SIZEOF_INDICES = 9800, 552, 36
OFF = dict(fs_kHz=4600, nb_subfr=4604, frame_length=4608, subfr_length=4612, ltp_mem_length=4616, la_pitch=4620, la_shape=4624,
           predictLPCOrder=4664, prefill=4712, LBRR_enabled=6144, LP_mode=16 + 12)


def _lib():
    from concentus_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return lib.load()


class Buf:
    """A caller-owned buffer: `fill` bytes, optionally with little-endian fields packed at byte offsets."""

    def __init__(self, nbytes, fill=0xA5, fields=()):
        self.raw = (C.c_ubyte * nbytes)()
        C.memset(self.raw, fill, nbytes)
        for off, fmt, *vals in fields:
            struct.pack_into("<" + fmt, self.raw, off, *vals)

    def ptr(self, byte_off=0):
        return C.c_void_p(C.addressof(self.raw) + byte_off)


class At:
    """A pointer `byte_off` bytes into a Buf (x[-T-2] and friends must exist behind the pointer the hook is given)."""

    def __init__(self, buf, byte_off):
        self.buf, self.byte_off = buf, byte_off


def state(**f):
    """A zero-filled silk_encoder_state_FIX with the named silk_encoder_state fields set."""
    return Buf(SIZEOF_STATE_FIX, 0, [(OFF[k], "i", v) for k, v in f.items()])


def fft_cfg(nfft=480, scale=17476, scale_shift=8):
    return Buf(64, 0, [(0, "ihxxii", nfft, scale, scale_shift, 0)])           # head of kiss_fft_state


def mdct_lookup(n=1920, maxshift=3):
    return Buf(64, 0, [(0, "ii", n, maxshift)])                               # head of mdct_lookup


def celt_mode(Fs=48000, overlap=120, nbEBands=21):
    return Buf(64, 0, [(0, "iiii", Fs, overlap, nbEBands, 21)])               # head of CELTMode


def ec_ctx(buf, storage=1275, offs=0, end_offs=0):
    """The tree's ec_ctx (56 bytes on x86-64, trailing EC_DIFF included) on `buf` (None: a NULL buffer pointer)."""
    p = C.addressof(buf.raw) if buf is not None else 0
    return Buf(56, 0, [(0, "QIIIiiIIIIiii", p, storage, end_offs, 0, 0, 33, offs, 0x80000000, 0, 0, -1, 0, 0)])


def W(n=64):
    return Buf(n)


# ---- the table: id -> (function, builder of the argument list, code, return value or None) ----------------------------------
CASES = {}


def case(cid, fn, build, code, ret=None):
    assert cid not in CASES, cid
    CASES[cid] = (fn, build, code, ret)


def nulls(prefix, fn, build, positions, code=BAD_ARG, ret=None):
    """One row per pointer position: the valid call of `build` with that argument NULL."""
    for name, idx in positions.items():
        def b(idx=idx):
            a = build()
            a[idx] = None
            return a
        case("%s-null_%s" % (prefix, name), fn, b, code, ret)


def varied(prefix, fn, build, rows, code=BAD_ARG, ret=None):
    """One row per (name, keyword arguments of `build`)."""
    for name, kw in rows.items():
        case("%s-%s" % (prefix, name), fn, (lambda kw=kw: build(**kw)), code, ret)


# opus_fft / opus_ifft (cfg, fin, fout)
for _f in ("opusgpu_opus_fft", "opusgpu_opus_ifft"):
    _p = _f[len("opusgpu_"):]
    nulls(_p, _f, lambda: [fft_cfg(), W(3840), W(3840)], dict(cfg=0, fin=1, fout=2))
    case(_p + "-bad_head", _f, lambda: [Buf(64, 0), W(3840), W(3840)], BAD_ARG)
    case(_p + "-bad_scale_shift", _f, lambda: [fft_cfg(240, 17476, 8), W(3840), W(3840)], BAD_ARG)

    def _in_place():
        b = W(3840)
        return [fft_cfg(), b, b]
    case(_p + "-in_place", _f, _in_place, BAD_ARG)


# clt_mdct_forward / _backward (l, in, out, window, overlap, shift, stride, arch)
def _mdct(l=None, overlap=120, shift=0, stride=1):
    return [l or mdct_lookup(), W(4320), W(4320), W(240), overlap, shift, stride, 0]


for _f in ("opusgpu_clt_mdct_forward", "opusgpu_clt_mdct_backward"):
    _p = _f[len("opusgpu_"):]
    nulls(_p, _f, _mdct, dict(l=0, window=3))
    varied(_p, _f, _mdct, dict(overlap_119=dict(overlap=119), overlap_0=dict(overlap=0), shift_neg=dict(shift=-1), shift_4=dict(shift=4),
                               stride_0=dict(stride=0), lookup_n=dict(l=mdct_lookup(960, 3)), lookup_maxshift=dict(l=mdct_lookup(1920, 2)),
                               lookup_zero=dict(l=Buf(64, 0))))


# celt_pitch_xcorr (x, y, xcorr, len, max_pitch, arch) -> 0 on failure
def _xcorr(len_=64, max_pitch=16):
    return [W(4096), W(8192), W(64), len_, max_pitch, 0]


nulls("celt_pitch_xcorr", "opusgpu_celt_pitch_xcorr", _xcorr, dict(x=0, y=1, xcorr=2), ret=0)
varied("celt_pitch_xcorr", "opusgpu_celt_pitch_xcorr", _xcorr,
       dict(len_0=dict(len_=0), len_2049=dict(len_=2049), max_pitch_0=dict(max_pitch=0)), ret=0)


# silk_burg_modified_c (res_nrg, res_nrg_Q, A_Q16, x, minInvGain_Q30, subfr_length, nb_subfr, D, arch)
def _burg(subfr_length=80, nb_subfr=4, D=16):
    return [W(4), W(4), W(64), W(768), 1 << 20, subfr_length, nb_subfr, D, 0]


nulls("silk_burg_modified_c", "opusgpu_silk_burg_modified_c", _burg, dict(res_nrg=0, res_nrg_Q=1, A_Q16=2, x=3))
varied("silk_burg_modified_c", "opusgpu_silk_burg_modified_c", _burg,
       dict(D_0=dict(D=0), D_17=dict(D=17), nb_subfr_0=dict(nb_subfr=0), subfr_le_D=dict(subfr_length=16),
            too_long=dict(subfr_length=97)))


# comb_filter_const (y, x, T, N, g10, g11, g12): x is preceded by T + 2 samples
def _comb(T=15, N=64, y_off=None):
    xb = Buf(4 * (8192 + 4200))
    y = W(4 * 8192) if y_off is None else At(xb, 4 * (4100 + y_off))
    return [y, At(xb, 4 * 4100), T, N, 9000, 6000, 3000]


nulls("comb_filter_const", "opusgpu_comb_filter_const", _comb, dict(y=0, x=1))
varied("comb_filter_const", "opusgpu_comb_filter_const", _comb,
       dict(N_0=dict(N=0), N_8193=dict(N=8193), T_2=dict(T=2), T_4097=dict(T=4097), overlap_ahead=dict(y_off=1),
            overlap_behind=dict(y_off=-3), overlap_history=dict(y_off=-64 - 10)))


# exp_rotation1 (X, len, stride, c, s)
def _rot(len_=64, stride=4):
    return [W(8194), len_, stride, 30000, 12000]


nulls("exp_rotation1", "opusgpu_exp_rotation1", _rot, dict(X=0))
varied("exp_rotation1", "opusgpu_exp_rotation1", _rot,
       dict(len_1=dict(len_=1), len_4097=dict(len_=4097), stride_0=dict(stride=0), stride_eq_len=dict(stride=64),
            stride_gt_len=dict(stride=65)))


# renormalise_vector (X, N, gain, arch)
def _renorm(N=64):
    return [W(8194), N, 32767, 0]


nulls("renormalise_vector", "opusgpu_renormalise_vector", _renorm, dict(X=0))
varied("renormalise_vector", "opusgpu_renormalise_vector", _renorm, dict(N_0=dict(N=0), N_4097=dict(N=4097)))


# silk_NSQ / silk_NSQ_del_dec (psEncC, NSQ, psIndices, x_Q3, pulses, PredCoef_Q12, LTPCoef_Q14, AR2_Q13, HarmShapeGain_Q14, Tilt_Q14,
# LF_shp_Q14, Gains_Q16, pitchL, Lambda_Q10, LTP_scale_Q14)
def _nsq(nb_subfr=4, frame_length=320):
    return [state(nb_subfr=nb_subfr, frame_length=frame_length, subfr_length=80, ltp_mem_length=320, predictLPCOrder=16),
            W(8192), Buf(SIZEOF_INDICES, 0), W(1280), W(320), W(64), W(40), W(128), W(16), W(16), W(16), W(16), W(16), 100, 16384]


_NSQ_PTRS = dict(psEncC=0, NSQ=1, psIndices=2, x_Q3=3, pulses=4, PredCoef_Q12=5, LTPCoef_Q14=6, AR2_Q13=7, HarmShapeGain_Q14=8,
                 Tilt_Q14=9, LF_shp_Q14=10, Gains_Q16=11, pitchL=12)
for _f in ("opusgpu_silk_NSQ", "opusgpu_silk_NSQ_del_dec"):
    _p = _f[len("opusgpu_"):]
    nulls(_p, _f, _nsq, _NSQ_PTRS)
    varied(_p, _f, _nsq, dict(nb_subfr_0=dict(nb_subfr=0), nb_subfr_5=dict(nb_subfr=5), frame_length_0=dict(frame_length=0),
                              frame_length_321=dict(frame_length=321)))


# quant_all_bands (encode, m, start, end, X, Y, collapse_masks, bandE, pulses, shortBlocks, spread, dual_stereo, intensity, tf_res,
# total_bits, balance, ec, LM, codedBands, seed, arch)
def _qab(encode=1, m=None, start=0, end=21, LM=3, shortBlocks=0, storage=1275, ec_buf=True):
    ec = ec_ctx(W(1280) if ec_buf else None, storage)
    return [encode, m or celt_mode(), start, end, W(1920), W(1920), W(48), W(168), W(84), shortBlocks, 2, 0, 21, W(84), 8000, 0, ec,
            LM, 21, W(4), 0]


_QAB_PTRS = dict(m=1, X=4, bandE=7, pulses=8, tf_res=13, ec=16)
nulls("quant_all_bands-enc", "opusgpu_quant_all_bands", _qab, _QAB_PTRS)
nulls("quant_all_bands-enc", "opusgpu_quant_all_bands", _qab, dict(Y=5), code=UNIMPLEMENTED)
nulls("quant_all_bands-dec", "opusgpu_quant_all_bands", lambda: _qab(encode=0), dict(m=1, X=4, pulses=8, tf_res=13, ec=16, collapse_masks=6, seed=19))
nulls("quant_all_bands-dec", "opusgpu_quant_all_bands", lambda: _qab(encode=0), dict(Y=5), code=UNIMPLEMENTED)
for _e in (0, 1):
    varied("quant_all_bands-%s" % ("enc" if _e else "dec"), "opusgpu_quant_all_bands", (lambda _e=_e, **kw: _qab(encode=_e, **kw)),
           dict(start_1=dict(start=1), end_20=dict(end=20), LM_2=dict(LM=2), LM_0=dict(LM=0), Fs_44100=dict(m=celt_mode(Fs=44100)),
                overlap_240=dict(m=celt_mode(overlap=240)), nbEBands_20=dict(m=celt_mode(nbEBands=20)), storage_1276=dict(storage=1276),
                ec_buf_null=dict(ec_buf=False), shortBlocks_4=dict(shortBlocks=4)), code=UNIMPLEMENTED)
case("quant_all_bands-encode_2", "opusgpu_quant_all_bands", lambda: _qab(encode=2), UNIMPLEMENTED)


# ec_enc_script (ec, ops, n_ops) / ec_dec_script (ec, ops, n_ops, out): the code is also the return value
def _ecs(decode, n=4, storage=1280, ec_buf=True):
    a = [ec_ctx(W(1280) if ec_buf else None, storage), W(64), n]
    return a + [W(16)] if decode else a


for _d, _f in ((0, "opusgpu_ec_enc_script"), (1, "opusgpu_ec_dec_script")):
    _p = _f[len("opusgpu_"):]
    nulls(_p, _f, (lambda _d=_d: _ecs(_d)), dict(ec=0, ops=1, **(dict(out=3) if _d else {})), ret=BAD_ARG)
    varied(_p, _f, (lambda _d=_d, **kw: _ecs(_d, **kw)), dict(ec_buf_null=dict(ec_buf=False), n_neg=dict(n=-1)), ret=BAD_ARG)
    varied(_p, _f, (lambda _d=_d, **kw: _ecs(_d, **kw)), dict(storage_1281=dict(storage=1281), n_65537=dict(n=65537)),
           code=UNIMPLEMENTED, ret=UNIMPLEMENTED)


# silk_find_LPC_FIX (psEncC, NLSF_Q15, x, minInvGain_Q30)
def _find_lpc(**f):
    g = dict(nb_subfr=4, subfr_length=80, predictLPCOrder=16)
    g.update(f)
    return [state(**g), W(32), W(1024), 1 << 20]


nulls("silk_find_LPC_FIX", "opusgpu_silk_find_LPC_FIX", _find_lpc, dict(psEncC=0, NLSF_Q15=1, x=2))
varied("silk_find_LPC_FIX", "opusgpu_silk_find_LPC_FIX", _find_lpc,
       dict(nb_subfr_0=dict(nb_subfr=0), subfr_length_0=dict(subfr_length=0), order_0=dict(predictLPCOrder=0), too_long=dict(nb_subfr=5)))


# silk_process_NLSFs (psEncC, PredCoef_Q12, pNLSF_Q15, prev_NLSFq_Q15)
def _nlsf(order=16):
    return [state(nb_subfr=4, predictLPCOrder=order), W(64), W(32), W(32)]


nulls("silk_process_NLSFs", "opusgpu_silk_process_NLSFs", _nlsf, dict(psEncC=0, PredCoef_Q12=1, pNLSF_Q15=2, prev_NLSFq_Q15=3))
varied("silk_process_NLSFs", "opusgpu_silk_process_NLSFs", _nlsf, dict(order_0=dict(order=0), order_12=dict(order=12), order_17=dict(order=17)))


# silk_residual_energy_FIX (nrgs, nrgsQ, x, a_Q12, gains, subfr_length, nb_subfr, LPC_order, arch)
def _res_nrg(subfr_length=80, nb_subfr=4, order=16):
    return [W(16), W(16), W(1024), W(64), W(16), subfr_length, nb_subfr, order, 0]


nulls("silk_residual_energy_FIX", "opusgpu_silk_residual_energy_FIX", _res_nrg, dict(nrgs=0, nrgsQ=1, x=2, a_Q12=3, gains=4))
varied("silk_residual_energy_FIX", "opusgpu_silk_residual_energy_FIX", _res_nrg,
       dict(nb_subfr_3=dict(nb_subfr=3), nb_subfr_1=dict(nb_subfr=1), subfr_length_0=dict(subfr_length=0), order_1=dict(order=1),
            order_17=dict(order=17), too_long=dict(subfr_length=100)))


# silk_find_pred_coefs_FIX (psEnc, psEncCtrl, res_pitch, x, condCoding): x is preceded by ltp_mem_length samples
def _pred(**f):
    g = dict(nb_subfr=4, subfr_length=80, predictLPCOrder=16, ltp_mem_length=320)
    g.update(f)
    xb = Buf(2 * 1024)
    return [state(**g), Buf(SIZEOF_CTRL_FIX), W(1280), At(xb, 2 * 512), 0]


nulls("silk_find_pred_coefs_FIX", "opusgpu_silk_find_pred_coefs_FIX", _pred, dict(psEnc=0, psEncCtrl=1, res_pitch=2, x=3))
varied("silk_find_pred_coefs_FIX", "opusgpu_silk_find_pred_coefs_FIX", _pred,
       dict(nb_subfr_3=dict(nb_subfr=3), subfr_length_0=dict(subfr_length=0), subfr_length_81=dict(subfr_length=81),
            order_12=dict(predictLPCOrder=12), ltp_below_order=dict(ltp_mem_length=15), ltp_321=dict(ltp_mem_length=321)))


# silk_find_pitch_lags_FIX (psEnc, psEncCtrl, res, x, arch): x is preceded by ltp_mem_length samples
def _pitch(**f):
    g = dict(fs_kHz=16, nb_subfr=4, frame_length=320, ltp_mem_length=320, la_pitch=32)
    g.update(f)
    xb = Buf(2 * 1024)
    return [state(**g), Buf(SIZEOF_CTRL_FIX), W(1344), At(xb, 2 * 512), 0]


nulls("silk_find_pitch_lags_FIX", "opusgpu_silk_find_pitch_lags_FIX", _pitch, dict(psEnc=0, psEncCtrl=1, res=2, x=3))
varied("silk_find_pitch_lags_FIX", "opusgpu_silk_find_pitch_lags_FIX", _pitch,
       dict(la_pitch_neg=dict(la_pitch=-1), frame_length_neg=dict(frame_length=-1), ltp_neg=dict(ltp_mem_length=-1),
            too_long=dict(la_pitch=33)))


# silk_noise_shape_analysis_FIX (psEnc, psEncCtrl, pitch_res, x, arch): x is preceded by la_shape samples
def _shape(**f):
    g = dict(fs_kHz=16, nb_subfr=4, subfr_length=80, la_shape=80)
    g.update(f)
    xb = Buf(2 * 1024)
    return [state(**g), Buf(SIZEOF_CTRL_FIX), W(640), At(xb, 2 * 256), 0]


nulls("silk_noise_shape_analysis_FIX", "opusgpu_silk_noise_shape_analysis_FIX", _shape, dict(psEnc=0, psEncCtrl=1, pitch_res=2, x=3))
varied("silk_noise_shape_analysis_FIX", "opusgpu_silk_noise_shape_analysis_FIX", _shape,
       dict(nb_subfr_0=dict(nb_subfr=0), subfr_length_0=dict(subfr_length=0), la_shape_neg=dict(la_shape=-1), la_shape_81=dict(la_shape=81),
            too_long=dict(subfr_length=81)))

# silk_process_gains_FIX (psEnc, psEncCtrl, condCoding)
nulls("silk_process_gains_FIX", "opusgpu_silk_process_gains_FIX", lambda: [state(nb_subfr=4, subfr_length=80), Buf(SIZEOF_CTRL_FIX), 0],
      dict(psEnc=0, psEncCtrl=1))


# silk_prefilter_FIX (psEnc, psEncCtrl, xw_Q3, x)
def _prefilter(**f):
    g = dict(nb_subfr=4, subfr_length=80)
    g.update(f)
    return [state(**g), Buf(SIZEOF_CTRL_FIX), W(1280), W(640)]


nulls("silk_prefilter_FIX", "opusgpu_silk_prefilter_FIX", _prefilter, dict(psEnc=0, psEncCtrl=1, xw_Q3=2, x=3))
varied("silk_prefilter_FIX", "opusgpu_silk_prefilter_FIX", _prefilter,
       dict(nb_subfr_0=dict(nb_subfr=0), subfr_length_0=dict(subfr_length=0), too_long=dict(subfr_length=81)))


# silk_VAD_GetSA_Q8_c (psEncC, pIn) -> -1 on failure
def _vad(frame_length=320):
    return [state(fs_kHz=16, frame_length=frame_length), W(640)]


nulls("silk_VAD_GetSA_Q8_c", "opusgpu_silk_VAD_GetSA_Q8_c", _vad, dict(psEncC=0, pIn=1), ret=-1)
varied("silk_VAD_GetSA_Q8_c", "opusgpu_silk_VAD_GetSA_Q8_c", _vad, dict(frame_length_7=dict(frame_length=7), frame_length_321=dict(frame_length=321)),
       ret=-1)


# silk_encode_indices (psEncC, psRangeEnc, FrameIndex, encode_LBRR, condCoding)
def _indices(encode_LBRR=0):
    return [state(fs_kHz=16, nb_subfr=4, frame_length=320, predictLPCOrder=16), ec_ctx(W(1280), 1280), 0, encode_LBRR, 0]


nulls("silk_encode_indices", "opusgpu_silk_encode_indices", _indices, dict(psEncC=0, psRangeEnc=1))
case("silk_encode_indices-encode_LBRR_1", "opusgpu_silk_encode_indices", lambda: _indices(1), UNIMPLEMENTED)


# silk_encode_pulses (psRangeEnc, signalType, quantOffsetType, pulses, frame_length)
def _pulses(frame_length=320):
    return [ec_ctx(W(1280), 1280), 2, 0, W(320), frame_length]


nulls("silk_encode_pulses", "opusgpu_silk_encode_pulses", _pulses, dict(psRangeEnc=0, pulses=3))
varied("silk_encode_pulses", "opusgpu_silk_encode_pulses", _pulses, dict(frame_length_0=dict(frame_length=0), frame_length_321=dict(frame_length=321)))


# silk_encode_frame_FIX (psEnc, pnBytesOut, psRangeEnc, condCoding, maxBits, useCBR) -> -1 on failure
def _frame(**f):
    g = dict(fs_kHz=16, nb_subfr=4, frame_length=320, ltp_mem_length=320, la_pitch=32)
    g.update(f)
    return [state(**g), W(4), ec_ctx(W(1280), 1280), 0, 1000, 0]


nulls("silk_encode_frame_FIX", "opusgpu_silk_encode_frame_FIX", _frame, dict(psEnc=0, pnBytesOut=1, psRangeEnc=2), ret=-1)
varied("silk_encode_frame_FIX", "opusgpu_silk_encode_frame_FIX", _frame,
       dict(fs_24=dict(fs_kHz=24), fs_0=dict(fs_kHz=0), nb_subfr_3=dict(nb_subfr=3), frame_length_mismatch=dict(frame_length=160),
            ltp_mismatch=dict(ltp_mem_length=160), la_pitch_neg=dict(la_pitch=-1), la_pitch_33=dict(la_pitch=33)), ret=-1)
varied("silk_encode_frame_FIX", "opusgpu_silk_encode_frame_FIX", _frame,
       dict(lp_mode=dict(LP_mode=1), lbrr=dict(LBRR_enabled=1), fs_12=dict(fs_kHz=12, frame_length=240, ltp_mem_length=240, la_pitch=24)),
       code=UNIMPLEMENTED, ret=-1)


def _set_last_error(L, code):
    """Leaves `code` as the thread's last error, through the public entry points only."""
    if code == BAD_ARG:
        L.opusgpu_exp_rotation1(None, 0, 0, 0, 0)
    else:
        a = _indices(1)
        L.opusgpu_silk_encode_indices(a[0].ptr(), a[1].ptr(), 0, 1, 0)
    assert L.opusgpu_get_last_error() == code


@pytest.mark.parametrize("cid", sorted(CASES))
def test_hook_rejects_before_touching_the_device(cid):
    L = _lib()
    fn, build, code, ret = CASES[cid]
    args = build()
    bufs, seen = [], set()

    def own(b):
        if id(b) not in seen:
            seen.add(id(b))
            bufs.append(b)

    call = []
    for a in args:
        if isinstance(a, At):
            own(a.buf)
            call.append(a.buf.ptr(a.byte_off))
        elif isinstance(a, Buf):
            own(a)
            call.append(a.ptr())
        else:
            call.append(a)
    before = [bytes(b.raw) for b in bufs]
    _set_last_error(L, UNIMPLEMENTED if code == BAD_ARG else BAD_ARG)       # the call must SET the code, not inherit it
    got = getattr(L, fn)(*call)
    assert L.opusgpu_get_last_error() == code
    if ret is not None:
        assert got == ret
    assert [bytes(b.raw) for b in bufs] == before, "a rejected call wrote to a caller's buffer"


def test_table_covers_every_hook():
    """Every entry point of include/opusgpu_hooks.h and the five older per-call hooks has rows in the table."""
    import re
    src = open(os.path.join(ROOT, "include", "opusgpu_hooks.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    hooks = set(re.findall(r"\b(opusgpu_\w+)\s*\(", src))
    hooks |= {"opusgpu_opus_fft", "opusgpu_clt_mdct_forward", "opusgpu_clt_mdct_backward", "opusgpu_celt_pitch_xcorr",
              "opusgpu_silk_burg_modified_c"}
    assert hooks == {fn for fn, _, _, _ in CASES.values()}
