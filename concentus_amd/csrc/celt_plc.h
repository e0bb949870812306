// celt_plc.h -- packet loss concealment of the batched decoder: celt_decode_lost (opus-fix/celt/celt_decoder.c:395-711) as
// celt_decode_with_ec calls it for data == NULL / len <= 1 (:827-833), under the Opus layer's handling of a lost packet
// (src/opus_decoder.c:246-267: no packet decoded yet -> zeros; :579-580: final range 0), for 48 kHz stereo 20 ms frames.
//
// Two stages. celt_plc_wave (one wavefront per stream; LANES == 1 in the host emulation) does everything with parallelism
// inside a frame: the pitch search on the first loss (pitch_downsample + pitch_search, pitch.c:147-369), the windowed
// autocorrelation and Levinson recursion of order 24 (celt_lpc.c:37-92, :232-328), the excitation (celt_fir), the decay estimate,
// the history move and the periodic extrapolation; or, from the sixth loss in a row, the noise fill of the normalised bands, which
// the ordinary synthesis (celt_decode_synth) then turns into a frame. celt_plc_tail_channel (one lane per stream and channel) is
// what remains of the pitch-based branch: celt_iir -- its fed-back sample is rounded to 16 bits, so it is a true recurrence --,
// the explosion check, the pre-filter on the overlap and the TDAC fold. De-emphasis follows as for a received frame.
// Every accumulation of the reference is a wrapping 32-bit add, so the lane-strided sums below are bit-exact in any order.
#pragma once
#include "celt_dec.h"

namespace ca {

enum { PLC_LAG_MAX = 720, PLC_LAG_MIN = 100, LPC_ORD = OPUSGPU_CELT_LPC_ORDER, PLC_EXT = FRAME + OVL };
enum { PLC_PS_LEN = DEC_BUF - PLC_LAG_MAX, PLC_PS_LAGS = PLC_LAG_MAX - PLC_LAG_MIN, PLC_PS_LAG = PLC_PS_LEN + PLC_PS_LAGS };
static_assert(DEC_MEM == DEC_BUF - FRAME + PLC_EXT, "the extrapolation fills decode_mem to its end");
static_assert(PLC_EXT % LPC_ORD == 0, "celt_plc_tail_channel walks the extrapolation in blocks of LPC_ORD samples");

// working set of celt_plc_wave (LDS of the wavefront; host memory in the emulation), 9.5 KB
struct __attribute__((aligned(16))) PlcLds {
    i16 xin[LPC_ORD + MAXP];             // ROUND16 of decode_mem[DEC_BUF - MAXP - LPC_ORD ..): the FIR's history, then the raw exc
    i16 exc[MAXP];                       // the windowed copy the autocorrelation reads, then the excitation (celt_fir's output)
    i16 lp[DEC_BUF >> 1];                // celt_plc_pitch_search's lp_pitch_buf
    i16 x4[PLC_PS_LEN >> 2], y4[(PLC_PS_LAG >> 2) + 1];
    i32 xcorr[PLC_PS_LAGS >> 1];
    i32 ac[LPC_ORD + 1];
    i32 lpc32[2][LPC_ORD];               // _celt_lpc's 32-bit coefficients, old and new of one recursion step
    i16 lpc16[LPC_ORD];
    i16 att[PLC_EXT / PLC_LAG_MIN + 2];  // attenuation of the extrapolation's period p
};

// pitch_downsample(decode_mem, lp, 2048, C = 2)  (pitch.c:147-217); the arithmetic of pitch_downsample_wave (celt_enc_front.h) on
// the decoder's history instead of the encoder's pre-filter memory
template <class L>
CA_DEVFN void plc_pitch_downsample(L &P, const opusgpu_celt_dec_state *st)
{
    const int len = DEC_BUF, n = len >> 1, lag = 4;
    i16 *x_lp = P.lp;
    i32 mx = 0, mn = 0;
    for (int c = 0; c < 2; c++)
        for (int k = lane(); k < len; k += LANES) {
            i32 v = st->decode_mem[c][k];
            mx = imax(mx, v);
            mn = imin(mn, v);
        }
    i32 maxabs = imax(wave_max(mx), neg32(wave_min(mn)));
    if (maxabs < 1) maxabs = 1;
    int shift = celt_ilog2(maxabs) - 10;
    if (shift < 0) shift = 0;
    shift++;                                                                       // C == 2
    for (int i = lane(); i < n; i += LANES) {
        i32 acc = 0;
        for (int c = 0; c < 2; c++) {
            const i32 *x = st->decode_mem[c];
            i32 v;
            if (i == 0) v = (add32(x[1] >> 1, x[0]) >> 1) >> shift;
            else v = (add32(add32(x[2 * i - 1], x[2 * i + 1]) >> 1, x[2 * i]) >> 1) >> shift;
            acc = c == 0 ? (i16)v : (i16)(acc + v);                               // x_lp is opus_val16
        }
        x_lp[i] = (i16)acc;
    }
    wave_sync();
    // _celt_autocorr(x_lp, ac, NULL, 0, 4, n)  (celt_lpc.c:232-328), overlap == 0
    i32 part = 0;
    for (int i = lane(); i < n; i += LANES) part = add32(part, mul16_16(x_lp[i], x_lp[i]) >> 9);
    i32 ac0 = add32(1 + (n << 7), wave_add(part));
    int sh = (celt_ilog2(ac0) - 30 + 10) / 2;
    if (sh <= 0) sh = 0;
    i32 ac[5];
    for (int k = 0; k <= lag; k++) {
        i32 p = 0;
        for (int i = lane(); i + k < n; i += LANES) {
            i32 a = sh ? (i16)pshr32(x_lp[i], sh) : x_lp[i];
            i32 b = sh ? (i16)pshr32(x_lp[i + k], sh) : x_lp[i + k];
            p = mac16_16(p, a, b);
        }
        ac[k] = wave_add(p);
    }
    if (2 * sh <= 0) ac[0] = add32(ac[0], 1);
    if (ac[0] < 268435456) {
        int s2 = 29 - ec_ilog((u32)ac[0]);
        for (int k = 0; k <= lag; k++) ac[k] = shl32(ac[k], s2);
    } else if (ac[0] >= 536870912) {
        int s2 = 1;
        if (ac[0] >= 1073741824) s2++;
        for (int k = 0; k <= lag; k++) ac[k] = ac[k] >> s2;
    }
    ac[0] = add32(ac[0], ac[0] >> 13);
    for (int i = 1; i <= 4; i++) ac[i] = sub32(ac[i], mul16_32_q15(2 * i * i, ac[i]));
    i32 lpc32[4] = {0, 0, 0, 0};
    i32 err = ac[0];
    if (ac[0] != 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            i32 rr = 0;
#pragma unroll
            for (int j = 0; j < i; j++) rr = add32(rr, mul32_32_q31(lpc32[j], ac[i - j]));
            rr = add32(rr, ac[i + 1] >> 3);
            i32 r = neg32(frac_div32(shl32(rr, 3), err));
            lpc32[i] = r >> 3;
#pragma unroll
            for (int j = 0; j < ((i + 1) >> 1); j++) {
                i32 t1 = lpc32[j], t2 = lpc32[i - 1 - j];
                lpc32[j] = add32(t1, mul32_32_q31(r, t2));
                lpc32[i - 1 - j] = add32(t2, mul32_32_q31(r, t1));
            }
            err = sub32(err, mul32_32_q31(mul32_32_q31(r, r), err));
            if (err < (ac[0] >> 10)) break;
        }
    }
    i32 lpc[4], tmp = 32767;
    for (int i = 0; i < 4; i++) {
        i32 l = (i16)pshr32(lpc32[i], 16);
        tmp = (i16)mul16_16_q15(29491, tmp);
        lpc[i] = (i16)mul16_16_q15(l, tmp);
    }
    const i32 c1 = 26214;
    i32 num[5];
    num[0] = (i16)(lpc[0] + 3277);
    num[1] = (i16)(lpc[1] + mul16_16_q15(c1, lpc[0]));
    num[2] = (i16)(lpc[2] + mul16_16_q15(c1, lpc[1]));
    num[3] = (i16)(lpc[3] + mul16_16_q15(c1, lpc[2]));
    num[4] = (i16)mul16_16_q15(c1, lpc[3]);
    // celt_fir5 in place, zero initial memory: chunks from the end, so that the taps are still unfiltered when read
    for (int base = ((n - 1) / LANES) * LANES; base >= 0; base -= LANES) {
        int i = base + lane();
        i32 y = 0;
        if (i < n) {
            i32 sum = shl32(x_lp[i], 12);
#pragma unroll
            for (int k = 0; k < 5; k++) {
                i32 xm = i - 1 - k >= 0 ? x_lp[i - 1 - k] : 0;
                sum = mac16_16(sum, num[k], xm);
            }
            y = (i16)pshr32(sum, 12);
        }
        wave_sync();
        if (i < n) x_lp[i] = (i16)y;
        wave_sync();
    }
}

// pitch_search(lp + 360, lp, 1328, 620)  (pitch.c:260-369): 155 lags at a quarter of the rate, then the lags within two of the best
// two at half the rate
template <class L>
CA_DEVFN int plc_pitch_search(L &P)
{
    const int len = PLC_PS_LEN, max_pitch = PLC_PS_LAGS, lag = PLC_PS_LAG;
    const i16 *y = P.lp, *x_lp = P.lp + (PLC_LAG_MAX >> 1);
    i16 *x4 = P.x4, *y4 = P.y4;
    i32 *xcorr = P.xcorr;
    i32 mx = 0, mn = 0;
    for (int j = lane(); j < (len >> 2); j += LANES) { i32 v = x_lp[2 * j]; x4[j] = (i16)v; mx = imax(mx, v); mn = imin(mn, v); }
    for (int j = lane(); j < (lag >> 2); j += LANES) { i32 v = y[2 * j]; y4[j] = (i16)v; mx = imax(mx, v); mn = imin(mn, v); }
    int shift = celt_ilog2(imax(1, imax(wave_max(mx), -wave_min(mn)))) - 11;
    wave_sync();
    if (shift > 0) {
        for (int j = lane(); j < (len >> 2); j += LANES) x4[j] = (i16)(x4[j] >> shift);
        for (int j = lane(); j < (lag >> 2); j += LANES) y4[j] = (i16)(y4[j] >> shift);
        shift *= 2;
    } else {
        shift = 0;
    }
    wave_sync();
    // celt_pitch_xcorr(x4, y4, xcorr, 332, 155): one lag per lane
    i32 mc = 1;
    for (int i = lane(); i < (max_pitch >> 2); i += LANES) {
        i32 s = 0;
        for (int j = 0; j < (len >> 2); j++) s = add32(s, __mul24(x4[j], y4[i + j]));
        xcorr[i] = s;
        mc = imax(mc, s);
    }
    i32 maxcorr = wave_max(mc);
    wave_sync();
    int best_pitch[2];
    find_best_pitch_wave(xcorr, y4, len >> 2, max_pitch >> 2, best_pitch, 0, maxcorr);
    wave_sync();
    for (int i = lane(); i < (max_pitch >> 1); i += LANES) xcorr[i] = 0;
    wave_sync();
    maxcorr = 1;
    for (int cand = 0; cand < 2; cand++) {
        const int bpc = cand ? best_pitch[1] : best_pitch[0];
        for (int i = imax(0, 2 * bpc - 2); i <= imin((max_pitch >> 1) - 1, 2 * bpc + 2); i++) {
            if (cand == 1) { int d0 = i - 2 * best_pitch[0]; if ((d0 < 0 ? -d0 : d0) <= 2) continue; }   // done already
            i32 p = 0;
            for (int j = lane(); j < (len >> 1); j += LANES) p = add32(p, mul16_16(x_lp[j], y[i + j]) >> shift);
            i32 sum = wave_add(p);
            st0(&xcorr[i], imax(-1, sum));
            maxcorr = imax(maxcorr, sum);
        }
    }
    wave_sync();
    find_best_pitch_wave(xcorr, y, len >> 1, max_pitch >> 1, best_pitch, shift + 1, maxcorr);
    int offset = 0;
    if (best_pitch[0] > 0 && best_pitch[0] < (max_pitch >> 1) - 1) {
        i32 a = xcorr[best_pitch[0] - 1], b = xcorr[best_pitch[0]], c = xcorr[best_pitch[0] + 1];
        if (sub32(c, a) > mul16_32_q15(22938, sub32(b, a))) offset = 1;
        else if (sub32(a, c) > mul16_32_q15(22938, sub32(b, c))) offset = -1;
    }
    wave_sync();
    return 2 * best_pitch[0] - offset;
}

// The LPC filter of the first loss (celt_decoder.c:541-565): _celt_autocorr(exc, ac, window, 120, 24, 1024), the -40 dB floor, lag
// windowing, _celt_lpc of order 24. raw = the 1024 samples before the loss; leaves the coefficients in P.lpc16 and in lpc_out.
template <class L>
CA_DEVFN void plc_lpc(L &P, const i16 *raw, i16 *lpc_out)
{
    const int n = MAXP;
    i16 *xx = P.exc;
    for (int i = lane(); i < n; i += LANES) {
        i32 v = raw[i];
        if (i < OVL) v = mul16_16_q15(v, CLT_window120[i]);
        else if (i >= n - OVL) v = mul16_16_q15(v, CLT_window120[n - 1 - i]);
        xx[i] = (i16)v;
    }
    wave_sync();
    i32 part = 0;
    for (int i = lane(); i < n; i += LANES) part = add32(part, mul16_16(xx[i], xx[i]) >> 9);
    const i32 ac0 = add32(1 + (n << 7), wave_add(part));
    int sh = (celt_ilog2(ac0) - 30 + 10) / 2;
    if (sh > 0) {
        for (int i = lane(); i < n; i += LANES) xx[i] = (i16)pshr32(xx[i], sh);
    } else {
        sh = 0;
    }
    wave_sync();
    // ac[k] = sum_{i + k < n} xx[i] * xx[i + k]: celt_pitch_xcorr over fastN plus the tail loop add up to exactly this
    for (int k = 0; k <= LPC_ORD; k++) {
        i32 p = 0;
        for (int i = lane(); i + k < n; i += LANES) p = add32(p, __mul24(xx[i], xx[i + k]));
        p = wave_add(p);
        st0(&P.ac[k], p);
    }
    wave_sync();
    i32 a0 = P.ac[0];
    if (sh == 0) a0 = add32(a0, 1);
    int up = 0, down = 0;
    if (a0 < 268435456) up = 29 - ec_ilog((u32)a0);
    else if (a0 >= 536870912) down = a0 >= 1073741824 ? 2 : 1;
    wave_sync();
    for (int k = lane(); k <= LPC_ORD; k += LANES) {
        i32 v = k == 0 ? a0 : P.ac[k];
        v = up ? shl32(v, up) : v >> down;
        if (k == 0) v = add32(v, v >> 13);                                          // noise floor of -40 dB
        else v = sub32(v, mul16_32_q15(2 * k * k, v));                               // lag windowing
        P.ac[k] = v;
    }
    for (int k = lane(); k < LPC_ORD; k += LANES) { P.lpc32[0][k] = 0; P.lpc32[1][k] = 0; }
    wave_sync();
    // _celt_lpc (celt_lpc.c:37-92). One step reads the old coefficients and writes the new ones into the other row.
    const i32 acz = P.ac[0];
    i32 err = acz;
    int cur = 0;
    if (acz != 0) {
        for (int i = 0; i < LPC_ORD; i++) {
            const i32 *lo = P.lpc32[cur];
            i32 *ln = P.lpc32[cur ^ 1];
            i32 p = 0;
            for (int j = lane(); j < i; j += LANES) p = add32(p, mul32_32_q31(lo[j], P.ac[i - j]));
            const i32 rr = add32(wave_add(p), P.ac[i + 1] >> 3);
            const i32 r = neg32(frac_div32(shl32(rr, 3), err));
            for (int j = lane(); j < i; j += LANES) ln[j] = add32(lo[j], mul32_32_q31(r, lo[i - 1 - j]));
            st0(&ln[i], r >> 3);
            wave_sync();
            cur ^= 1;
            err = sub32(err, mul32_32_q31(mul32_32_q31(r, r), err));
            if (err < (acz >> 10)) break;
        }
    }
    for (int k = lane(); k < LPC_ORD; k += LANES) {
        const i16 v = (i16)pshr32(P.lpc32[cur][k], 16);
        P.lpc16[k] = v;
        lpc_out[k] = v;
    }
    wave_sync();
}

// celt_lcg_rand applied n times is x -> a*x + c with (a, c) = the n-th power of the map; the powers of one map commute
CA_DEV u32 plc_lcg_jump(u32 seed, int n)
{
    u32 a = 1, c = 0, pa = 1664525u, pc = 1013904223u;
    for (int b = 0; b < 12; b++) {
        if ((n >> b) & 1) { c = pa * c + pc; a = pa * a; }
        pc = pa * pc + pc;
        pa = pa * pa;
    }
    return a * seed + c;
}

// Stage 1 of a lost frame (see the head of this file). In: st->mid_plc == OPUSGPU_PLC_LOST; out: st->mid_plc = what is still owed.
// ANYN (opusgpu_decode_batch_any after a short packet): the concealed frame is n = 120 << lm samples, celt_decode_lost(st, N, LM);
// without it N = 960 and LM = 3 are the constants they were.
template <bool ANYN = false, class L>
CA_DEVFN void celt_plc_wave(L &P, opusgpu_celt_dec_state *st, const int n = FRAME, const int lm = LM3)
{
    if (uni(st->mid_plc) != OPUSGPU_PLC_LOST) return;
    const int N = ANYN ? n : (int)FRAME, MM = ANYN ? 1 << lm : (int)M8;
    if (!uni(st->started)) {
        // no packet decoded yet: zeros, and the state stays as it is (src/opus_decoder.c:261-268)
        CA_COUNT("plc_no_history", 1);
        wave_sync();
        st0(&st->mid_plc, OPUSGPU_PLC_ZEROS);
        return;
    }
    const int loss_count = uni(st->loss_count);
    if (loss_count >= 5) {
        // noise-based PLC/CNG (celt_decoder.c:451-506): decay the energies toward the background, fill the bands with noise;
        // celt_synthesis is celt_decode_synth, fed through the hand-off
        CA_COUNT("plc_noise", 1);
        // both channels of the decoder, the bands [0, end) of the last packet's bandwidth (st->end); the synthesis zeroes the rest
        const int end = uni(celt_state_end(st));
        if (end < NB) CA_COUNT("chbw_plc_noise_narrow", 1);
        const i32 decay = loss_count == 0 ? 1536 : 512;                            // QCONST16(1.5f / .5f, DB_SHIFT)
        const u32 seed0 = uni(st->rng);
        for (int i = lane(); i < 2 * NB; i += LANES)
            if (i % NB < end) st->oldBandE[i] = (i16)imax(st->backgroundLogE[i], st->oldBandE[i] - decay);
        // one lane per (channel, band): the band's first draw is (channel * M * eBands[end] + its first bin) steps down the chain
        for (int b = lane(); b < 2 * NB; b += LANES) {
            const int c = b >= NB, i = b - c * NB;
            if (i >= end) continue;
            const int first = MM * CLT_eband5ms[i], blen = MM * (CLT_eband5ms[i + 1] - CLT_eband5ms[i]);
            x16_t *X = (x16_t *)st->mid_X + c * N + first;
            u32 seed = plc_lcg_jump(seed0, c * MM * CLT_eband5ms[end] + first);
            for (int j = 0; j < blen; j++) {
                seed = celt_lcg_rand(seed);
                X[j] = (i16)((i32)seed >> 20);
            }
            renormalise_vector_dec(X, blen, 32767);
        }
        wave_sync();
        if (lane() == 0) {
            st->rng = plc_lcg_jump(seed0, 2 * MM * CLT_eband5ms[end]);
            if (ANYN) st->mid_LM = lm;
            st->mid_valid = 1;
            st->mid_isTransient = 0;
            st->mid_silence = 0;
            st->mid_mono = 0;
            st->mid_pf_period_old = st->mid_pf_period = st->mid_pf_period_new = MINP;   // no post-filter on a concealed frame
            st->mid_pf_gain_old = st->mid_pf_gain = st->mid_pf_gain_new = 0;
            st->mid_pf_tapset_old = st->mid_pf_tapset = st->mid_pf_tapset_new = 0;
            st->mid_plc = OPUSGPU_PLC_NOISE;
            st->loss_count = loss_count + 1;
        }
        return;
    }

    // pitch-based PLC (celt_decoder.c:507-706)
    int pitch_index;
    i32 fade = 32767;
    if (loss_count == 0) {
        CA_COUNT("plc_pitch_first", 1);
        plc_pitch_downsample(P, st);
        pitch_index = PLC_LAG_MAX - plc_pitch_search(P);
    } else {
        CA_COUNT("plc_pitch_repeat", 1);
        pitch_index = uni(st->last_pitch_index);
        fade = 26214;                                                              // QCONST16(.8f, 15)
    }
    pitch_index = imin(imax(pitch_index, PLC_LAG_MIN), PLC_LAG_MAX);               // (what the search returns lies inside anyway)
    if (uni(st->postfilter_gain) != 0) CA_COUNT("plc_pitch_postfilter_gain", 1);
    const int exc_length = imin(2 * pitch_index, (int)MAXP);
    const int off = MAXP - pitch_index;                                            // extrapolation_offset
    for (int c = 0; c < 2; c++) {
        i32 *buf = st->decode_mem[c];
        for (int k = lane(); k < LPC_ORD + MAXP; k += LANES) P.xin[k] = (i16)pshr32(buf[DEC_BUF - MAXP - LPC_ORD + k], 12);
        wave_sync();
        const i16 *raw = P.xin + LPC_ORD;                                          // raw[i] = ROUND16(buf[DEC_BUF - MAXP + i]), i >= -24
        if (loss_count == 0) {
            plc_lpc(P, raw, st->lpc[c]);
        } else {
            for (int k = lane(); k < LPC_ORD; k += LANES) P.lpc16[k] = st->lpc[c][k];
            wave_sync();
        }
        // celt_fir over the last exc_length samples, its memory the samples before them (celt_lpc.c:95-149)
        for (int i = MAXP - exc_length + lane(); i < MAXP; i += LANES) {
            i32 sum = 0;
#pragma unroll
            for (int k = 0; k < LPC_ORD; k++) sum = add32(sum, __mul24(P.lpc16[k], raw[i - 1 - k]));
            const i32 v = add32(raw[i], pshr32(sum, 12));
            P.exc[i] = (i16)imin(imax(v, -32768), 32767);
        }
        wave_sync();
        // is the waveform decaying, and how fast (celt_decoder.c:586-603)
        i32 decay;
        {
            i32 mx = 0, mn = 0;
            for (int i = MAXP - exc_length + lane(); i < MAXP; i += LANES) { mx = imax(mx, P.exc[i]); mn = imin(mn, P.exc[i]); }
            const int shift = imax(0, 2 * celt_zlog2(imax(wave_max(mx), -wave_min(mn))) - 20);
            const int decay_length = exc_length >> 1;
            i32 e1 = 0, e2 = 0;
            for (int i = lane(); i < decay_length; i += LANES) {
                i32 e = P.exc[MAXP - decay_length + i];
                e1 = add32(e1, mul16_16(e, e) >> shift);
                e = P.exc[MAXP - 2 * decay_length + i];
                e2 = add32(e2, mul16_16(e, e) >> shift);
            }
            i32 E1 = add32(1, wave_add(e1));
            const i32 E2 = add32(1, wave_add(e2));
            E1 = imin(E1, E2);
            decay = (i16)celt_sqrt(frac_div32(E1 >> 1, E2));
        }
        // attenuation of period p of the extrapolation (celt_decoder.c:618-625)
        if (lane() == 0) {
            i32 a = (i16)mul16_16_q15(fade, decay);
            for (int p = 0; p < PLC_EXT / PLC_LAG_MIN + 1; p++) {
                P.att[p] = (i16)a;
                a = (i16)mul16_16_q15(a, decay);
            }
        }
        // OPUS_MOVE(buf, buf + N, DECODE_BUFFER_SIZE - N)
        if (ANYN) {
            // ascending blocks of four loads, then their stores: the source runs N >= 120 ahead, so nothing is read after it was written
            for (int k0 = 0; k0 < DEC_BUF - N; k0 += 4 * LANES) {
                i32 hv[4];
#pragma unroll
                for (int m = 0; m < 4; m++)
                    if (k0 + lane() + LANES * m < DEC_BUF - N) hv[m] = buf[N + k0 + lane() + LANES * m];
                wave_sync();
#pragma unroll
                for (int m = 0; m < 4; m++)
                    if (k0 + lane() + LANES * m < DEC_BUF - N) buf[k0 + lane() + LANES * m] = hv[m];
                wave_sync();
            }
        } else if (LANES == 64) {
            enum { NM = (DEC_BUF - FRAME) / 64 };
            static_assert((DEC_BUF - FRAME) % 64 == 0, "history move in whole wavefronts");
            i32 hv[NM];
#pragma unroll
            for (int m = 0; m < NM; m++) hv[m] = buf[FRAME + lane() + 64 * m];
            wave_sync();
#pragma unroll
            for (int m = 0; m < NM; m++) buf[lane() + 64 * m] = hv[m];
        } else {
            for (int k = 0; k < DEC_BUF - FRAME; k++) buf[k] = buf[k + FRAME];
        }
        wave_sync();
        // the excitation repeated with period pitch_index, and the energy S1 of the signal it came from (celt_decoder.c:613-635:
        // after the move that signal is what raw[] holds)
        i32 s1 = 0;
        for (int i = lane(); i < N + OVL; i += LANES) {
            const int p = i / pitch_index, j = i - p * pitch_index;
            buf[DEC_BUF - N + i] = shl32(mul16_16_q15(P.att[p], P.exc[off + j]), 12);
            const i32 t = raw[off + j];
            s1 = add32(s1, mul16_16(t, t) >> 8);
        }
        s1 = wave_add(s1);
        st0(&st->mid_plc_S1[c], s1);
        wave_sync();
    }
    if (lane() == 0) {
        if (loss_count == 0) st->last_pitch_index = pitch_index;
        st->mid_plc = OPUSGPU_PLC_PITCH;
        st->loss_count = loss_count + 1;
    }
}

// Stage 2 of the pitch-based branch for one channel (celt_decoder.c:637-704): celt_iir over the 1080 extrapolated samples, the
// explosion check, the pre-filter on the overlap and the TDAC fold. etmp lives in the stream's mid_X row, which a lost frame
// does not use otherwise.
// ANYN: over n + 120 samples (a multiple of LPC_ORD for n = 120, 240, 480 too)
template <bool ANYN = false>
CA_DEV void celt_plc_tail_channel(opusgpu_celt_dec_state *st, int c, const int n = FRAME)
{
    const int EXT = ANYN ? n + OVL : (int)PLC_EXT;
    i32 *buf = st->decode_mem[c];
    i32 *x = buf + DEC_BUF - (EXT - OVL);
    // celt_iir (celt_lpc.c:151-230, the unrolled form): the filter's memory holds the NEGATED outputs as opus_val16
    i32 den[LPC_ORD], m[LPC_ORD];
#pragma unroll
    for (int k = 0; k < LPC_ORD; k++) {
        den[k] = st->lpc[c][k];
        m[LPC_ORD - 1 - k] = (i16)neg32((i16)pshr32(x[-1 - k], 12));
    }
    i32 S2 = 0;
    for (int i0 = 0; i0 < EXT; i0 += LPC_ORD) {
        i32 in[LPC_ORD];
#pragma unroll
        for (int u = 0; u < LPC_ORD; u++) in[u] = x[i0 + u];
#pragma unroll
        for (int u = 0; u < LPC_ORD; u++) {
            i32 sum = in[u];
#pragma unroll
            for (int k = 0; k < LPC_ORD; k++) sum = add32(sum, __mul24(den[k], m[(u + LPC_ORD - 1 - k) % LPC_ORD]));
            in[u] = sum;
            const i32 y = (i16)pshr32(sum, 12);
            m[u] = (i16)neg32(y);
            S2 = add32(S2, mul16_16(y, y) >> 8);
        }
#pragma unroll
        for (int u = 0; u < LPC_ORD; u++) x[i0 + u] = in[u];
    }
    // an "explosion" in the synthesis is zeroed, more energy than the signal had is attenuated (celt_decoder.c:653-687)
    const i32 S1 = st->mid_plc_S1[c];
    if (!(S1 > (S2 >> 2))) {
        CA_COUNT("plc_explosion_zeroed", 1);
        for (int i = 0; i < EXT; i++) x[i] = 0;
    } else if (S1 < S2) {
        CA_COUNT("plc_explosion_attenuated", 1);
        const i32 ratio = (i16)celt_sqrt(frac_div32(add32(S1 >> 1, 1), add32(S2, 1)));
        for (int i = 0; i < OVL; i++) {
            const i32 tmp_g = (i16)(32767 - mul16_16_q15(CLT_window120[i], 32767 - ratio));
            x[i] = mul16_32_q15(tmp_g, x[i]);
        }
        for (int i = OVL; i < EXT; i++) x[i] = mul16_32_q15(ratio, x[i]);
    }
    // comb_filter(etmp, buf + 2048, T, T, 120, -g, -g, tapset, tapset) (celt.c:183-244: g0 == g1, so the constant filter alone).
    // It looks back T + 2 samples from buf + 2048: T in [15, 1022] and tapset in [0, 2] whatever the state holds.
    i32 *xo = buf + DEC_BUF;
    i32 *etmp = reinterpret_cast<i32 *>(st->mid_X) + c * OVL;
    const i32 g = (i16)neg32(st->postfilter_gain);
    const int T = imin(imax(st->postfilter_period, MINP), MAXP - 2);
    const int tapset = imin(imax(st->postfilter_tapset, 0), 2);
    if (g == 0) {
        for (int i = 0; i < OVL; i++) etmp[i] = xo[i];
    } else {
        const i32 g10 = (i16)mul16_16_p15(g, CLT_comb_gains[tapset * 3 + 0]), g11 = (i16)mul16_16_p15(g, CLT_comb_gains[tapset * 3 + 1]),
                  g12 = (i16)mul16_16_p15(g, CLT_comb_gains[tapset * 3 + 2]);
        i32 x4 = xo[-T - 2], x3 = xo[-T - 1], x2 = xo[-T], x1 = xo[-T + 1];
        for (int i = 0; i < OVL; i++) {
            const i32 x0 = xo[i - T + 2];
            etmp[i] = add32(add32(add32(xo[i], mul16_32_q15(g10, x2)), mul16_32_q15(g11, add32(x1, x3))), mul16_32_q15(g12, add32(x0, x4)));
            x4 = x3; x3 = x2; x2 = x1; x1 = x0;
        }
    }
    wave_sync();
    // simulate TDAC on the concealed audio so that it blends with the MDCT of the next frame
    for (int i = 0; i < OVL / 2; i++)
        xo[i] = add32(mul16_32_q15(CLT_window120[i], etmp[OVL - 1 - i]), mul16_32_q15(CLT_window120[OVL - i - 1], etmp[i]));
}

// deemphasis (celt_decoder.c:183-285) of one channel, as at the end of celt_decode_post_channel
CA_DEV void celt_deemphasis_channel(opusgpu_celt_dec_state *st, int c, i16 *pcm, const int N = FRAME)
{
    const i32 *out_syn = st->decode_mem[c] + DEC_BUF - N;
    i32 m = st->preemph_memD[c];
    for (int j = 0; j < N; j++) {
        i32 t = add32(out_syn[j], m);
        m = mul16_32_q15(27853, t);
        i32 v = pshr32(t, 12);
        v = imax(v, -32768);
        v = imin(v, 32767);
        pcm[j * 2 + c] = (i16)v;
    }
    st->preemph_memD[c] = m;
}

// which packets opusgpu_decode_batch_plc conceals: a lost one (no length) and DTX, a packet whose payload behind the TOC byte is
// empty or a single byte (src/opus_decoder.c:245-251: "Payloads of 1 (2 including ToC) or 0 trigger the PLC/DTX"); only the
// TOCs this decoder implements. The stream takes such a TOC's bandwidth and channel
// count before it is concealed (celt_plc_dtx_toc).
CA_DEV bool celt_plc_conceals(const u8 *data, int len);
CA_DEV bool celt_plc_is_dtx(int toc, int len) { return (len == 1 || len == 2) && celt_toc_accepted(toc); }

CA_DEV void celt_plc_dtx_toc(opusgpu_celt_dec_state *st, int toc)
{
    if (celt_toc_end(toc) != celt_state_end(st)) CA_COUNT("chbw_dtx_end_change", 1);
    celt_state_note_toc(st, toc);
}

#if defined(CA_HOST_EMU)
// The emulation asks celt_plc_conceals(data, len) and then calls celt_decode_lost_frame(P, L, st, pcm), which does not see the
// packet: the TOC of a DTX packet travels between the two calls here (the emulation is one thread).
static int g_emu_dtx_toc = -1;
#endif

CA_DEV bool celt_plc_conceals(const u8 *data, int len)
{
    const bool dtx = (len == 1 || len == 2) && celt_plc_is_dtx(data[0], len);
    if (dtx && len == 2) CA_COUNT("corrupt_payload_one_byte", 1);
#if defined(CA_HOST_EMU)
    g_emu_dtx_toc = dtx ? data[0] : -1;
#endif
    return len == 0 || dtx;
}

// a lost frame through all stages, for the host emulation
template <class LP_, class S>
CA_DEV DecResult celt_decode_lost_frame(LP_ &P, S &L, opusgpu_celt_dec_state *st, i16 *pcm)
{
#if defined(CA_HOST_EMU)
    if (g_emu_dtx_toc >= 0) celt_plc_dtx_toc(st, g_emu_dtx_toc);
    g_emu_dtx_toc = -1;
#endif
    st->mid_valid = 0;
    st->mid_plc = OPUSGPU_PLC_LOST;
    celt_plc_wave(P, st);
    celt_decode_synth(L, st);
    for (int c = 0; c < 2; c++) {
        if (st->mid_plc == OPUSGPU_PLC_ZEROS) {
            for (int j = 0; j < FRAME; j++) pcm[j * 2 + c] = 0;
        } else if (st->mid_plc == OPUSGPU_PLC_PITCH) {
            celt_plc_tail_channel(st, c);
            celt_deemphasis_channel(st, c, pcm);
        } else {
            celt_decode_post_channel(st, c, pcm);
        }
    }
    DecResult r;
    r.samples = FRAME;
    r.final_range = st->final_range = 0;                                           // src/opus_decoder.c:579-580
    return r;
}

// opusgpu_decode_batch_any: a lost packet is concealed as above when the stream's last packet was a 20 ms one (or none came yet).
// After a packet of N < 960 samples the reference conceals the 960 samples in steps of N (src/opus_decoder.c:250 clamps the concealed
// duration to the last packet's, :613-622 loops): 960 / N calls of celt_decode_lost(st, N, LM), each followed by its de-emphasis.
// The steps depend on each other, so ONE wavefront (one "lane" in the emulation) does them all: celt_plc_wave, the synthesis
// where the step is noise-based, and -- on lanes 0 and 1, one per channel -- the tail of the pitch-based branch and the
// de-emphasis into the step's N sample pairs of the stream's row. st->last_short is LM + 1 of that last packet.
// GIVEN (opusgpu_decode_batch_packets, a DTX frame under a short-frame TOC): the caller names the step's size, lm_given, and how many
// steps, steps_given -- one, the TOC's own duration (src/opus_decoder.c:250 with st->frame_size already the packet's, :685).
template <bool GIVEN = false, class LP_, class S>
CA_DEVFN void celt_plc_short_steps(LP_ &P, S &L, opusgpu_celt_dec_state *st, i16 *pcm, const int lm_given = 0, const int steps_given = 0)
{
    const int lm = GIVEN ? lm_given & 3 : (uni(st->last_short) - 1) & 3, N = (FRAME / M8) << lm;
    const int steps = GIVEN ? steps_given : FRAME / N;
    CA_COUNT(GIVEN ? "multi_dtx_short" : "fs_loss_after_short", 1);
    for (int k = 0; k < steps; k++) {
        const int loss_count = uni(st->loss_count);
        const int noise = loss_count >= 5;
        CA_COUNT(noise ? "fs_short_step_noise" : "fs_short_step_pitch", 1);
        if (lane() == 0) st->mid_plc = OPUSGPU_PLC_LOST;
        wave_sync();
        celt_plc_wave<true>(P, st, N, lm);
        wave_sync();
        if (noise) celt_decode_synth_any(L, st);
        wave_sync();
        for (int c = lane(); c < 2; c += LANES) {
            if (!noise) celt_plc_tail_channel<true>(st, c, N);
            celt_deemphasis_channel(st, c, pcm + (size_t)k * N * 2, N);
        }
        wave_sync();
    }
    if (lane() == 0) {
        st->mid_valid = 0;
        st->mid_plc = OPUSGPU_PLC_DONE;
        st->final_range = 0;
    }
}

// a lost frame through the stages of opusgpu_decode_batch_any, for the host emulation (celt_plc_conceals was asked before)
template <class LP_, class S>
CA_DEV DecResult celt_decode_lost_frame_any(LP_ &P, S &L, opusgpu_celt_dec_state *st, i16 *pcm)
{
#if defined(CA_HOST_EMU)
    const int dtx_toc = g_emu_dtx_toc;
    g_emu_dtx_toc = -1;
    if (dtx_toc < 0 && st->last_short != 0) {
        celt_plc_short_steps(P, L, st, pcm);
        DecResult r;
        r.samples = FRAME;
        r.final_range = 0;
        return r;
    }
    if (dtx_toc >= 0) celt_plc_dtx_toc(st, dtx_toc);
#endif
    st->last_short = 0;                                                           // (a DTX packet's TOC says 20 ms)
    st->mid_LM = LM3;
    st->mid_valid = 0;
    st->mid_plc = OPUSGPU_PLC_LOST;
    celt_plc_wave(P, st);
    celt_decode_synth_any(L, st);
    for (int c = 0; c < 2; c++) {
        if (st->mid_plc == OPUSGPU_PLC_ZEROS) {
            for (int j = 0; j < FRAME; j++) pcm[j * 2 + c] = 0;
        } else if (st->mid_plc == OPUSGPU_PLC_PITCH) {
            celt_plc_tail_channel(st, c);
            celt_deemphasis_channel(st, c, pcm);
        } else {
            celt_decode_post_channel_any(st, c, pcm);
        }
    }
    DecResult r;
    r.samples = FRAME;
    r.final_range = st->final_range = 0;
    return r;
}

}  // namespace ca
