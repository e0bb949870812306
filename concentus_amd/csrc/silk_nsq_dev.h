// silk_nsq_dev.h -- the arithmetic of the two SILK noise-shaping quantisers as device functions: what silk_NSQ and
// silk_NSQ_del_dec share (quantisation-level decision, fused re-whitening filter, per-subframe scalars, the vector types of the
// 4-byte-aligned records) and the whole plain quantiser for one record, one lane per call. Used by silk_nsq_kernel
// (silk_kernels.hip), by silk_nsq_del_dec_kernel (silk_nsq_del_dec.hip: the shared pieces) and by the host build of tests/emu.
//
//   silk_NSQ_c                  opus-fix/silk/NSQ.c:74-180
//   silk_noise_shape_quantizer  opus-fix/silk/NSQ.c:183-421            (level decision :303-351; the same at NSQ_del_dec.c:436-484)
//   silk_nsq_scale_states       opus-fix/silk/NSQ.c:423-496            (NSQ_del_dec.c:632-724)
//   silk_LPC_analysis_filter    opus-fix/silk/LPC_analysis_filter.c:47-108 (FIXED_POINT branch)
//
// Arithmetic: the reference's x86-64 build uses the 64-bit macro forms (OPUS_FAST_INT64, silk/macros.h:47-102);
// 16x32 products are evaluated on split halves (full-rate 24-bit multiplier), 32x32 ones as 64-bit.
#pragma once
#include "silk_math.h"
#include "../../include/opusgpu_silk.h"

namespace ca {

// per-record scratch in HBM: the scaled re-whitened prediction buffer int32 sLTP_Q15[640] (the int16 sLTP[640] behind it is
// unused since the re-whitening writes its outputs scaled; it stays in the workspace's size).
struct NsqScratch { i32 sLTP_Q15[640]; i16 sLTP[640]; };

// Four (two) values per access. The records are only 4-byte aligned (opusgpu_nsq_state is 4 380 bytes), hence vector types of
// that alignment; a lane's access to its own record costs a cache line whatever its width. H4: four samples of xq at any index.
struct __attribute__((packed, aligned(4), may_alias)) Q4 { i32 v[4]; };
struct __attribute__((packed, aligned(4), may_alias)) Q2 { i32 v[2]; };
struct __attribute__((packed, aligned(2), may_alias)) H4 { i16 v[4]; };

// A step of the single-sample mode reads what the step before it stored: the compiler must not carry the taps over the stores.
// Within a lane memory operations are performed in program order, so the fence costs no s_waitcnt (cf. wave_sync(), wave.h).
#if defined(CA_HOST_EMU)
CA_DEV void nsq_store_fence() { asm volatile("" ::: "memory"); }
#else
CA_DEV void nsq_store_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
#endif

CA_DEV int nsq_offset_Q10(const int signalType, const int quantOffsetType)               // silk/tables_other.c:95-97
{
    return signalType == 2 ? (quantOffsetType ? 100 : 32) : (quantOffsetType ? 240 : 100);
}

CA_DEV i32 nsq_harm_packed_Q14(const i32 HarmShapeGain_Q14)                               // NSQ.c:133-134: both FIR taps in one word
{
    return (HarmShapeGain_Q14 >> 2) | shl32(HarmShapeGain_Q14 >> 1, 16);
}

// the set-up of silk_nsq_scale_states (NSQ.c:433-441, :458-460) for one subframe
struct NsqGains { i32 inv_gain_Q31, gain_adj_Q16, inv_gain_Q23; };
CA_DEV NsqGains nsq_subfr_gains(const i32 gain_Q16, const i32 prev_gain_Q16)
{
    NsqGains g;
    g.inv_gain_Q31 = s_inverse32_varq(gain_Q16 > 1 ? gain_Q16 : 1, 47);
    g.gain_adj_Q16 = gain_Q16 != prev_gain_Q16 ? s_div32_varq(prev_gain_Q16, gain_Q16, 16) : (i32)1 << 16;
    g.inv_gain_Q23 = s_rshift_round(g.inv_gain_Q31, 8);
    return g;
}

// The quantisation-level decision (NSQ.c:303-351): the two candidate levels around r_Q10 and their rate-distortion values.
// silk_NSQ keeps the cheaper one; silk_NSQ_del_dec scales both values down by 10 bits and carries both candidates on.
struct NsqLevels { i32 q1_Q10, q2_Q10, rd1_Q20, rd2_Q20; };
CA_DEV NsqLevels nsq_levels(const i32 r_Q10, const int offset_Q10, const int Lambda_Q10)
{
    NsqLevels l;
    l.q1_Q10 = r_Q10 - offset_Q10;
    const i32 q1_Q0 = l.q1_Q10 >> 10;
    if (q1_Q0 > 0) {
        l.q1_Q10 = shl32(q1_Q0, 10) - 80 + offset_Q10;
        l.q2_Q10 = l.q1_Q10 + 1024;
        l.rd1_Q20 = s_smulbb(l.q1_Q10, Lambda_Q10);
        l.rd2_Q20 = s_smulbb(l.q2_Q10, Lambda_Q10);
    } else if (q1_Q0 == 0) {
        l.q1_Q10 = offset_Q10;
        l.q2_Q10 = l.q1_Q10 + (1024 - 80);
        l.rd1_Q20 = s_smulbb(l.q1_Q10, Lambda_Q10);
        l.rd2_Q20 = s_smulbb(l.q2_Q10, Lambda_Q10);
    } else if (q1_Q0 == -1) {
        l.q2_Q10 = offset_Q10;
        l.q1_Q10 = l.q2_Q10 - (1024 - 80);
        l.rd1_Q20 = s_smulbb(-l.q1_Q10, Lambda_Q10);
        l.rd2_Q20 = s_smulbb(l.q2_Q10, Lambda_Q10);
    } else {
        l.q1_Q10 = shl32(q1_Q0, 10) + 80 + offset_Q10;
        l.q2_Q10 = l.q1_Q10 + 1024;
        l.rd1_Q20 = s_smulbb(-l.q1_Q10, Lambda_Q10);
        l.rd2_Q20 = s_smulbb(-l.q2_Q10, Lambda_Q10);
    }
    i32 rr_Q10 = r_Q10 - l.q1_Q10;
    l.rd1_Q20 = s_addw(l.rd1_Q20, s_smulbb(rr_Q10, rr_Q10));
    rr_Q10 = r_Q10 - l.q2_Q10;
    l.rd2_Q20 = s_addw(l.rd2_Q20, s_smulbb(rr_Q10, rr_Q10));
    return l;
}

// gain of the re-whitened samples (NSQ.c:437, :445-456): the subframe's inverse gain, with the LTP scaling in the first subframe
CA_DEV i32 nsq_rewhite_gain_Q31(const i32 gain_Q16, const bool first_subfr, const int LTP_scale_Q14)
{
    i32 ig_Q31 = s_inverse32_varq(gain_Q16 > 1 ? gain_Q16 : 1, 47);
    if (first_subfr) ig_Q31 = shl32(s_smulwb(ig_Q31, LTP_scale_Q14), 2);
    return ig_Q31;
}

// one output of the filter below: nA = the negated coefficients, w = the previous input samples (w[0] newest), moved on by xi
CA_DEV i32 nsq_rewhiten_step(const i32 (&nA)[16], i32 (&w)[16], const i32 ig_Q31, const i32 xi)
{
    i32 sum = 0;
#pragma unroll
    for (int m = 0; m < 16; m++) sum = s_addw(sum, __mul24(nA[m], w[m]));
    i32 v = xi + pshr32(sum, 12);
    v = v > 32767 ? 32767 : (v < -32768 ? -32768 : v);
#pragma unroll
    for (int m = 15; m > 0; m--) w[m] = w[m - 1];
    w[0] = xi;
    return s_smulwb(ig_Q31, v);
}
// silk_LPC_analysis_filter (celt_fir form): out = SAT16(in + PSHR32(-sum A[m] in[ix-1-m], 12)) for ix in [i0, i1), fused with
// the scaling silk_nsq_scale_states applies to exactly these outputs (NSQ.c:445-456: sLTP_Q15[i] = SMULWB(inv_gain_Q31,
// sLTP[i])): the 16-bit sLTP buffer in between is never written or read. The `order` previous input samples travel in a
// register window, so every sample of the input is read once; four inputs per load, four results per 16-byte store.
CA_DEV void nsq_rewhiten_scaled(const i16 *inp, i32 *outq, const i16 *A_Q12, const int order, const i32 ig_Q31, const int i0, const int i1)
{
    i32 nA[16], w[16];
#pragma unroll
    for (int m = 0; m < 16; m++) {
        nA[m] = m < order ? (i32)(i16)(-A_Q12[m]) : 0;
        w[m] = (m < order && i0 < i1) ? (i32)inp[i0 - 1 - m] : 0;
    }
    int ix = i0;
    for (; ix + 4 <= i1; ix += 4) {
        const H4 xi4 = *reinterpret_cast<const H4 *>(&inp[ix]);
        Q4 o;
#pragma unroll
        for (int u = 0; u < 4; u++) o.v[u] = nsq_rewhiten_step(nA, w, ig_Q31, (i32)xi4.v[u]);
        *reinterpret_cast<Q4 *>(&outq[ix]) = o;
    }
#pragma clang loop vectorize(disable) interleave(disable)   // at most three trips: a two-wide copy of the body only adds code
    for (; ix < i1; ix++) outq[ix] = nsq_rewhiten_step(nA, w, ig_Q31, (i32)inp[ix]);
}

// ---- silk_NSQ: the whole quantiser for one record, one lane per call ------------------------------------------------------

// a[i .. end) *= gain_adj_Q16. Four values per access, and the loads of eight accesses in flight before the first store: written
// as load - scale - store per element the loop is one exposed memory round trip per trip.
CA_DEV void nsq_scale_run(i32 *a, int i, const int end, const i32 gain_adj_Q16)
{
    for (; i + 32 <= end; i += 32) {
        Q4 q[8];
#pragma unroll
        for (int c = 0; c < 8; c++) q[c] = *reinterpret_cast<const Q4 *>(&a[i + 4 * c]);
#pragma unroll
        for (int c = 0; c < 8; c++) {
#pragma unroll
            for (int u = 0; u < 4; u++) q[c].v[u] = s_smulww(gain_adj_Q16, q[c].v[u]);
            *reinterpret_cast<Q4 *>(&a[i + 4 * c]) = q[c];
        }
    }
    for (; i + 4 <= end; i += 4) {
        Q4 q = *reinterpret_cast<const Q4 *>(&a[i]);
#pragma unroll
        for (int u = 0; u < 4; u++) q.v[u] = s_smulww(gain_adj_Q16, q.v[u]);
        *reinterpret_cast<Q4 *>(&a[i]) = q;
    }
    for (; i < end; i++) a[i] = s_smulww(gain_adj_Q16, a[i]);
}

// d[0 .. n) = sc[0 .. n), ascending, dst below src: eight 16-byte pieces are loaded before the first of them is stored (one round
// trip per eight instead of per piece); a piece is stored below everything a later batch loads
CA_DEV void nsq_move_run(Q4 *d, const Q4 *sc, const int n)
{
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        Q4 v[8];
#pragma unroll
        for (int c = 0; c < 8; c++) v[c] = sc[i + c];
#pragma unroll
        for (int c = 0; c < 8; c++) d[i + c] = v[c];
    }
    for (; i < n; i++) { const Q4 v = sc[i]; d[i] = v; }
}

struct NsqSubfr {                      // what is constant over a subframe
    bool voiced;
    int lag, offset_Q10, Lambda_Q10, Tilt_Q14;
    i32 b[5], harm_Q14, LF_shp_Q14, inv_gain_Q23, Gain_Q10;
};
// What a sample hands to the next one. The pitch-lag taps slide by one sample per step: they are kept in registers
// (pt[j] = sLTP_Q15[pred_lag - j], st[j] = sLTP_shp_Q14[shp_lag - j]) and only the newest one is loaded.
struct NsqCarry { i32 rand_seed, sLF_AR_shp_Q14, shp_prev, pt[5], st[3]; };
struct NsqSample { i32 xq_Q14, shp_Q14, ltp_Q15; u32 pulse, xq; };      // sLPC_Q14 / sLTP_shp_Q14 / sLTP_Q15 entries, pulse and xq as bytes / half-words

// One sample of silk_noise_shape_quantizer (NSQ.c:247-400) from the short-term prediction and the raw noise-shaping feedback sum on,
// which the callers form from their own view of the two 16-deep histories. pn / sn: the taps that enter pt[0] / st[0].
CA_DEV NsqSample nsq_sample(const NsqSubfr &c, NsqCarry &s, const i32 x_Q3, const i32 LPC_pred_Q10, i32 n_AR_Q12, const i32 pn, const i32 sn)
{
    NsqSample o;
    s.rand_seed = (i32)(907633515u + (u32)s.rand_seed * 196314165u);                    // silk_RAND
    i32 LTP_pred_Q13 = 0;
    if (c.voiced) {
        LTP_pred_Q13 = 2;
#pragma unroll
        for (int j = 0; j < 5; j++) LTP_pred_Q13 = s_smlawb(LTP_pred_Q13, s.pt[j], c.b[j]);
    }
    n_AR_Q12 = shl32(n_AR_Q12, 1);
    n_AR_Q12 = s_smlawb(n_AR_Q12, s.sLF_AR_shp_Q14, c.Tilt_Q14);
    i32 n_LF_Q12 = s_smulwb(s.shp_prev, c.LF_shp_Q14);
    n_LF_Q12 = s_smlawt(n_LF_Q12, s.sLF_AR_shp_Q14, c.LF_shp_Q14);
    i32 tmp1 = s_subw(shl32(LPC_pred_Q10, 2), n_AR_Q12);
    tmp1 = s_subw(tmp1, n_LF_Q12);
    if (c.lag > 0) {
        i32 n_LTP_Q13 = s_smulwb(s_addw(s.st[0], s.st[2]), c.harm_Q14);
        n_LTP_Q13 = s_smlawt(n_LTP_Q13, s.st[1], c.harm_Q14);
        n_LTP_Q13 = shl32(n_LTP_Q13, 1);
        const i32 tmp2 = s_subw(LTP_pred_Q13, n_LTP_Q13);
        tmp1 = s_addw(tmp2, shl32(tmp1, 1));
        tmp1 = s_rshift_round(tmp1, 3);
    } else {
        tmp1 = s_rshift_round(tmp1, 2);
    }
    i32 r_Q10 = s_subw(s_smulww(x_Q3, c.inv_gain_Q23), tmp1);
    if (s.rand_seed < 0) r_Q10 = (i32)(0u - (u32)r_Q10);                                 // the dither
    r_Q10 = s_limit(r_Q10, -(31 << 10), 30 << 10);
    const NsqLevels l = nsq_levels(r_Q10, c.offset_Q10, c.Lambda_Q10);
    const i32 q1_Q10 = l.rd2_Q20 < l.rd1_Q20 ? l.q2_Q10 : l.q1_Q10;
    const i32 pulse = (i8)s_rshift_round(q1_Q10, 10);
    o.pulse = (u32)pulse & 0xffu;
    i32 exc_Q14 = shl32(q1_Q10, 4);
    if (s.rand_seed < 0) exc_Q14 = (i32)(0u - (u32)exc_Q14);
    const i32 LPC_exc_Q14 = s_addw(exc_Q14, shl32(LTP_pred_Q13, 1));
    const i32 xq_Q14 = s_addw(LPC_exc_Q14, shl32(LPC_pred_Q10, 4));
    {   // silk_SAT16(silk_RSHIFT_ROUND(silk_SMULWW(xq_Q14, Gain_Q10), 8)) in 64 bits
        i64 t = ((i64)xq_Q14 * c.Gain_Q10) >> 16;
        t = ((t >> 7) + 1) >> 1;
        o.xq = (u32)(i32)(t > 32767 ? 32767 : (t < -32768 ? -32768 : t)) & 0xffffu;
    }
    o.xq_Q14 = xq_Q14;
    s.sLF_AR_shp_Q14 = s_subw(xq_Q14, shl32(n_AR_Q12, 2));
    s.shp_prev = s_subw(s.sLF_AR_shp_Q14, shl32(n_LF_Q12, 2));
    o.shp_Q14 = s.shp_prev;
    o.ltp_Q15 = shl32(LPC_exc_Q14, 1);
    s.rand_seed = (i32)((u32)s.rand_seed + (u32)pulse);
    s.pt[4] = s.pt[3]; s.pt[3] = s.pt[2]; s.pt[2] = s.pt[1]; s.pt[1] = s.pt[0]; s.pt[0] = pn;
    s.st[2] = s.st[1]; s.st[1] = s.st[0]; s.st[0] = sn;
    return o;
}

// the five per-sample outputs of a group of four samples, one store each (a store instruction costs the wavefront one cache line
// per lane whatever its width)
CA_DEV void nsq_store_group(const NsqSample (&o)[4], i8 *pulses, i16 *xq, i32 *sLPC_Q14, i32 *sLTP_shp_Q14, i32 *sLTP_Q15)
{
    *reinterpret_cast<u32 *>(pulses) = o[0].pulse | (o[1].pulse << 8) | (o[2].pulse << 16) | (o[3].pulse << 24);
    Q2 xv;
    xv.v[0] = (i32)(o[0].xq | (o[1].xq << 16)); xv.v[1] = (i32)(o[2].xq | (o[3].xq << 16));
    *reinterpret_cast<Q2 *>(xq) = xv;
    Q4 v;
#pragma unroll
    for (int u = 0; u < 4; u++) v.v[u] = o[u].xq_Q14;
    *reinterpret_cast<Q4 *>(sLPC_Q14) = v;
#pragma unroll
    for (int u = 0; u < 4; u++) v.v[u] = o[u].shp_Q14;
    *reinterpret_cast<Q4 *>(sLTP_shp_Q14) = v;
#pragma unroll
    for (int u = 0; u < 4; u++) v.v[u] = o[u].ltp_Q15;
    *reinterpret_cast<Q4 *>(sLTP_Q15) = v;
}

// in: a record that passed nsq_record_ok (silk_validate.h). NSQ is updated in place; pulses[frame_length] out;
// sLTP_Q15: the record's NsqScratch.
CA_DEV void silk_nsq_record_dev(const opusgpu_nsq_in &in, opusgpu_nsq_state &NSQ, i8 *pulses, i32 *sLTP_Q15)
{
    const int nb_subfr = in.nb_subfr, subfr_length = in.subfr_length, frame_length = in.frame_length;
    const int ltp_mem_length = in.ltp_mem_length, predictLPCOrder = in.predictLPCOrder, shapingLPCOrder = in.shapingLPCOrder;
    NsqSubfr c;
    NsqCarry s;
    c.voiced = in.signalType == 2;
    c.lag = NSQ.lagPrev;
    c.offset_Q10 = nsq_offset_Q10(in.signalType, in.quantOffsetType);
    c.Lambda_Q10 = in.Lambda_Q10;
    s.rand_seed = in.Seed;
    s.sLF_AR_shp_Q14 = NSQ.sLF_AR_shp_Q14;
    const int LSF_interpolation_flag = in.NLSFInterpCoef_Q2 == 4 ? 0 : 1;
    int sLTP_shp_buf_idx = ltp_mem_length, sLTP_buf_idx = ltp_mem_length;
    i32 prev_gain_Q16 = NSQ.prev_gain_Q16;
    int rewhite_flag = 0;
    // short filter states in registers: sAR2_Q14[16] and the last 16 sLPC_Q14 samples (lp[0] = newest)
    i32 ar[16], lp[16];
#pragma unroll
    for (int j = 0; j < 16; j++) { ar[j] = NSQ.sAR2_Q14[j]; lp[j] = NSQ.sLPC_Q14[31 - j]; }
    i32 lpc_old[16];                  // sLPC_Q14[0..16): the older half of the 32-sample history (state output only)
#pragma unroll
    for (int j = 0; j < 16; j++) lpc_old[j] = NSQ.sLPC_Q14[j];

    for (int k = 0; k < nb_subfr; k++) {
        const i16 *A_Q12 = &in.PredCoef_Q12[((k >> 1) | (1 - LSF_interpolation_flag)) * 16];
        const i16 *B_Q14 = &in.LTPCoef_Q14[k * 5];
        const i16 *AR_shp_Q13 = &in.AR2_Q13[k * 16];
        c.harm_Q14 = nsq_harm_packed_Q14(in.HarmShapeGain_Q14[k]);
        rewhite_flag = 0;
        if (c.voiced) {
            c.lag = in.pitchL[k];
            if ((k & (3 - (LSF_interpolation_flag << 1))) == 0) {
                // re-whitening of the lag + 2 samples the long-term predictor reaches back to
                const int start_idx = ltp_mem_length - c.lag - predictLPCOrder - 5 / 2;
                nsq_rewhiten_scaled(&NSQ.xq[start_idx + k * subfr_length], &sLTP_Q15[start_idx], A_Q12, predictLPCOrder,
                                    nsq_rewhite_gain_Q31(in.Gains_Q16[k], k == 0, in.LTP_scale_Q14), predictLPCOrder, ltp_mem_length - start_idx);
                rewhite_flag = 1;
                sLTP_buf_idx = ltp_mem_length;
            }
        }
        // ---- silk_nsq_scale_states (NSQ.c:423-496) ----
        const i32 gain = in.Gains_Q16[k];
        const NsqGains g = nsq_subfr_gains(gain, prev_gain_Q16);
        prev_gain_Q16 = gain;
        // (rewhite_flag: sLTP_Q15[idx - lag - 2 .. idx) was scaled where it was produced, above)
        if (g.gain_adj_Q16 != (i32)1 << 16) {
            nsq_scale_run(NSQ.sLTP_shp_Q14, sLTP_shp_buf_idx - ltp_mem_length, sLTP_shp_buf_idx, g.gain_adj_Q16);
            if (c.voiced && rewhite_flag == 0) nsq_scale_run(sLTP_Q15, sLTP_buf_idx - in.pitchL[k] - 5 / 2, sLTP_buf_idx, g.gain_adj_Q16);
            s.sLF_AR_shp_Q14 = s_smulww(g.gain_adj_Q16, s.sLF_AR_shp_Q14);
#pragma unroll
            for (int j = 0; j < 16; j++) {
                lp[j] = s_smulww(g.gain_adj_Q16, lp[j]);
                lpc_old[j] = s_smulww(g.gain_adj_Q16, lpc_old[j]);
                ar[j] = s_smulww(g.gain_adj_Q16, ar[j]);
            }
        }
        // ---- silk_noise_shape_quantizer (NSQ.c:183-421) ----
        c.inv_gain_Q23 = g.inv_gain_Q23;
        c.Gain_Q10 = gain >> 6;
        c.Tilt_Q14 = in.Tilt_Q14[k];
        c.LF_shp_Q14 = in.LF_shp_Q14[k];
        const int lag = c.lag;
        int shp_lag = sLTP_shp_buf_idx - lag + 3 / 2;          // index of shp_lag_ptr[0]
        int pred_lag = sLTP_buf_idx - lag + 5 / 2;             // index of pred_lag_ptr[0]
        s.shp_prev = NSQ.sLTP_shp_Q14[sLTP_shp_buf_idx - 1];   // sLTP_shp_Q14[idx-1], carried in a register
        i32 a12[16], ar13[16];
#pragma unroll
        for (int j = 0; j < 16; j++) { a12[j] = A_Q12[j]; ar13[j] = AR_shp_Q13[j]; }
#pragma unroll
        for (int j = 0; j < 5; j++) c.b[j] = B_Q14[j];
        const i32 *x_Q3 = in.x_Q3 + k * subfr_length;
        i8 *pl = pulses + k * subfr_length;
        i16 *pxq = &NSQ.xq[ltp_mem_length + k * subfr_length];
        // A step writes position idx and the newest taps of the NEXT step sit at idx + 3 - lag / idx + 2 - lag, i.e. were written
        // at least a step ago when lag >= 4 (pitch lags are >= 2 ms): they are fetched a whole step ahead, like the next input sample.
        auto load_taps = [&]() __attribute__((always_inline)) {
            if (c.voiced) {
#pragma unroll
                for (int j = 0; j < 5; j++) s.pt[j] = sLTP_Q15[pred_lag - j];
            }
            if (lag > 0) {
#pragma unroll
                for (int j = 0; j < 3; j++) s.st[j] = NSQ.sLTP_shp_Q14[shp_lag - j];
            }
        };
#pragma unroll
        for (int j = 0; j < 5; j++) s.pt[j] = 0;
        s.st[0] = s.st[1] = s.st[2] = 0;
        load_taps();
        // ---- the usual case (no pitch lag, or one of >= 12 samples; subframes of 4n samples), four samples per group ----
        // What limits the kernel is the memory pipeline, not arithmetic: a lane's load or store of its own record occupies it for a
        // cache line whatever its width, and loads queue behind earlier stores (one counter orders both). So a group's three inputs
        // (x_Q3, the prediction tap, the shaping tap: four values each) are ONE 16-byte load each, issued BEFORE the previous group's
        // five 16-byte stores, whose completion then overlaps the next group's arithmetic. Inside a group the two 16-deep
        // histories (sLPC_Q14's newest samples, the sAR2 delay line) are not shifted per sample: sample u reads them through
        // compile-time indices into [the group's new values | the registers as they were at the group's start].
        if ((lag <= 0 || lag >= 12) && (subfr_length & 3) == 0) {
            i32 ar13z[16];
#pragma unroll
            for (int j = 0; j < 16; j++) ar13z[j] = j < shapingLPCOrder ? ar13[j] : 0;       // the delay line beyond the order adds nothing
            Q4 xg, pg, sg;
#pragma unroll
            for (int u = 0; u < 4; u++) { pg.v[u] = 0; sg.v[u] = 0; }
            xg = *reinterpret_cast<const Q4 *>(&x_Q3[0]);
            if (c.voiced) pg = *reinterpret_cast<const Q4 *>(&sLTP_Q15[pred_lag + 1]);
            if (lag > 0) sg = *reinterpret_cast<const Q4 *>(&NSQ.sLTP_shp_Q14[shp_lag + 1]);
            for (int i0 = 0; i0 < subfr_length; i0 += 4) {
                NsqSample o[4];
                i32 sv[4] = {0, 0, 0, 0};
                const int shp_idx0 = sLTP_shp_buf_idx, ltp_idx0 = sLTP_buf_idx;
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    sv[u] = u == 0 ? lp[0] : o[u - 1].xq_Q14;                              // the newest sLPC_Q14 sample enters the delay line
                    i32 LPC_pred_Q10 = predictLPCOrder >> 1;
#pragma unroll
                    for (int j = 0; j < 10; j++) LPC_pred_Q10 = s_smlawb(LPC_pred_Q10, j < u ? o[u - 1 - j].xq_Q14 : lp[j - u], a12[j]);
                    if (predictLPCOrder == 16) {
#pragma unroll
                        for (int j = 10; j < 16; j++) LPC_pred_Q10 = s_smlawb(LPC_pred_Q10, j < u ? o[u - 1 - j].xq_Q14 : lp[j - u], a12[j]);
                    }
                    // noise shape feedback (NSQ.c:262-279): after the shift the delay line holds [sv[u], sv[u-1], .., ar[0], ar[1], ..]
                    i32 n_AR_Q12 = shapingLPCOrder >> 1;
#pragma unroll
                    for (int j = 0; j < 16; j++) n_AR_Q12 = s_smlawb(n_AR_Q12, j <= u ? sv[u - j] : ar[j - u - 1], ar13z[j]);
                    o[u] = nsq_sample(c, s, xg.v[u], LPC_pred_Q10, n_AR_Q12, pg.v[u], sg.v[u]);
                }
                sLTP_shp_buf_idx += 4;
                sLTP_buf_idx += 4;
                pred_lag += 4;
                shp_lag += 4;
                if (i0 + 4 < subfr_length) {                                                // the next group's inputs, ahead of this group's stores
                    xg = *reinterpret_cast<const Q4 *>(&x_Q3[i0 + 4]);
                    if (c.voiced) pg = *reinterpret_cast<const Q4 *>(&sLTP_Q15[pred_lag + 1]);
                    if (lag > 0) sg = *reinterpret_cast<const Q4 *>(&NSQ.sLTP_shp_Q14[shp_lag + 1]);
                }
                nsq_store_group(o, &pl[i0], &pxq[i0], &NSQ.sLPC_Q14[32 + i0], &NSQ.sLTP_shp_Q14[shp_idx0], &sLTP_Q15[ltp_idx0]);
                // the histories move by the four samples at once: [lpc_old (older 16) | lp (newer 16, newest first)], the delay line up to its order
#pragma unroll
                for (int j = 0; j < 16; j++) lpc_old[j] = j < 12 ? lpc_old[j + 4] : lp[27 - j];
#pragma unroll
                for (int j = 15; j >= 4; j--) lp[j] = lp[j - 4];
#pragma unroll
                for (int j = 0; j < 4; j++) lp[j] = o[3 - j].xq_Q14;
#pragma unroll
                for (int j = 15; j >= 0; j--) {
                    const i32 moved = j < 4 ? sv[3 - j] : ar[j - 4];
                    ar[j] = j < shapingLPCOrder ? moved : ar[j];
                }
            }
            continue;                                         // next subframe
        }
        // ---- short lags (never produced by the SILK pitch analysis, whose lags are >= 2 ms) and ragged subframes: the histories
        // shift per sample. The five outputs are still collected for four samples and written with one store each: nothing reads
        // them back within the group when lag >= 8 (or there is no pitch lag at all); otherwise the group is one sample.
        const bool ahead = lag >= 8;
        i32 xn = x_Q3[0], pn = 0, sn = 0;
        const int G = (ahead || lag <= 0) ? 4 : 1;
        for (int i0 = 0; i0 < subfr_length; i0 += G) {
            NsqSample o[4] = {};
            const int shp_idx0 = sLTP_shp_buf_idx, ltp_idx0 = sLTP_buf_idx;
            int cnt = 0;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = i0 + u;
                if (u >= G || i >= subfr_length) break;
                cnt = u + 1;
                const i32 xcur = xn;
                xn = x_Q3[i + 1 < subfr_length ? i + 1 : i];
                if (ahead) {
                    if (c.voiced) pn = sLTP_Q15[pred_lag + 1];
                    sn = NSQ.sLTP_shp_Q14[shp_lag + 1];
                }
                i32 LPC_pred_Q10 = predictLPCOrder >> 1;
#pragma unroll
                for (int j = 0; j < 10; j++) LPC_pred_Q10 = s_smlawb(LPC_pred_Q10, lp[j], a12[j]);
                if (predictLPCOrder == 16) {
#pragma unroll
                    for (int j = 10; j < 16; j++) LPC_pred_Q10 = s_smlawb(LPC_pred_Q10, lp[j], a12[j]);
                }
                // noise shape feedback: the sAR2 delay line shifts by one (NSQ.c:262-279)
                i32 tmp2 = lp[0], tmp1 = ar[0];
                ar[0] = tmp2;
                i32 n_AR_Q12 = shapingLPCOrder >> 1;
                n_AR_Q12 = s_smlawb(n_AR_Q12, tmp2, ar13[0]);
#pragma unroll
                for (int j = 2; j < 16; j += 2) {
                    if (j < shapingLPCOrder) {
                        tmp2 = ar[j - 1];
                        ar[j - 1] = tmp1;
                        n_AR_Q12 = s_smlawb(n_AR_Q12, tmp1, ar13[j - 1]);
                        tmp1 = ar[j];
                        ar[j] = tmp2;
                        n_AR_Q12 = s_smlawb(n_AR_Q12, tmp2, ar13[j]);
                    }
                }
                {
                    // ar[shapingLPCOrder-1] = tmp1 with a uniform (batch-wide) order: 10 or 16 in practice
                    i32 last_coef = 0;
#pragma unroll
                    for (int j = 1; j < 16; j += 2)
                        if (j == shapingLPCOrder - 1) { ar[j] = tmp1; last_coef = ar13[j]; }
                    n_AR_Q12 = s_smlawb(n_AR_Q12, tmp1, last_coef);
                }
                o[u] = nsq_sample(c, s, xcur, LPC_pred_Q10, n_AR_Q12, pn, sn);
                {
                    // the 32-sample history is [lpc_old (older 16) | lp (newer 16)]: the sample leaving lp enters lpc_old
                    const i32 leaving = lp[15];
#pragma unroll
                    for (int j = 0; j < 15; j++) lpc_old[j] = lpc_old[j + 1];
                    lpc_old[15] = leaving;
#pragma unroll
                    for (int j = 15; j > 0; j--) lp[j] = lp[j - 1];
                    lp[0] = o[u].xq_Q14;
                }
                sLTP_shp_buf_idx++;
                sLTP_buf_idx++;
                pred_lag++;
                shp_lag++;
            }
            if (cnt == 4) {
                nsq_store_group(o, &pl[i0], &pxq[i0], &NSQ.sLPC_Q14[32 + i0], &NSQ.sLTP_shp_Q14[shp_idx0], &sLTP_Q15[ltp_idx0]);
            } else {
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (u >= cnt) break;
                    pl[i0 + u] = (i8)o[u].pulse;
                    pxq[i0 + u] = (i16)o[u].xq;
                    NSQ.sLPC_Q14[32 + i0 + u] = o[u].xq_Q14;
                    NSQ.sLTP_shp_Q14[shp_idx0 + u] = o[u].shp_Q14;
                    sLTP_Q15[ltp_idx0 + u] = o[u].ltp_Q15;
                }
            }
            if (G == 1) {
                // a step may read what the step before it stored, so the taps are re-read from memory after every (single-sample) group
                nsq_store_fence();
                load_taps();
            }
        }
    }
    // ---- state write-back ----
#pragma unroll
    for (int j = 0; j < 16; j++) {
        NSQ.sAR2_Q14[j] = ar[j];
        NSQ.sLPC_Q14[j] = lpc_old[j];
        NSQ.sLPC_Q14[31 - j] = lp[j];
    }
    NSQ.sLF_AR_shp_Q14 = s.sLF_AR_shp_Q14;
    NSQ.lagPrev = in.pitchL[nb_subfr - 1];
    NSQ.sLTP_buf_idx = sLTP_buf_idx;
    NSQ.sLTP_shp_buf_idx = sLTP_shp_buf_idx;
    NSQ.rand_seed = s.rand_seed;
    NSQ.prev_gain_Q16 = prev_gain_Q16;
    NSQ.rewhite_flag = rewhite_flag;
    // silk_memmove of the histories (NSQ.c:176-177): ascending copy is safe (dst < src)
    if ((ltp_mem_length & 7) == 0 && (frame_length & 1) == 0) {
        nsq_move_run(reinterpret_cast<Q4 *>(NSQ.xq), reinterpret_cast<const Q4 *>(NSQ.xq + frame_length), ltp_mem_length / 8);
        nsq_move_run(reinterpret_cast<Q4 *>(NSQ.sLTP_shp_Q14), reinterpret_cast<const Q4 *>(NSQ.sLTP_shp_Q14 + frame_length), ltp_mem_length / 4);
    } else {
        for (int i = 0; i < ltp_mem_length; i++) NSQ.xq[i] = NSQ.xq[i + frame_length];
        for (int i = 0; i < ltp_mem_length; i++) NSQ.sLTP_shp_Q14[i] = NSQ.sLTP_shp_Q14[i + frame_length];
    }
}

}  // namespace ca
