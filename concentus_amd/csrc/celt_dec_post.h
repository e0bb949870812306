// celt_dec_post.h -- the per-channel post stage of the batched decoder on the device, one lane per (stream, channel): the pitch
// post-filter and the de-emphasis as the post kernels of celt_dec_kernel.hip and celt_dec_packets_kernel.hip run them. Device
// only (the two lanes of a stream exchange samples by DPP); the host emulation runs celt_decode_post_channel (celt_dec.h).
#pragma once
#include "celt_dec.h"

namespace ca {

// celt_decode_post_channel (celt_dec.h) for the lane pair (2k, 2k+1) = the two channels of stream k. The post-filter is the
// same code; the de-emphasis (celt_decoder.c:183-285) runs in blocks of 32 samples -- eight 16-byte loads issued together, the
// recurrence over them, then the stores -- and the two lanes exchange their outputs (DPP) so that each writes interleaved
// stereo 16 bytes at a time: a load, the recurrence step and a 2-byte store per sample was one exposed memory round trip per
// sample (loads queue behind stores), 960 per channel and most of this kernel's 0.70 ms.
__device__ __forceinline__ void celt_postfilter_channel(opusgpu_celt_dec_state *st, int c)
{
    const int N = FRAME;
    i32 *out_syn = st->decode_mem[c] + DEC_BUF - N;
    comb_filter_inplace_dec(out_syn, st->mid_pf_period_old, st->mid_pf_period, 120, st->mid_pf_gain_old, st->mid_pf_gain,
                            st->mid_pf_tapset_old, st->mid_pf_tapset);
    comb_filter_inplace_dec(out_syn + 120, st->mid_pf_period, st->mid_pf_period_new, N - 120, st->mid_pf_gain, st->mid_pf_gain_new,
                            st->mid_pf_tapset, st->mid_pf_tapset_new);
}

// G groups of eight samples from j0 on (G = 4: the block of 32 above)
template <int G>
__device__ __forceinline__ void celt_deemphasis_block(const int4 *src, int j0, i32 &m, int c, i16 *pcm)
{
    {
        int4 in[2 * G];
#pragma unroll
        for (int q = 0; q < 2 * G; q++) in[q] = src[(j0 >> 2) + q];
        int4 res[G];
#pragma unroll
        for (int g = 0; g < G; g++) {
            const i32 w[8] = {in[2 * g].x, in[2 * g].y, in[2 * g].z, in[2 * g].w, in[2 * g + 1].x, in[2 * g + 1].y, in[2 * g + 1].z, in[2 * g + 1].w};
            u32 v[8], o[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const i32 t = add32(w[k], m);
                m = mul16_32_q15(27853, t);
                i32 x = pshr32(t, 12);
                x = imax(x, -32768);
                x = imin(x, 32767);
                v[k] = (u32)x & 0xffffu;
                o[k] = (u32)__builtin_amdgcn_update_dpp(0, (int)v[k], 0xB1, 0xF, 0xF, false);     // quad_perm [1,0,3,2]: the other channel
            }
            // channel 0's lane writes the group's stereo pairs 0..3, channel 1's lane pairs 4..7
            u32 pr[4];
#pragma unroll
            for (int i = 0; i < 4; i++) pr[i] = c ? (o[4 + i] | (v[4 + i] << 16)) : (v[i] | (o[i] << 16));
            res[g] = make_int4((int)pr[0], (int)pr[1], (int)pr[2], (int)pr[3]);
        }
#pragma unroll
        for (int g = 0; g < G; g++) *reinterpret_cast<int4 *>(pcm + 2 * (j0 + 8 * g + 4 * c)) = res[g];
    }
}

__device__ __forceinline__ void celt_deemphasis_pair(opusgpu_celt_dec_state *st, int c, i16 *pcm)
{
    const int N = FRAME;
    const i32 *out_syn = st->decode_mem[c] + DEC_BUF - N;
    i32 m = st->preemph_memD[c];
    const int4 *src = reinterpret_cast<const int4 *>(out_syn);
    for (int j0 = 0; j0 < N; j0 += 32) celt_deemphasis_block<4>(src, j0, m, c, pcm);
    st->preemph_memD[c] = m;
}

// ... of a frame of N = 120, 240, 480 or 960 samples: blocks of 32, then the groups of eight that are left (N is a multiple of
// eight, so every store is 16 bytes inside the first N sample pairs of the row; the rest of the row is not written)
__device__ __forceinline__ void celt_deemphasis_pair_any(opusgpu_celt_dec_state *st, int c, i16 *pcm, int N)
{
    const i32 *out_syn = st->decode_mem[c] + DEC_BUF - N;
    i32 m = st->preemph_memD[c];
    const int4 *src = reinterpret_cast<const int4 *>(out_syn);
    int j0 = 0;
    for (; j0 + 32 <= N; j0 += 32) celt_deemphasis_block<4>(src, j0, m, c, pcm);
    for (; j0 < N; j0 += 8) celt_deemphasis_block<1>(src, j0, m, c, pcm);
    st->preemph_memD[c] = m;
}

}  // namespace ca
