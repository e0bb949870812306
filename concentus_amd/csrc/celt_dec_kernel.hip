// celt_dec_kernel.hip -- batched opus_decode() for CELT-only 20 ms packets (mono or stereo, NB / WB / SWB / FB), one lane per stream.
//
// Replaces opus_decode() (opus-fix/src/opus_decoder.c:758; include/opus.h:462) -> opus_decode_native ->
// opus_decode_frame -> celt_decode_with_ec (celt/celt_decoder.c:713) for N streams at once. Decoding a
// packet is a serial chain (range decoder -> energies -> allocation -> PVQ), so that part uses the mapping of
// the encoder's back phase: 64 streams share a wavefront (celt_decode_lane_kernel, this file, LANES == 1 build).
// The synthesis has data parallelism inside a frame (denormalisation, inverse MDCT) and runs one wavefront per
// stream (celt_dec_synth_kernel.hip); the post-filter and de-emphasis are recurrences per channel and run one
// lane per (stream, channel) (celt_decode_post_kernel, this file). The stream state (decode_mem, energies,
// post-filter) and the hand-off between the three kernels live in opusgpu_celt_dec_state in HBM.
// opusgpu_decode_batch_plc is the same pipeline with packet loss concealment (celt_plc.h): the lane kernel marks the lost streams,
// celt_dec_plc_kernel (celt_dec_plc_kernel.hip) runs between it and the synthesis, and celt_decode_post_plc_kernel (this file)
// adds the concealment's per-channel recurrences to the post stage.
#define CA_LANE_FRAME 1
#include "celt_lane_tables.h"
#include "celt_plc.h"
#include "celt_dec_post.h"
#include "hook_host.h"                 // opusgpu_qab_dec_record: this unit holds the decode side of the quant_all_bands hook

namespace ca {

// A = streams per wavefront (64, or 32 / 16 with 2 / 4 partly filled waves per 64-stream workgroup; see
// celt_back_lane_kernel.hip)
// PLC (opusgpu_decode_batch_plc): a stream whose packet is lost (len == NULL or len[k] == 0) or is a DTX packet (one or two bytes) is left to
// the concealment kernels (celt_dec_plc_kernel.hip), which find it by st->mid_plc
// ANY (opusgpu_decode_batch_any, with PLC): the packets may be 2.5, 5, 10 or 20 ms long (celt_decode_front_as<FBS, true>); a lost
// packet is concealed as a 20 ms frame (mid_LM = 3) unless the stream's last packet was a shorter one (last_short)
template <int A, bool PLC, bool ANY = false>
__global__ __launch_bounds__(64 * (64 / A)) void celt_decode_lane_kernel(opusgpu_celt_dec_state *states, const u8 *__restrict__ packets,
                                                              int packet_stride, const int *__restrict__ len,
                                                              int *__restrict__ ret, u32 *__restrict__ rng, int n)
{
    fill_lds_tables();
    const int l = threadIdx.x & 63;
    if (l >= A) return;
    const int slot = (threadIdx.x >> 6) * A + l;
    const int k = blockIdx.x * 64 + slot;
    if (k >= n) return;
    DecWork F;
    F.lds_iy16 = (CA_AS_LDS i16 *)(g_lds_iy16 + slot);
    F.lds_pvq16 = (CA_AS_LDS i16 *)(g_lds_pvq16 + slot);
    const int ln = PLC && !len ? 0 : len[k];
    if (PLC) {
        const int toc = (ln == 1 || ln == 2) && packet_stride >= 1 ? packets[(size_t)k * packet_stride] : -1;
        const bool dtx = toc >= 0 && celt_plc_is_dtx(toc, ln);
        const bool lost = ln == 0 || dtx;
        states[k].mid_plc = lost ? OPUSGPU_PLC_LOST : OPUSGPU_PLC_NONE;
        if (lost) {
            // (a DTX packet's TOC says 20 ms; a loss after a shorter packet is concealed in steps by celt_dec_plc_any_kernel)
            if (ANY) { states[k].mid_LM = LM3; if (dtx) states[k].last_short = 0; }
            if (dtx) celt_plc_dtx_toc(states + k, toc);
            states[k].mid_valid = 0;
            states[k].final_range = 0;
            ret[k] = FRAME;
            rng[k] = 0;
            return;
        }
    }
    if (ln > packet_stride) {
        // a length past this stream's row would read the next stream's packet (or, for the last stream, past the slab)
        states[k].mid_valid = 0;
        ret[k] = OPUSGPU_BAD_ARG;
        rng[k] = states[k].final_range;
        return;
    }
    // The streams of a wavefront may differ in channel count and bandwidth, so both are run-time values of the lane -- unless
    // every stream still in this wavefront holds a fullband stereo packet: then the instantiation with both fixed runs, which is
    // the code the received-only fullband-stereo batch ran before the other TOCs were taken (3.07 ms against 3.15 ms for 65 536).
    const u8 *pkt = packets + (size_t)k * packet_stride;
    const bool other = ln < 2 || pkt[0] != 0xFC;
    DecResult r;
    if (__builtin_amdgcn_ballot_w64(other) == 0) r = celt_decode_front_as<true, ANY>(F, states + k, pkt, ln);
    else r = celt_decode_front_as<false, ANY>(F, states + k, pkt, ln);
    ret[k] = r.samples;
    rng[k] = r.final_range;
}

__device__ __forceinline__ void celt_decode_post_pair(opusgpu_celt_dec_state *st, int c, i16 *pcm)
{
    if (!st->mid_valid) return;
    celt_postfilter_channel(st, c);
    celt_deemphasis_pair(st, c, pcm);
}

__global__ __launch_bounds__(256) void celt_decode_post_kernel(opusgpu_celt_dec_state *states, i16 *__restrict__ pcm, int n)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = t >> 1, c = t & 1;
    if (k >= n) return;
    celt_decode_post_pair(states + k, c, pcm + (size_t)k * FRAME * 2);
}

// The post kernel of opusgpu_decode_batch_plc. A received stream (and one concealed from noise, which went through the synthesis)
// is treated as above; a stream in the pitch-based branch first gets the per-channel tail of celt_decode_lost (celt_plc.h:
// celt_iir, explosion check, TDAC fold); a stream without history gets zeros. Both lanes of a stream take the same way.
__global__ __launch_bounds__(256) void celt_decode_post_plc_kernel(opusgpu_celt_dec_state *states, i16 *__restrict__ pcm, int n)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = t >> 1, c = t & 1;
    if (k >= n) return;
    opusgpu_celt_dec_state *st = states + k;
    i16 *out = pcm + (size_t)k * FRAME * 2;
    const int plc = st->mid_plc;
    bool deemph = false;
    if (plc == OPUSGPU_PLC_ZEROS) {
        int4 *z = reinterpret_cast<int4 *>(out + c * FRAME);                 // each lane clears half of the stream's 3840 bytes
        for (int j = 0; j < FRAME * 2 / 16; j++) z[j] = make_int4(0, 0, 0, 0);
    } else if (plc == OPUSGPU_PLC_PITCH) {
        celt_plc_tail_channel(st, c);
        deemph = true;
    } else if (st->mid_valid) {
        celt_postfilter_channel(st, c);
        deemph = true;
    }
    if (deemph) celt_deemphasis_pair(st, c, out);
}

// The post kernel of opusgpu_decode_batch_any: as above, a received stream over the N = 120 << mid_LM samples of its frame. A
// concealed stream is a 20 ms frame (mid_LM == 3).
__global__ __launch_bounds__(256) void celt_decode_post_any_kernel(opusgpu_celt_dec_state *states, i16 *__restrict__ pcm, int n)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = t >> 1, c = t & 1;
    if (k >= n) return;
    opusgpu_celt_dec_state *st = states + k;
    i16 *out = pcm + (size_t)k * FRAME * 2;
    const int plc = st->mid_plc;
    if (plc == OPUSGPU_PLC_ZEROS) {
        int4 *z = reinterpret_cast<int4 *>(out + c * FRAME);
        for (int j = 0; j < FRAME * 2 / 16; j++) z[j] = make_int4(0, 0, 0, 0);
    } else if (plc == OPUSGPU_PLC_PITCH) {
        celt_plc_tail_channel(st, c);
        celt_deemphasis_pair(st, c, out);
    } else if (st->mid_valid) {
        const int N = (FRAME / M8) << (st->mid_LM & 3);
        celt_postfilter_channel_any(st, c, N);
        celt_deemphasis_pair_any(st, c, out, N);
    }
}

// fresh decoder state (opus_decoder_create + OPUS_RESET_STATE, celt_decoder.c:1177-1190)
__global__ void celt_dec_state_init_kernel(opusgpu_celt_dec_state *states, int n)
{
    const int i = blockIdx.x;
    if (i >= n) return;
    u32 *w = reinterpret_cast<u32 *>(&states[i]);
    for (int k = threadIdx.x; k < (int)(sizeof(opusgpu_celt_dec_state) / 4); k += blockDim.x) w[k] = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < 2 * NB; k += blockDim.x) {
        states[i].oldLogE[k] = -28672;
        states[i].oldLogE2[k] = -28672;
    }
}

// quant_all_bands(encode = 0) on its own (bands.c:1337-1502 as called at celt_decoder.c:977), for the per-call hook
// opusgpu_quant_all_bands: ONE lane of the lane build runs quant_all_bands_dec on a record -- the same code the batched
// decoder runs per stream.
__global__ __launch_bounds__(64) void quant_all_bands_dec_hook_kernel(opusgpu_qab_dec_record *rec)
{
    fill_lds_tables();
    if (threadIdx.x != 0) return;
    DecWork F;
    F.lds_iy16 = (CA_AS_LDS i16 *)(g_lds_iy16);
    F.lds_pvq16 = (CA_AS_LDS i16 *)(g_lds_pvq16);
    F.X = (x16_t *)rec->X;
    F.norm = (x16_t *)rec->norm;
    F.diag = nullptr;
    for (int k = 0; k < NB; k++) { F.pulses[k] = rec->pulses[k]; F.tf_res[k] = rec->tf_res[k]; }
    for (int k = 0; k < 2 * NB; k++) F.collapse_masks[k] = 0;
    RangeDec dec;
    dec.buf = rec->buf;
    load(dec, rec->ec);
    u32 seed = rec->seed;
    quant_all_bands_dec(F, dec, rec->shortBlocks, rec->spread, rec->dual_stereo, rec->intensity, rec->total_bits, rec->balance,
                        rec->codedBands, &seed, 2, NB);
    for (int k = 0; k < 2 * NB; k++) rec->collapse_masks[k] = F.collapse_masks[k];
    rec->seed = seed;
    store(rec->ec, dec);
}

}  // namespace ca

extern "C" int opusgpu_launch_quant_all_bands_dec(opusgpu_qab_dec_record *d_rec)
{
    hipLaunchKernelGGL(ca::quant_all_bands_dec_hook_kernel, dim3(1), dim3(64), 0, 0, d_rec);
    return opusgpu_check_launch();
}

extern "C" void opusgpu_launch_dec_synth(void *states, int n, hipStream_t s);

extern "C" int opusgpu_celt_dec_state_size(void) { return (int)sizeof(opusgpu_celt_dec_state); }

extern "C" int opusgpu_celt_dec_state_init(void *d_states, int n_streams, void *stream)
{
    if (n_streams < 0 || (n_streams > 0 && !d_states)) return OPUSGPU_BAD_ARG;
    if (n_streams == 0) return OPUSGPU_OK;
    hipLaunchKernelGGL(ca::celt_dec_state_init_kernel, dim3(n_streams), dim3(256), 0, (hipStream_t)stream,
                       (opusgpu_celt_dec_state *)d_states, n_streams);
    return opusgpu_check_launch();
}

extern "C" void opusgpu_launch_dec_plc(void *states, int n, hipStream_t s);
extern "C" void opusgpu_launch_dec_synth_any(void *states, int n, hipStream_t s);
extern "C" void opusgpu_launch_dec_plc_any(void *states, int16_t *pcm, int n, hipStream_t s);

// The pipeline of the batched entry points, arguments checked: the lane kernel, with PLC the concealment's wave-per-stream kernel
// (it leaves at once on a received stream), the synthesis, and the post kernel of the matching kind; each in its timing bracket.
template <bool PLC, bool ANY = false>
static int decode_batch_launch(void *d_states, const unsigned char *d_packets, int packet_stride, const int32_t *d_len, int16_t *d_pcm,
                               int32_t *d_ret, uint32_t *d_rng, int n_streams, hipStream_t s)
{
    int slot = opusgpu_timing_begin(OPUSGPU_KERNEL_DEC_LANE, s);
    {
        const int a = opusgpu_lane_frames(32);          // (decoder lane kernel: 5.06 ms at 32 streams per wavefront, 5.39 ms at 64)
        const dim3 grid((n_streams + 63) / 64), block(64 * (64 / a));
#define CA_LAUNCH(A) hipLaunchKernelGGL((ca::celt_decode_lane_kernel<A, PLC, ANY>), grid, block, 0, s, (opusgpu_celt_dec_state *)d_states, \
                                        d_packets, packet_stride, d_len, d_ret, d_rng, n_streams)
        if (a == 32) CA_LAUNCH(32);
        else CA_LAUNCH(64);
#undef CA_LAUNCH
    }
    opusgpu_timing_end(slot, s);
    if (PLC) {
        slot = opusgpu_timing_begin(OPUSGPU_KERNEL_DEC_PLC, s);
        if (ANY) opusgpu_launch_dec_plc_any(d_states, d_pcm, n_streams, s);
        else opusgpu_launch_dec_plc(d_states, n_streams, s);
        opusgpu_timing_end(slot, s);
    }
    slot = opusgpu_timing_begin(OPUSGPU_KERNEL_DEC_SYNTH, s);
    if (ANY) opusgpu_launch_dec_synth_any(d_states, n_streams, s);
    else opusgpu_launch_dec_synth(d_states, n_streams, s);
    opusgpu_timing_end(slot, s);
    slot = opusgpu_timing_begin(OPUSGPU_KERNEL_DEC_POST, s);
    const auto post = ANY ? ca::celt_decode_post_any_kernel : PLC ? ca::celt_decode_post_plc_kernel : ca::celt_decode_post_kernel;
    hipLaunchKernelGGL(post, dim3((2 * n_streams + 255) / 256), dim3(256), 0, s, (opusgpu_celt_dec_state *)d_states, d_pcm, n_streams);
    opusgpu_timing_end(slot, s);
    return opusgpu_check_launch();
}

extern "C" int opusgpu_decode_batch(void *d_states, const unsigned char *d_packets, int packet_stride, const int32_t *d_len,
                                    int16_t *d_pcm, int32_t *d_ret, uint32_t *d_rng, int n_streams, void *stream)
{
    if (n_streams < 0) return OPUSGPU_BAD_ARG;
    if (n_streams == 0) return OPUSGPU_OK;
    if (!d_states || !d_packets || !d_len || !d_pcm || !d_ret || !d_rng || packet_stride <= 0) return OPUSGPU_BAD_ARG;
    if (((uintptr_t)d_pcm & 15) != 0) return OPUSGPU_BAD_ARG;         // the post kernel stores 16 bytes at a time
    return decode_batch_launch<false>(d_states, d_packets, packet_stride, d_len, d_pcm, d_ret, d_rng, n_streams, (hipStream_t)stream);
}

// opusgpu_decode_batch with packet loss concealment (the post kernel knows about concealed streams)
extern "C" int opusgpu_decode_batch_plc(void *d_states, const unsigned char *d_packets, int packet_stride, const int32_t *d_len,
                                        int16_t *d_pcm, int32_t *d_ret, uint32_t *d_rng, int n_streams, void *stream)
{
    if (n_streams < 0) return OPUSGPU_BAD_ARG;
    if (n_streams == 0) return OPUSGPU_OK;
    if (!d_states || !d_pcm || !d_ret || !d_rng) return OPUSGPU_BAD_ARG;
    if (d_len && (!d_packets || packet_stride <= 0)) return OPUSGPU_BAD_ARG;     // d_len == NULL: every stream is lost, no packets
    if (((uintptr_t)d_pcm & 15) != 0) return OPUSGPU_BAD_ARG;
    if (!d_len) { d_packets = nullptr; packet_stride = 0; }
    return decode_batch_launch<true>(d_states, d_packets, packet_stride, d_len, d_pcm, d_ret, d_rng, n_streams, (hipStream_t)stream);
}

// opusgpu_decode_batch_plc for every code-0 CELT-only packet: 2.5, 5, 10 and 20 ms frames, in any mix (include/opusgpu.h)
extern "C" int opusgpu_decode_batch_any(void *d_states, const unsigned char *d_packets, int packet_stride, const int32_t *d_len,
                                        int16_t *d_pcm, int32_t *d_ret, uint32_t *d_rng, int n_streams, void *stream)
{
    if (n_streams < 0) return OPUSGPU_BAD_ARG;
    if (n_streams == 0) return OPUSGPU_OK;
    if (!d_states || !d_pcm || !d_ret || !d_rng) return OPUSGPU_BAD_ARG;
    if (d_len && (!d_packets || packet_stride <= 0)) return OPUSGPU_BAD_ARG;
    if (((uintptr_t)d_pcm & 15) != 0) return OPUSGPU_BAD_ARG;
    if (!d_len) { d_packets = nullptr; packet_stride = 0; }
    return decode_batch_launch<true, true>(d_states, d_packets, packet_stride, d_len, d_pcm, d_ret, d_rng, n_streams, (hipStream_t)stream);
}
