// celt_dec_packets_kernel.hip -- opusgpu_decode_batch_packets: batched opus_decode() for CELT-only packets of 1..48 frames (frame-count
// codes 0-3, padding, DTX frames), celt_dec_packets.h. After the parse (opus_packet_kernel.hip), pass f = 0 .. max_frames - 1 runs
// the pipeline of opusgpu_decode_batch_any on frame f of every stream that has one: the lane and post kernels below, the concealment
// of celt_dec_plc_packets_kernel.hip, and opusgpu_decode_batch_any's own synthesis kernel, which needs to know nothing of packets.
// A unit of its own: the kernels of celt_dec_kernel.hip keep the code and the registers they had.
#define CA_LANE_FRAME 1
#include "celt_lane_tables.h"
#include "celt_dec_packets.h"
#include "celt_dec_post.h"
#include "opusgpu_internal.h"

namespace ca {

// celt_decode_lane_kernel<A, true, true> (celt_dec_kernel.hip) for frame f of the parsed packets: the TOC, the frame's place and
// its size come from the stream's record. ret / rng were written by the parse for a rejected stream; an accepted stream's last
// frame writes rng.
template <int A>
__global__ __launch_bounds__(64 * (64 / A)) void celt_decode_lane_packets_kernel(opusgpu_celt_dec_state *states, const u8 *__restrict__ packets,
                                                                                 int packet_stride, opusgpu_packet_frames *frames, int f,
                                                                                 int *__restrict__ ret, u32 *__restrict__ rng, int n)
{
    fill_lds_tables();
    const int l = threadIdx.x & 63;
    if (l >= A) return;
    const int slot = (threadIdx.x >> 6) * A + l;
    const int k = blockIdx.x * 64 + slot;
    if (k >= n) return;
    const opusgpu_packet_frames *fr = frames + k;
    if (celt_packets_lane_skips(states + k, fr, f, rng + k)) return;
    DecWork F;
    F.lds_iy16 = (CA_AS_LDS i16 *)(g_lds_iy16 + slot);
    F.lds_pvq16 = (CA_AS_LDS i16 *)(g_lds_pvq16 + slot);
    // (a wavefront whose remaining streams all hold fullband stereo 20 ms frames runs the instantiation with all three fixed, as in
    // celt_decode_lane_kernel)
    // (what the frame needs of the record is read here; the record's address is formed again afterwards, not kept across the frame)
    const int toc = fr->toc & ~3, size = fr->size[f];
    const u8 *payload = packets + (size_t)k * packet_stride + fr->offset[f];
    const bool last = celt_packets_last_frame(fr, f);
    DecResult r;
    if (__builtin_amdgcn_ballot_w64(toc != 0xFC) == 0) r = celt_decode_front_frame<true>(F, states + k, toc, payload, size);
    else r = celt_decode_front_frame<false>(F, states + k, toc, payload, size);
    celt_packets_lane_result(frames + k, f, last, r, ret + k, rng + k);
}

// celt_decode_post_any_kernel for pass f: the stream's frame goes to its row of frame_size sample pairs at f * frame_samples.
// A DTX frame of 20 ms arrives here from celt_plc_wave like a lost packet; a shorter one is already written (OPUSGPU_PLC_DONE).
__global__ __launch_bounds__(256) void celt_decode_post_packets_kernel(opusgpu_celt_dec_state *states, const opusgpu_packet_frames *__restrict__ frames,
                                                                       int f, i16 *__restrict__ pcm, int frame_size, int n)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int k = t >> 1, c = t & 1;
    if (k >= n) return;
    opusgpu_celt_dec_state *st = states + k;
    const opusgpu_packet_frames *fr = frames + k;
    const int plc = st->mid_plc;
    if (plc == OPUSGPU_PLC_NONE && !st->mid_valid) return;
    i16 *out = pcm + ((size_t)k * frame_size + (size_t)f * fr->frame_samples) * 2;
    if (plc == OPUSGPU_PLC_ZEROS) {
        const int nz = celt_packets_zeros(fr);                                     // a multiple of 8: each lane clears half, 16 bytes at a time
        int4 *z = reinterpret_cast<int4 *>(out + c * nz);
        for (int j = 0; j < nz * 2 / 16; j++) z[j] = make_int4(0, 0, 0, 0);
    } else if (plc == OPUSGPU_PLC_PITCH) {
        celt_plc_tail_channel(st, c);
        celt_deemphasis_pair(st, c, out);
    } else if (st->mid_valid) {
        const int N = (FRAME / M8) << (st->mid_LM & 3);
        celt_postfilter_channel_any(st, c, N);
        celt_deemphasis_pair_any(st, c, out, N);
    }
}

}  // namespace ca

extern "C" void opusgpu_launch_packet_decide(const void *states, const unsigned char *d_packets, int packet_stride, const int32_t *d_len,
                                             opusgpu_packet_frames *d_frames, int frame_size, int max_frames, int32_t *d_ret,
                                             uint32_t *d_rng, int n, hipStream_t s);
extern "C" void opusgpu_launch_dec_plc_packets(void *states, const opusgpu_packet_frames *frames, int f, int16_t *pcm, int frame_size, int n,
                                               hipStream_t s);
extern "C" void opusgpu_launch_dec_synth_any(void *states, int n, hipStream_t s);

// opus_decode(st, data, len, pcm, frame_size, 0) for every stream (include/opusgpu.h)
extern "C" int opusgpu_decode_batch_packets(void *d_states, const unsigned char *d_packets, int packet_stride, const int32_t *d_len,
                                            int16_t *d_pcm, int frame_size, int max_frames, opusgpu_packet_frames *d_frames,
                                            int32_t *d_ret, uint32_t *d_rng, int n_streams, void *stream)
{
    if (n_streams < 0) return OPUSGPU_BAD_ARG;
    if (frame_size < 960 || frame_size > 5760 || frame_size % 120 != 0 || max_frames < 1 || max_frames > 48) return OPUSGPU_BAD_ARG;
    if (n_streams == 0) return OPUSGPU_OK;
    if (!d_states || !d_pcm || !d_frames || !d_ret || !d_rng) return OPUSGPU_BAD_ARG;
    if (d_len && (!d_packets || packet_stride <= 0)) return OPUSGPU_BAD_ARG;     // d_len == NULL: every stream is lost, no packets
    if (((uintptr_t)d_pcm & 15) != 0) return OPUSGPU_BAD_ARG;                    // (rows and frames then start on 16 bytes: 4 * 120 * k)
    if (!d_len) { d_packets = nullptr; packet_stride = 0; }
    hipStream_t s = (hipStream_t)stream;
    opusgpu_celt_dec_state *states = (opusgpu_celt_dec_state *)d_states;
    opusgpu_launch_packet_decide(d_states, d_packets, packet_stride, d_len, d_frames, frame_size, max_frames, d_ret, d_rng, n_streams, s);
    const int a = opusgpu_lane_frames(32);
    for (int f = 0; f < max_frames; f++) {
        int slot = opusgpu_timing_begin(OPUSGPU_KERNEL_DEC_LANE, s);
        {
            const dim3 grid((n_streams + 63) / 64), block(64 * (64 / a));
#define CA_LAUNCH(A) hipLaunchKernelGGL((ca::celt_decode_lane_packets_kernel<A>), grid, block, 0, s, states, d_packets, packet_stride, d_frames, f, \
                                        d_ret, d_rng, n_streams)
            if (a == 32) CA_LAUNCH(32);
            else CA_LAUNCH(64);
#undef CA_LAUNCH
        }
        opusgpu_timing_end(slot, s);
        slot = opusgpu_timing_begin(OPUSGPU_KERNEL_DEC_PLC, s);
        opusgpu_launch_dec_plc_packets(d_states, d_frames, f, d_pcm, frame_size, n_streams, s);
        opusgpu_timing_end(slot, s);
        slot = opusgpu_timing_begin(OPUSGPU_KERNEL_DEC_SYNTH, s);
        opusgpu_launch_dec_synth_any(d_states, n_streams, s);
        opusgpu_timing_end(slot, s);
        slot = opusgpu_timing_begin(OPUSGPU_KERNEL_DEC_POST, s);
        hipLaunchKernelGGL(ca::celt_decode_post_packets_kernel, dim3((2 * n_streams + 255) / 256), dim3(256), 0, s, states, d_frames, f, d_pcm,
                           frame_size, n_streams);
        opusgpu_timing_end(slot, s);
    }
    return opusgpu_check_launch();
}
