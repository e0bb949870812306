// opus_packet_kernel.hip -- opus_packet_parse() for a batch (opus_packet.h), one lane per stream: opusgpu_packet_parse_batch, and
// the first launch of opusgpu_decode_batch_packets, which also decides what each stream gets (celt_dec_packets.h).
// A lane reads its own packet's bytes one at a time; nothing here is worth more than that (a packet's framing is a few bytes).
#include "celt_dec_packets.h"
#include "opusgpu_internal.h"

namespace ca {

// DECIDE: the parse of opusgpu_decode_batch_packets. len == NULL: every stream is lost. A rejected stream gets its answer here and
// is left alone by every pass; an accepted one gets the sample count now and its final range from its last frame.
template <bool DECIDE>
__global__ __launch_bounds__(64) void opus_packet_parse_kernel(const u8 *__restrict__ packets, int packet_stride, const int *__restrict__ len,
                                                               opusgpu_packet_frames *__restrict__ frames, int n,
                                                               const opusgpu_celt_dec_state *__restrict__ states, int frame_size,
                                                               int max_frames, int *__restrict__ ret, u32 *__restrict__ rng)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    opusgpu_packet_frames *fr = frames + k;
    const int ln = DECIDE && !len ? 0 : len[k];
    const int count = opus_packet_parse_stream(packets + (size_t)k * packet_stride, ln, packet_stride, fr);
    if (DECIDE) {
        const int r = celt_packets_decide(fr, count, frame_size, max_frames);
        ret[k] = r;
        if (r < 0) rng[k] = states[k].final_range;
    } else {
        fr->pad_ = 0;
    }
}

}  // namespace ca

extern "C" void opusgpu_launch_packet_decide(const void *states, const unsigned char *d_packets, int packet_stride, const int32_t *d_len,
                                             opusgpu_packet_frames *d_frames, int frame_size, int max_frames, int32_t *d_ret,
                                             uint32_t *d_rng, int n, hipStream_t s)
{
    hipLaunchKernelGGL(ca::opus_packet_parse_kernel<true>, dim3((n + 63) / 64), dim3(64), 0, s, d_packets, packet_stride, d_len, d_frames, n,
                       (const opusgpu_celt_dec_state *)states, frame_size, max_frames, d_ret, d_rng);
}

extern "C" int opusgpu_packet_parse_batch(const unsigned char *d_packets, int packet_stride, const int32_t *d_len,
                                          opusgpu_packet_frames *d_frames, int n_streams, void *stream)
{
    if (n_streams < 0) return OPUSGPU_BAD_ARG;
    if (n_streams == 0) return OPUSGPU_OK;
    if (!d_packets || !d_len || !d_frames || packet_stride <= 0) return OPUSGPU_BAD_ARG;
    hipLaunchKernelGGL(ca::opus_packet_parse_kernel<false>, dim3((n_streams + 63) / 64), dim3(64), 0, (hipStream_t)stream, d_packets,
                       packet_stride, d_len, d_frames, n_streams, (const opusgpu_celt_dec_state *)nullptr, 0, 0, (int *)nullptr,
                       (ca::u32 *)nullptr);
    return opusgpu_check_launch();
}
