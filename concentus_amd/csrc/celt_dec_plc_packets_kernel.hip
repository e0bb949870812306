// celt_dec_plc_packets_kernel.hip -- the concealment stage of opusgpu_decode_batch_packets (celt_dec_packets.h: celt_packets_conceal),
// one wavefront per stream, in a unit of its own like celt_dec_plc_any_kernel, whose working set it shares (17 KB of LDS).
#include "celt_dec_packets.h"
#include "opusgpu_internal.h"

namespace ca {

// Pass f: a stream the lane kernel marked lost is a lost packet (concealed for 960 samples from the row's start) or holds a DTX
// frame f (concealed for the TOC's duration at the frame's place); every other wavefront leaves after one load.
__global__ __launch_bounds__(64, 2) void celt_dec_plc_packets_kernel(opusgpu_celt_dec_state *states, const opusgpu_packet_frames *__restrict__ frames,
                                                                     int f, i16 *__restrict__ pcm, int frame_size, int n)
{
    __shared__ PlcLds P;
    __shared__ SynthLds L;
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        celt_packets_conceal(P, L, states + k, frames + k, f, pcm + (size_t)k * frame_size * 2);
        wave_sync();
    }
}

}  // namespace ca

extern "C" void opusgpu_launch_dec_plc_packets(void *states, const opusgpu_packet_frames *frames, int f, int16_t *pcm, int frame_size, int n,
                                               hipStream_t s)
{
    const int cus = opusgpu_num_cus();
    const int g = n < cus * 16 ? n : cus * 16;
    hipLaunchKernelGGL(ca::celt_dec_plc_packets_kernel, dim3(g), dim3(64), 0, s, (opusgpu_celt_dec_state *)states, frames, f, pcm, frame_size, n);
}
