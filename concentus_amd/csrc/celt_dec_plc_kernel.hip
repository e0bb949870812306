// celt_dec_plc_kernel.hip -- packet loss concealment of the batched decoder, the stage with parallelism inside a frame
// (celt_plc.h, celt_plc_wave: opus-fix/celt/celt_decoder.c:395-635 of celt_decode_lost) with one wavefront per stream, between the
// lane kernel and the synthesis of opusgpu_decode_batch_plc. The lane kernel marks the lost streams (mid_plc); a wavefront that
// finds its stream received leaves after one load. The pitch buffers, the excitation and the LPC work arrays are 9.5 KB of LDS.
#include "celt_plc.h"
#include "opusgpu_internal.h"

namespace ca {

__global__ __launch_bounds__(64, 2) void celt_dec_plc_kernel(opusgpu_celt_dec_state *states, int n)
{
    __shared__ PlcLds P;
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        celt_plc_wave(P, states + k);
        wave_sync();
    }
}

}  // namespace ca

extern "C" void opusgpu_launch_dec_plc(void *states, int n, hipStream_t s)
{
    const int cus = opusgpu_num_cus();
    const int g = n < cus * 16 ? n : cus * 16;
    hipLaunchKernelGGL(ca::celt_dec_plc_kernel, dim3(g), dim3(64), 0, s, (opusgpu_celt_dec_state *)states, n);
}
