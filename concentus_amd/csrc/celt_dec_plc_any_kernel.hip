// celt_dec_plc_any_kernel.hip -- the concealment stage of opusgpu_decode_batch_any (celt_plc.h), one wavefront per stream, in a unit
// of its own: next to celt_dec_plc_kernel in one unit the compiler allocated that kernel's registers differently.
#include "celt_plc.h"
#include "opusgpu_internal.h"

namespace ca {

// celt_dec_plc_kernel for a stream whose last packet was a 20 ms one; a stream lost after a shorter packet is
// concealed here in full, in steps of that packet's duration (celt_plc_short_steps: the steps depend on each other, so they cannot be
// spread over the later kernels), PCM included. The synthesis' working set lies next to the concealment's, 17 KB of LDS.
__global__ __launch_bounds__(64, 2) void celt_dec_plc_any_kernel(opusgpu_celt_dec_state *states, i16 *__restrict__ pcm, int n)
{
    __shared__ PlcLds P;
    __shared__ SynthLds L;
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        opusgpu_celt_dec_state *st = states + k;
        if (uni(st->mid_plc) == OPUSGPU_PLC_LOST) {
            if (uni(st->last_short) != 0 && uni(st->started)) celt_plc_short_steps(P, L, st, pcm + (size_t)k * FRAME * 2);
            else celt_plc_wave(P, st);
        }
        wave_sync();
    }
}

}  // namespace ca

extern "C" void opusgpu_launch_dec_plc_any(void *states, int16_t *pcm, int n, hipStream_t s)
{
    const int cus = opusgpu_num_cus();
    const int g = n < cus * 16 ? n : cus * 16;
    hipLaunchKernelGGL(ca::celt_dec_plc_any_kernel, dim3(g), dim3(64), 0, s, (opusgpu_celt_dec_state *)states, pcm, n);
}
