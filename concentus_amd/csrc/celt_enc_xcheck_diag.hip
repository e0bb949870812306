// celt_enc_xcheck_diag.hip -- CROSS-CHECK builds of stages of opusgpu_encode_batch: the kernels the product pipeline
// superseded, kept in the diagnostic library so that tests can run the pipeline with one stage swapped for its older
// mapping and compare packets. Plain builds (no stage stamps): the fused front phase and the wave-per-frame back phase
// are the first design (one wavefront per frame end to end, ~23 KB / ~9.6 KB of LDS per workgroup), the streaming
// transient kernel is what celt_transient_tile_kernel replaced. Never used for reported throughput.
#include "celt_enc.h"
#include "celt_stage_lane.h"
#include "opusgpu_internal.h"
#include "../../include/opusgpu_diag.h"

namespace ca {

__global__ __launch_bounds__(64, 2) void celt_front_kernel(opusgpu_celt_config cfg, opusgpu_celt_state *states,
                                                           const i16 *__restrict__ pcm, FrameMid *__restrict__ mid, int nframes)
{
    __shared__ FrontLds F;
    for (int n = blockIdx.x; n < nframes; n += gridDim.x) {
        opusgpu_celt_state *st = states ? states + n : nullptr;
        celt_encode_front(F, cfg, st, st, pcm + (size_t)n * FRAME * cfg.channels, mid + n);
        wave_sync();
    }
}

__global__ __launch_bounds__(64, 4) void celt_back_kernel(opusgpu_celt_config cfg, opusgpu_celt_state *states,
                                                          const FrameMid *__restrict__ mid, u8 *__restrict__ out, int out_stride,
                                                          int *__restrict__ out_len, u32 *__restrict__ out_rng, int nframes)
{
    __shared__ BackLds F;
    for (int n = blockIdx.x; n < nframes; n += gridDim.x) {
        opusgpu_celt_state *st = states ? states + n : nullptr;
        FrameResult r = celt_encode_back(F, cfg, mid + n, st, out + (size_t)n * out_stride);
        if (lane() == 0) {
            out_len[n] = r.bytes;
            out_rng[n] = r.final_range;
        }
        wave_sync();
    }
}

// transient metric per channel: in_ws [n][2][1080] int32 -> mid[f].trans_unmask[c]; mid[f].X is scratch here
__global__ __launch_bounds__(256) void celt_transient_kernel(FrameMid *__restrict__ mid, const i32 *__restrict__ in_ws, int nframes)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int f = t >> 1, c = t & 1;
    if (f >= nframes) return;
    mid[f].trans_unmask[c] = stage_transient_channel(in_ws + ((size_t)f * 2 + c) * (FRAME + OVL), mid[f].X + c * FRAME);
}

}  // namespace ca

using namespace ca;

// opusgpu_encode_batch with the stages named in `variant` replaced; every other stage is the product library's own launcher
extern "C" int opusgpu_encode_batch_xcheck(const opusgpu_celt_config *cfg, void *d_states, const int16_t *d_pcm,
                                           unsigned char *d_out, int out_stride, int32_t *d_out_len, uint32_t *d_out_rng,
                                           int n_frames, void *d_workspace, size_t workspace_bytes, unsigned variant, void *stream)
{
    const unsigned fused = variant & OPUSGPU_XCHECK_FRONT_FUSED, wave = variant & OPUSGPU_XCHECK_BACK_WAVE,
                   tlane = variant & OPUSGPU_XCHECK_TRANSIENT_LANE;
    if ((variant & ~(OPUSGPU_XCHECK_FRONT_FUSED | OPUSGPU_XCHECK_BACK_WAVE | OPUSGPU_XCHECK_TRANSIENT_LANE)) || (fused && tlane))
        return OPUSGPU_BAD_ARG;                             // the fused front phase has no transient stage to replace
    size_t chunk;
    int32_t *in_ws;
    int rc = opusgpu_encode_batch_args(cfg, d_pcm, d_out, out_stride, d_out_len, d_out_rng, n_frames, d_workspace, workspace_bytes,
                                       &chunk, &in_ws);
    if (rc != OPUSGPU_OK || n_frames == 0) return rc;
    const int cus = opusgpu_num_cus();
    opusgpu_celt_state *st = (opusgpu_celt_state *)d_states;
    FrameMid *mid = (FrameMid *)d_workspace;
    hipStream_t s = (hipStream_t)stream;
    for (size_t first = 0; first < (size_t)n_frames; first += chunk) {
        int n = (int)(((size_t)n_frames - first) < chunk ? ((size_t)n_frames - first) : chunk);
        int g1 = n < cus * 7 ? n : cus * 7;          // 22.8 KB LDS per workgroup -> 7 resident per CU (measured best)
        int g2 = n < cus * 16 ? n : cus * 16;        // ~9.6 KB LDS per workgroup -> 16 resident per CU
        opusgpu_celt_state *st_n = st ? st + first : nullptr;
        const int16_t *pcm_n = d_pcm + first * FRAME * cfg->channels;
        if (fused) {
            hipLaunchKernelGGL(celt_front_kernel, dim3(g1), dim3(64), 0, s, *cfg, st_n, pcm_n, mid, n);
        } else {
            opusgpu_launch_dc_reject(st_n, pcm_n, mid, n, s);
            opusgpu_launch_front1(cfg, st_n, mid, in_ws, n, s);
            if (tlane)
                hipLaunchKernelGGL(celt_transient_kernel, dim3((2 * n + 255) / 256), dim3(256), 0, s, mid, in_ws, n);
            else
                opusgpu_launch_transient(mid, in_ws, n, s);
            opusgpu_launch_front2(cfg, mid, in_ws, n, s);
        }
        if (wave)
            hipLaunchKernelGGL(celt_back_kernel, dim3(g2), dim3(64), 0, s, *cfg, st_n, mid, d_out + first * (size_t)out_stride,
                               out_stride, d_out_len + first, d_out_rng + first, n);
        else
            opusgpu_launch_back_lane(cfg, st_n, mid, d_out + first * (size_t)out_stride, out_stride, d_out_len + first,
                                     d_out_rng + first, n, s);
    }
    return opusgpu_check_launch();
}
