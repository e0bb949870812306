// celt_enc_kernel.hip -- batched Opus CELT-only encode for gfx950 (BASELINE config #3): opusgpu_encode_batch.
//
// One pipeline of five kernels per chunk of frames, each stage with the mapping of frames onto wavefronts it wants
// (DESIGN.md section 2); what a stage leaves for the next lies in a caller-provided HBM workspace, per frame one
// FrameMid record + the [2][1080] int32 time signal in_ws:
//   celt_dc_reject_kernel       pcm -> FrameMid.X (planar int16), hp_mem. Lane per (frame, channel), no LDS.
//                               (celt_stage_kernels.hip)
//   celt_front1_kernel          FrameMid.X, stream state -> in_ws after the pitch pre-filter; scalars + the first
//                               range-coder bytes -> FrameMid; in_mem / prefilter_mem of the stream. Wave per frame,
//                               13.9 KB LDS per workgroup, 11 wavefronts per CU.
//   celt_transient_tile_kernel  in_ws (twice) -> FrameMid.trans_unmask[2]. Lane per (frame, channel), 64 rows per
//                               wavefront tiled through LDS, 78.5 KB per workgroup, 2 wavefronts per CU.
//                               (celt_stage_kernels.hip)
//   celt_front2_kernel          in_ws, FrameMid -> MDCT, band energies, patch_transient_decision, normalised bands X
//                               -> FrameMid. Wave per frame, both channels through every lane loop together, 9.3 KB LDS
//                               per workgroup, 16 wavefronts per CU.
//   celt_back_lane_kernel       FrameMid -> packet, length, final range; the rest of the stream state (TF, coarse/fine
//                               energy, allocation, PVQ, range coder). Lane per frame, 64 frames per wavefront, 40.6 KB
//                               LDS per 64-frame workgroup, one wavefront per SIMD = 4 per CU.
//                               (celt_back_lane_kernel.hip)
// Batches larger than the workspace are processed in chunks on the same stream. Frames are independent units (streams
// advance one frame per call), so the batch shards across workgroups, CUs and GPUs with no communication.
// The first design -- one wavefront per frame end to end, celt_front_kernel + celt_back_kernel -- lives on as a
// cross-check in the diagnostic library (celt_enc_xcheck_diag.hip), not here.
//
// Replaces, for 48 kHz / 20 ms / restricted-lowdelay / fullband: opus_encode() (opus-fix/src/opus_encoder.c:2007)
// -> opus_encode_native (:938) -> celt_encode_with_ec (opus-fix/celt/celt_encoder.c:1379).
#include "celt_enc.h"
#include "opusgpu_internal.h"

namespace ca {

// The front phase in two kernels: phase 1 = rate bookkeeping .. pitch pre-filter, phase 2 = MDCT ..
// normalisation; the serial dc_reject and transient stages run in celt_stage_kernels.hip in between.
__global__ __launch_bounds__(64, 3) void celt_front1_kernel(opusgpu_celt_config cfg, opusgpu_celt_state *states,
                                                            FrameMid *__restrict__ mid, i32 *__restrict__ in_ws, int nframes)
{
    __shared__ Front1Lds F;
    for (int n = blockIdx.x; n < nframes; n += gridDim.x) {
        opusgpu_celt_state *st = states ? states + n : nullptr;
        i32 *in = in_ws + (size_t)n * 2 * (FRAME + OVL);
        if (lane() == 0) F.in_g = in;
        wave_sync();
        celt_encode_front_phase<1>(F, cfg, st, st, nullptr, mid + n, nullptr, in);
        wave_sync();
    }
}

// (64, 4): the register budget is set for 16 wavefronts per CU, and the working set has to admit as many (160 KB of LDS)
static_assert(sizeof(Front2Lds) * 16 <= 160 * 1024, "celt_front2_kernel: 16 wavefronts per CU");
__global__ __launch_bounds__(64, 4) void celt_front2_kernel(opusgpu_celt_config cfg, FrameMid *__restrict__ mid,
                                                            i32 *__restrict__ in_ws, int nframes)
{
    __shared__ Front2Lds F;
    for (int n = blockIdx.x; n < nframes; n += gridDim.x) {
        i32 *in = in_ws + (size_t)n * 2 * (FRAME + OVL);
        if (lane() == 0) { F.in_g = in; F.x_g = mid[n].X; }
        wave_sync();
        celt_encode_front_phase<2>(F, cfg, nullptr, nullptr, nullptr, mid + n, nullptr, in);
        wave_sync();
    }
}

// fresh encoder state (opus_encoder_create + OPUS_RESET_STATE, celt_encoder.c:2443-2462)
__global__ void celt_state_init_kernel(opusgpu_celt_state *states, int n)
{
    int i = blockIdx.x;
    if (i >= n) return;
    u32 *w = reinterpret_cast<u32 *>(&states[i]);
    for (int k = threadIdx.x; k < (int)(sizeof(opusgpu_celt_state) / 4); k += blockDim.x) w[k] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        states[i].spread_decision = SPREAD_NORMAL;
        states[i].delayedIntra = 1;
        states[i].tonal_average = 256;
    }
    for (int k = threadIdx.x; k < 2 * NB; k += blockDim.x) {
        states[i].oldLogE[k] = -28672;
        states[i].oldLogE2[k] = -28672;
    }
}

}  // namespace ca

using namespace ca;

static int config_ok(const opusgpu_celt_config *c)
{
    if (!c) return OPUSGPU_BAD_ARG;
    if (c->channels != 2 && c->channels != 1) return OPUSGPU_BAD_ARG;
    if (c->complexity < 0 || c->complexity > 10 || c->loss_rate < 0 || c->loss_rate > 100) return OPUSGPU_BAD_ARG;
    if (c->lsb_depth < 8 || c->lsb_depth > 24 || c->max_data_bytes <= 0) return OPUSGPU_BAD_ARG;
    if (c->bitrate <= 0) return OPUSGPU_BAD_ARG;
    // Only the operating region where the Opus layer's automatic decisions are constant is implemented:
    // stereo kept stereo (equiv_rate > stereo threshold 30 kb/s +- 1 kb/s hysteresis, opus_encoder.c:1121-1131)
    // and bandwidth stays FULLBAND (stereo music/voice thresholds <= 30 kb/s, :1263-1305).
    if (c->channels != 2 || c->bitrate < 32000) return OPUSGPU_UNIMPLEMENTED;
    // CBR: the packet size caps the rate the decisions see (cbrBytes, opus_encoder.c:1054-1061)
    if (!c->vbr) {
        int maxb = c->max_data_bytes < 1276 ? c->max_data_bytes : 1276;
        int cbr = (3 * c->bitrate / 8 + 75) / 150;
        if ((cbr < maxb ? cbr : maxb) * 400 < 32000) return OPUSGPU_UNIMPLEMENTED;
    }
    // PLC-frame corner (opus_encoder.c:1056-1084) and too-small buffers
    if (c->max_data_bytes < 3 || c->bitrate > 1276 * 400) return OPUSGPU_UNIMPLEMENTED;     // 510 400 = OPUS_BITRATE_MAX into a 1276-byte buffer
    return OPUSGPU_OK;
}

extern "C" int opusgpu_celt_state_size(void) { return (int)sizeof(opusgpu_celt_state); }

extern "C" int opusgpu_celt_state_init(void *d_states, int n_streams, void *stream)
{
    if (n_streams < 0) return OPUSGPU_BAD_ARG;
    if (n_streams == 0) return OPUSGPU_OK;
    if (!d_states) return OPUSGPU_BAD_ARG;
    hipLaunchKernelGGL(celt_state_init_kernel, dim3(n_streams), dim3(256), 0, (hipStream_t)stream,
                       (opusgpu_celt_state *)d_states, n_streams);
    return opusgpu_check_launch();
}

// per frame in flight: the FrameMid record + the [2][1080] int32 time signal handed from front phase 1 to 2
static const size_t WS_IN_BYTES = 2 * (FRAME + OVL) * sizeof(i32);
static const size_t WS_FRAME_BYTES = sizeof(FrameMid) + WS_IN_BYTES;

extern "C" size_t opusgpu_encode_workspace_bytes(int n_frames)
{
    return n_frames <= 0 ? 0 : (size_t)n_frames * WS_FRAME_BYTES;
}

// argument checks + workspace layout of opusgpu_encode_batch (opusgpu_internal.h): chunk FrameMid records, then chunk in_ws rows
extern "C" int opusgpu_encode_batch_args(const opusgpu_celt_config *cfg, const int16_t *d_pcm, const unsigned char *d_out, int out_stride,
                                         const int32_t *d_out_len, const uint32_t *d_out_rng, int n_frames, void *d_workspace,
                                         size_t workspace_bytes, size_t *chunk, int32_t **in_ws)
{
    *chunk = 0;
    *in_ws = nullptr;
    int rc = config_ok(cfg);
    if (rc != OPUSGPU_OK) return rc;
    if (n_frames < 0) return OPUSGPU_BAD_ARG;
    if (n_frames == 0) return OPUSGPU_OK;
    if (!d_pcm || !d_out || !d_out_len || !d_out_rng || !d_workspace) return OPUSGPU_BAD_ARG;
    int maxbytes = cfg->max_data_bytes < 1276 ? cfg->max_data_bytes : 1276;
    if (out_stride < ((maxbytes + 3) & ~3) || (out_stride & 3)) return OPUSGPU_BUFFER_TOO_SMALL;
    *chunk = workspace_bytes / WS_FRAME_BYTES;
    if (*chunk == 0) return OPUSGPU_BUFFER_TOO_SMALL;
    *in_ws = (int32_t *)((char *)d_workspace + *chunk * sizeof(FrameMid));
    return OPUSGPU_OK;
}

// persistent grids sized to what a CU holds: 13.9 KB of LDS per workgroup (11) / 9.3 KB at <= 128 VGPRs (16)
enum { FRONT1_WAVES = 11, FRONT2_WAVES = 16 };

extern "C" void opusgpu_launch_front1(const opusgpu_celt_config *cfg, void *states, void *mid, int32_t *in_ws, int n, hipStream_t s)
{
    const int cus = opusgpu_num_cus(), g = n < cus * FRONT1_WAVES ? n : cus * FRONT1_WAVES;
    hipLaunchKernelGGL(celt_front1_kernel, dim3(g), dim3(64), 0, s, *cfg, (opusgpu_celt_state *)states, (FrameMid *)mid, in_ws, n);
}

extern "C" void opusgpu_launch_front2(const opusgpu_celt_config *cfg, void *mid, int32_t *in_ws, int n, hipStream_t s)
{
    const int cus = opusgpu_num_cus(), g = n < cus * FRONT2_WAVES ? n : cus * FRONT2_WAVES;
    hipLaunchKernelGGL(celt_front2_kernel, dim3(g), dim3(64), 0, s, *cfg, (FrameMid *)mid, in_ws, n);
}

extern "C" int opusgpu_encode_batch(const opusgpu_celt_config *cfg, void *d_states, const int16_t *d_pcm,
                                    unsigned char *d_out, int out_stride, int32_t *d_out_len, uint32_t *d_out_rng,
                                    int n_frames, void *d_workspace, size_t workspace_bytes, void *stream)
{
    size_t chunk;
    int32_t *in_ws;
    int rc = opusgpu_encode_batch_args(cfg, d_pcm, d_out, out_stride, d_out_len, d_out_rng, n_frames, d_workspace, workspace_bytes,
                                       &chunk, &in_ws);
    if (rc != OPUSGPU_OK || n_frames == 0) return rc;
    opusgpu_celt_state *st = (opusgpu_celt_state *)d_states;
    void *mid = d_workspace;
    hipStream_t s = (hipStream_t)stream;
    for (size_t first = 0; first < (size_t)n_frames; first += chunk) {
        int n = (int)(((size_t)n_frames - first) < chunk ? ((size_t)n_frames - first) : chunk);
        opusgpu_celt_state *st_n = st ? st + first : nullptr;
        int slot = opusgpu_timing_begin(OPUSGPU_KERNEL_CELT_DC_REJECT, s);
        opusgpu_launch_dc_reject(st_n, d_pcm + first * FRAME * cfg->channels, mid, n, s);
        opusgpu_timing_end(slot, s);
        slot = opusgpu_timing_begin(OPUSGPU_KERNEL_CELT_FRONT1, s);
        opusgpu_launch_front1(cfg, st_n, mid, in_ws, n, s);
        opusgpu_timing_end(slot, s);
        slot = opusgpu_timing_begin(OPUSGPU_KERNEL_CELT_TRANSIENT, s);
        opusgpu_launch_transient(mid, in_ws, n, s);
        opusgpu_timing_end(slot, s);
        slot = opusgpu_timing_begin(OPUSGPU_KERNEL_CELT_FRONT2, s);
        opusgpu_launch_front2(cfg, mid, in_ws, n, s);
        opusgpu_timing_end(slot, s);
        slot = opusgpu_timing_begin(OPUSGPU_KERNEL_CELT_BACK_LANE, s);
        opusgpu_launch_back_lane(cfg, st_n, mid, d_out + first * (size_t)out_stride, out_stride, d_out_len + first, d_out_rng + first, n, s);
        opusgpu_timing_end(slot, s);
    }
    return opusgpu_check_launch();
}
