// opusgpu_internal.h -- helpers shared by the translation units of libopusgpu.so (not exported API).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/opusgpu.h"

extern "C" void opusgpu_set_last_error(int err);
// hipGetLastError() mapped to an OPUSGPU_* code
extern "C" int opusgpu_check_launch(void);
// optional per-kernel timing (see opusgpu_kernel_timing_enable); slot -1 = timing off
extern "C" int opusgpu_timing_begin(int kernel, hipStream_t s);
extern "C" void opusgpu_timing_end(int slot, hipStream_t s);
// frames (streams) per wavefront of the lane-per-frame kernels: 64 or 32 (OPUSGPU_LANE_FRAMES overrides the kernel's default)
extern "C" int opusgpu_lane_frames(int dflt);
// device counter of SILK records whose header failed the bounds checks (silk_validate.h); nullptr = allocation failed
extern "C" int *opusgpu_bad_record_counter(void);
extern "C" int opusgpu_private_bad_counter_begin(void);
extern "C" int opusgpu_private_bad_counter_end(void);
// Argument checks of opusgpu_encode_batch: the configuration inside the supported region, pointers, strides, workspace. Returns an
// error code, or OPUSGPU_OK with *chunk = frames per pass of the pipeline (what the workspace holds; 0 when n_frames == 0: nothing
// to do) and *in_ws = the time-signal rows of the workspace, which follow its chunk FrameMid records.
extern "C" int opusgpu_encode_batch_args(const opusgpu_celt_config *cfg, const int16_t *d_pcm, const unsigned char *d_out, int out_stride,
                                         const int32_t *d_out_len, const uint32_t *d_out_rng, int n_frames, void *d_workspace,
                                         size_t workspace_bytes, size_t *chunk, int32_t **in_ws);
// The five stages of opusgpu_encode_batch, in order, on n frames of one chunk (mid, in_ws: the workspace): grid sizing + launch.
// Defined in celt_stage_kernels.hip (dc_reject, transient), celt_enc_kernel.hip (front1, front2), celt_back_lane_kernel.hip.
extern "C" void opusgpu_launch_dc_reject(const void *states, const int16_t *pcm, void *mid, int n, hipStream_t s);
extern "C" void opusgpu_launch_front1(const opusgpu_celt_config *cfg, void *states, void *mid, int32_t *in_ws, int n, hipStream_t s);
extern "C" void opusgpu_launch_transient(void *mid, const int32_t *in_ws, int n, hipStream_t s);
extern "C" void opusgpu_launch_front2(const opusgpu_celt_config *cfg, void *mid, int32_t *in_ws, int n, hipStream_t s);
extern "C" void opusgpu_launch_back_lane(const opusgpu_celt_config *cfg, void *states, const void *mid, unsigned char *out,
                                         int out_stride, int32_t *out_len, uint32_t *out_rng, int n, hipStream_t s);
// Records per wavefront of the lane-per-record SILK analysis kernels whose work arrays live in scratch memory (silk_pitch_kernels.hip,
// silk_nlsf_kernels.hip). They are bound by the latency of one record's serial chain, not by issue slots, so partially filled
// wavefronts (16 or 32 records: more wavefronts per SIMD) were swept against the full one (64), which is what ships.
enum { SILK_LANES_PER_BLOCK = 64 };
