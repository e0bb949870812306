// pitch_hooks.hip -- celt_pitch_xcorr() with the reference's own argument list, as a per-call hook (host pointers).
//
// opus-fix/celt/pitch.c:214-258 (celt_pitch_xcorr), the CELT_PITCH_XCORR_IMPL[] table entry of celt/pitch.h:186-204:
//   xcorr[i] = sum_j x[j] * y[i + j]   (MAC16_16 in wrapping 32-bit arithmetic),  i < max_pitch,  j < len
//   returns max(1, max_i xcorr[i])
// Inside the frame encoder the same sums are computed by the front kernel on LDS-resident buffers (celt_enc_front.h);
// this entry point exists so the reference's RTCD slot has a target, for plumbing and parity. One lane per lag, x
// staged in LDS, the maximum by a wave reduction and one atomic per wavefront.
#include "fixmath.h"
#include "hook_host.h"

namespace ca {

enum { XCORR_MAX_LEN = 2048 };

__global__ __launch_bounds__(256) void pitch_xcorr_kernel(const i16 *__restrict__ x, const i16 *__restrict__ y,
                                                          i32 *__restrict__ xcorr, int len, int max_pitch, i32 *maxcorr)
{
    // the sums go through dot2_i16, two products at a time (the primitive of the front kernel's pitch loops, driven here at
    // the caller's values): x staged as pairs, an odd len padded with a zero sample; y packed from its two halves, since
    // y + i is only 2-byte aligned
    __shared__ __attribute__((aligned(4))) i16 xs[XCORR_MAX_LEN];
    for (int j = threadIdx.x; j < len; j += blockDim.x) xs[j] = x[j];
    if ((len & 1) && threadIdx.x == 0) xs[len] = 0;                                  // len odd => len < XCORR_MAX_LEN
    __syncthreads();
    const u32a *xw = reinterpret_cast<const u32a *>(xs);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    i32 sum = (i32)0x80000000;
    if (i < max_pitch) {
        i32 acc = 0;
        for (int j = 0; j + 1 < len; j += 2) acc = dot2_i16(xw[j >> 1], pack_i16(y[i + j], y[i + j + 1]), acc);
        if (len & 1) acc = dot2_i16(xw[len >> 1], pack_i16(y[i + len - 1], 0), acc);
        sum = acc;
        xcorr[i] = sum;
    }
    const i32 m = wave_max(sum);
    if ((threadIdx.x & 63) == 0) atomicMax(maxcorr, m);
}

}  // namespace ca

extern "C" int32_t opusgpu_celt_pitch_xcorr(const int16_t *x, const int16_t *y, int32_t *xcorr, int len, int max_pitch, int arch)
{
    (void)arch;
    if (!x || !y || !xcorr || len < 1 || len > ca::XCORR_MAX_LEN || max_pitch < 1) { fail(OPUSGPU_BAD_ARG); return 0; }
    const size_t xb = (size_t)len * 2, yb = (size_t)(len + max_pitch - 1) * 2, cb = (size_t)max_pitch * 4;
    int32_t h_m = 1;                                                                           // maxcorr starts at 1 (pitch.c:224)
    DevBuf dx(xb), dy(yb), dc(cb), dm(4);
    int rc = allocated(dx, dy, dc, dm);
    if (rc == OPUSGPU_OK) rc = h2d(dx.p, x, xb);
    if (rc == OPUSGPU_OK) rc = h2d(dy.p, y, yb);
    if (rc == OPUSGPU_OK) rc = h2d(dm.p, &h_m, 4);
    if (rc == OPUSGPU_OK) {
        hipLaunchKernelGGL(ca::pitch_xcorr_kernel, dim3((max_pitch + 255) / 256), dim3(256), 0, 0, (const ca::i16 *)dx.p, (const ca::i16 *)dy.p,
                           (ca::i32 *)dc.p, len, max_pitch, (ca::i32 *)dm.p);
        rc = opusgpu_check_launch();
    }
    if (rc == OPUSGPU_OK) rc = d2h(xcorr, dc.p, cb);
    if (rc == OPUSGPU_OK) rc = d2h(&h_m, dm.p, 4);
    return fail(rc) == OPUSGPU_OK ? h_m : 0;
}
