// silk_kernels.hip -- the two SILK fixed-point inner loops named by the north star, batched over
// function-boundary records (BASELINE config #4).
//
//   silk_burg_kernel  <- silk_burg_modified_c        silk_burg_dev.h (opus-fix/silk/fixed/burg_modified_FIX.c:45-275)
//   silk_nsq_kernel   <- silk_NSQ_c                  silk_nsq_dev.h, which carries the line numbers of opus-fix/silk/NSQ.c
//
// The kernels here select a record, check its header (silk_validate.h) and call the device function.
//
// Mapping: both loops are recurrences that are serial in their own index (Burg: order n depends on
// order n-1; NSQ: sample i feeds back into sample i+1 through four filters), with only ~16-wide inner
// products. A wavefront per record would leave 48 lanes idle and pay a cross-lane reduction per
// sample, so here ONE LANE owns ONE record and a wavefront advances 64 independent records in
// lock-step: the loop trip counts (order, subframe length) are the same for every record of a batch, so
// the wave stays converged, per-lane temporaries are indexed uniformly (scratch accesses coalesce), the
// short filter states (sAR2, the last 16 sLPC samples) live in registers, and the only divergent
// addresses are the pitch-lag taps.
//
// Arithmetic: the reference's x86-64 build uses the 64-bit macro forms (OPUS_FAST_INT64, silk/macros.h:47-102);
// 16x32 products are evaluated on split halves (full-rate 24-bit multiplier), 32x32 ones as 64-bit.
#include <string.h>
#include "silk_burg_dev.h"
#include "silk_nsq_dev.h"
#include "hook_host.h"
#include "../../include/opusgpu_silk.h"
#include "silk_validate.h"

namespace ca {


// ---- silk_burg_modified: one lane per record --------------------------------------------------------
// A record's samples x[384] are read ~25 times each (16 autocorrelation lags, then both ends of every subframe in
// every order of the recursion). From HBM that is a 2-byte load per use at a 784-byte stride between lanes -- one cache
// line per lane per instruction. The wavefront instead copies its 64 records' samples into LDS once (16-byte loads),
// laid out [sample][lane], and every later use is a conflict-free LDS read.
struct BurgX {
    const i16 *p;                                              // this lane's column of the [sample][lane] block
    __device__ __forceinline__ i32 operator[](int k) const { return p[k * 64]; }
    __device__ __forceinline__ BurgX operator+(int o) const { BurgX r; r.p = p + o * 64; return r; }
};

__global__ __launch_bounds__(64) void silk_burg_kernel(const opusgpu_burg_in *__restrict__ recs, opusgpu_burg_out *__restrict__ outs, int n_rec,
                                                       int *__restrict__ bad_records)
{
    __shared__ i16 edge_s[BURG_EDGE_SLOTS * 64];               // the recursion's subframe edges, [slot][lane]: 16 KB, four workgroups per CU
    i16 xs[OPUSGPU_SILK_BURG_MAX_X];                           // private: the energy and lag-product passes read it once each, in order
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= n_rec) return;
    const opusgpu_burg_in &in = recs[r];
    if (!burg_record_ok(in)) {                                 // would index xs[] / the order-16 arrays out of bounds
        opusgpu_burg_out &o = outs[r];
        o.res_nrg = 0;
        o.res_nrg_Q = (i32)0x80000000;
        for (int k = 0; k < 16; k++) o.A_Q16[k] = 0;
        atomicAdd(bad_records, 1);
        return;
    }
    {
        static_assert(sizeof(opusgpu_burg_in) % 16 == 0 && OPUSGPU_SILK_BURG_MAX_X % 8 == 0, "16-byte loads of x");
        const int nx = in.subfr_length * in.nb_subfr;
        const int4 *src = reinterpret_cast<const int4 *>(in.x);
        for (int k = 0; k < nx; k += 8) {
            const int4 w = src[k >> 3];
            xs[k + 0] = (i16)w.x; xs[k + 1] = (i16)(w.x >> 16); xs[k + 2] = (i16)w.y; xs[k + 3] = (i16)(w.y >> 16);
            xs[k + 4] = (i16)w.z; xs[k + 5] = (i16)(w.z >> 16); xs[k + 6] = (i16)w.w; xs[k + 7] = (i16)(w.w >> 16);
        }
    }
    BurgEdgesCol e;
    e.p = edge_s + threadIdx.x;
    e.stage((const i16 *)xs, in.subfr_length, in.nb_subfr);
    silk_burg_modified_dev((const i16 *)xs, e, in.minInvGain_Q30, in.subfr_length, in.nb_subfr, in.D, outs[r].A_Q16, &outs[r].res_nrg, &outs[r].res_nrg_Q);
}

// ---- silk_NSQ: one lane per record (silk_nsq_dev.h) -------------------------------------------------------
// ws: per-record scratch in HBM (the scaled re-whitened prediction buffer)
__global__ __launch_bounds__(64) void silk_nsq_kernel(const opusgpu_nsq_in *__restrict__ recs, opusgpu_nsq_state *__restrict__ states,
                                                      opusgpu_nsq_out *__restrict__ outs, NsqScratch *__restrict__ ws, int n_rec,
                                                      int *__restrict__ bad_records, const int *__restrict__ rows)
{
    int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= n_rec) return;
    if (rows) r = rows[r];                                     // the bitrate loop's second passes: a list of frames, in place
    const opusgpu_nsq_in &in = recs[r];
    opusgpu_nsq_state &NSQ = states[r];
    if (!nsq_record_ok(in, NSQ.lagPrev)) {                     // state untouched, no pulses
        for (int k = 0; k < OPUSGPU_SILK_MAX_FRAME; k++) outs[r].pulses[k] = 0;
        atomicAdd(bad_records, 1);
        return;
    }
    silk_nsq_record_dev(in, NSQ, outs[r].pulses, ws[r].sLTP_Q15);
}

}  // namespace ca

using namespace ca;

extern "C" int opusgpu_silk_burg_modified_batch(const opusgpu_burg_in *d_in, opusgpu_burg_out *d_out, int n, void *stream)
{
    if (n < 0) return OPUSGPU_BAD_ARG;
    if (n == 0) return OPUSGPU_OK;
    if (!d_in || !d_out) return OPUSGPU_BAD_ARG;
    int *bad = opusgpu_bad_record_counter();
    if (!bad) return OPUSGPU_ALLOC_FAIL;
    hipLaunchKernelGGL(silk_burg_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, d_in, d_out, n, bad);
    return opusgpu_check_launch();
}

extern "C" size_t opusgpu_silk_nsq_workspace_bytes(int n) { return n <= 0 ? 0 : (size_t)n * sizeof(NsqScratch); }

extern "C" int opusgpu_silk_nsq_batch(const opusgpu_nsq_in *d_in, opusgpu_nsq_state *d_state, opusgpu_nsq_out *d_out, int n,
                                      void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (n < 0) return OPUSGPU_BAD_ARG;
    if (n == 0) return OPUSGPU_OK;
    if (!d_in || !d_state || !d_out || !d_workspace) return OPUSGPU_BAD_ARG;
    if (workspace_bytes < (size_t)n * sizeof(NsqScratch)) return OPUSGPU_BUFFER_TOO_SMALL;
    int *bad = opusgpu_bad_record_counter();
    if (!bad) return OPUSGPU_ALLOC_FAIL;
    hipLaunchKernelGGL(silk_nsq_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, d_in, d_state, d_out,
                       (NsqScratch *)d_workspace, n, bad, (const int *)nullptr);
    return opusgpu_check_launch();
}

// records d_rows[0 .. m) of the arrays, in place (workspace sized for the whole arrays): silk_chain.hip's bitrate loop
extern "C" int opusgpu_silk_nsq_rows(const opusgpu_nsq_in *d_in, opusgpu_nsq_state *d_state, opusgpu_nsq_out *d_out, const int *d_rows, int m,
                                     void *d_workspace, hipStream_t stream)
{
    if (m <= 0) return m < 0 ? OPUSGPU_BAD_ARG : OPUSGPU_OK;
    int *bad = opusgpu_bad_record_counter();
    if (!bad) return OPUSGPU_ALLOC_FAIL;
    hipLaunchKernelGGL(silk_nsq_kernel, dim3((m + 63) / 64), dim3(64), 0, stream, d_in, d_state, d_out, (NsqScratch *)d_workspace, m, bad, d_rows);
    return opusgpu_check_launch();
}

// Per-call hook with the reference's own signature (macro silk_burg_modified -> silk_burg_modified_c,
// opus-fix/silk/SigProc_FIX.h:601-602, fixed/burg_modified_FIX.c:45): host pointers, one record, synchronous.
// Plumbing / parity only -- a launch per call is latency-bound; throughput comes from the batch entry point.
extern "C" void opusgpu_silk_burg_modified_c(int32_t *res_nrg, int *res_nrg_Q, int32_t A_Q16[], const int16_t x[],
                                             const int32_t minInvGain_Q30, const int subfr_length, const int nb_subfr,
                                             const int D, int arch)
{
    (void)arch;
    if (!res_nrg || !res_nrg_Q || !A_Q16 || !x || D < 1 || D > OPUSGPU_SILK_MAX_ORDER || nb_subfr < 1 || subfr_length <= D ||
        subfr_length * nb_subfr > OPUSGPU_SILK_BURG_MAX_X) {
        fail(OPUSGPU_BAD_ARG);
        return;
    }
    opusgpu_burg_in h_in;
    opusgpu_burg_out h_out;
    memset(&h_in, 0, sizeof(h_in));
    memcpy(h_in.x, x, sizeof(int16_t) * (size_t)subfr_length * nb_subfr);
    h_in.minInvGain_Q30 = minInvGain_Q30; h_in.subfr_length = subfr_length; h_in.nb_subfr = nb_subfr; h_in.D = D;
    // Unchecked: the arguments were checked above and the out record has no status word
    const int rc = fail(run_record<Unchecked>(&h_in, &h_out, (NoState *)nullptr, [](const opusgpu_burg_in *i, NoState *, opusgpu_burg_out *o) {
        return opusgpu_silk_burg_modified_batch(i, o, 1, nullptr);
    }));
    if (rc != OPUSGPU_OK) return;
    *res_nrg = h_out.res_nrg;
    *res_nrg_Q = h_out.res_nrg_Q;
    memcpy(A_Q16, h_out.A_Q16, sizeof(int32_t) * (size_t)D);
}
