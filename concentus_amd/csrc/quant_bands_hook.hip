// quant_bands_hook.hip -- quant_all_bands() with the reference's own argument list as a per-call hook (include/opusgpu_hooks.h).
//
// One wavefront, the wave-per-frame build of the encoder sources: the caller's arguments are packed into one record, the
// kernel unpacks it into the BackLds working set (normalised bands, band energies, pulses, tf_res, the range coder's buffer),
// runs quant_all_bands_wave (celt_enc_back.h: bands.c:1337-1502 with quant_band / quant_band_stereo / quant_partition /
// compute_theta / alg_quant / encode_pulses and the ec_enc_* calls they make) and hands the coder state and buffer back.
// The host steps (mirrors of ec_ctx / CELTMode, the coder's fields, device buffer, heap record) are hook_host.h's.
#include "celt_enc.h"
#include "hook_host.h"
#include "../../include/opusgpu_hooks.h"

namespace ca {

struct QabRecord {
    i16 X[2 * FRAME];
    i32 bandE[2 * NB];
    i32 pulses[NB], tf_res[NB];
    i32 shortBlocks, spread, dual_stereo, intensity, total_bits, balance, codedBands, pad;
    EcFields ec;
    i32 pad2;
    u8 buf[1280];
};

__global__ __launch_bounds__(64) void quant_all_bands_hook_kernel(QabRecord *rec)
{
    __shared__ BackLds F;
    if (lane() == 0) F.diag = nullptr;
    for (int k = lane(); k < 2 * FRAME; k += LANES) F.x16[k] = rec->X[k];
    for (int k = lane(); k < 2 * NB; k += LANES) F.bandE[k] = rec->bandE[k];
    for (int k = lane(); k < NB; k += LANES) { F.pulses[k] = rec->pulses[k]; F.tf_res[k] = rec->tf_res[k]; }
    const u32 storage = uni(rec->ec.storage);
    for (u32 k = lane(); k < storage; k += LANES) F.packet[1 + k] = rec->buf[k];
    RangeEnc enc;
    enc.buf = F.packet + 1;
    load(enc, rec->ec);
    wave_sync();
    quant_all_bands_wave(F, enc, 2, uni(rec->shortBlocks), uni(rec->spread), uni(rec->dual_stereo), uni(rec->intensity),
                         uni(rec->total_bits), uni(rec->balance), uni(rec->codedBands));
    wave_sync();
    for (u32 k = lane(); k < storage; k += LANES) rec->buf[k] = F.packet[1 + k];
    if (lane() == 0) store(rec->ec, enc);
}

}  // namespace ca

extern "C" void opusgpu_quant_all_bands(int encode, const void *m, int start, int end, int16_t *X, int16_t *Y, unsigned char *collapse_masks,
                                        const int32_t *bandE, int *pulses, int shortBlocks, int spread, int dual_stereo, int intensity,
                                        int *tf_res, int32_t total_bits, int32_t balance, void *ec, int LM, int codedBands, uint32_t *seed,
                                        int arch)
{
    (void)arch;
    if (!m || !X || (encode && !bandE) || !pulses || !tf_res || !ec) { fail(OPUSGPU_BAD_ARG); return; }
    const ref_celt_mode_head *mh = (const ref_celt_mode_head *)m;
    ref_ec_ctx *e = (ref_ec_ctx *)ec;
    if ((encode != 0 && encode != 1) || !Y || start != 0 || end != 21 || LM != 3 || mh->Fs != 48000 || mh->overlap != 120 || mh->nbEBands != 21 ||
        e->storage > 1275 || !e->buf || (shortBlocks != 0 && shortBlocks != 8)) {
        fail(OPUSGPU_UNIMPLEMENTED);
        return;
    }
    if (!encode) {
        // decoder side (celt_decoder.c:977): the range DEcoder reads ec->buf, X / Y receive the decoded normalised bands,
        // collapse_masks and *seed are outputs the caller uses afterwards (anti_collapse, st->rng)
        if (!collapse_masks || !seed) { fail(OPUSGPU_BAD_ARG); return; }
        HeapRec<opusgpu_qab_dec_record> h;
        if (!h.p) { fail(OPUSGPU_ALLOC_FAIL); return; }
        for (int k = 0; k < 21; k++) { h->pulses[k] = pulses[k]; h->tf_res[k] = tf_res[k]; }
        h->shortBlocks = shortBlocks; h->spread = spread; h->dual_stereo = dual_stereo; h->intensity = intensity;
        h->total_bits = total_bits; h->balance = balance; h->codedBands = codedBands; h->seed = *seed;
        h->ec = ec_fields_from(e);
        memcpy(h->buf, e->buf, e->storage);
        const int rc = fail(run_in_place(h.p, sizeof(opusgpu_qab_dec_record), [](void *d) {
            return opusgpu_launch_quant_all_bands_dec((opusgpu_qab_dec_record *)d);
        }));
        if (rc != OPUSGPU_OK) return;
        memcpy(X, h->X, sizeof(int16_t) * 960);
        memcpy(Y, h->X + 960, sizeof(int16_t) * 960);
        memcpy(collapse_masks, h->collapse_masks, 42);
        *seed = h->seed;
        ec_fields_to(e, h->ec);
        return;
    }
    (void)collapse_masks; (void)seed;
    static_assert(sizeof(((ca::QabRecord *)nullptr)->buf) >= 1276, "range coder buffer");
    HeapRec<ca::QabRecord> h;                                                     // 6.4 KB: kept off a codec thread's stack
    if (!h.p) { fail(OPUSGPU_ALLOC_FAIL); return; }
    memcpy(h->X, X, sizeof(int16_t) * 960);
    memcpy(h->X + 960, Y, sizeof(int16_t) * 960);
    memcpy(h->bandE, bandE, sizeof(int32_t) * 42);
    for (int k = 0; k < 21; k++) { h->pulses[k] = pulses[k]; h->tf_res[k] = tf_res[k]; }
    h->shortBlocks = shortBlocks; h->spread = spread; h->dual_stereo = dual_stereo; h->intensity = intensity;
    h->total_bits = total_bits; h->balance = balance; h->codedBands = codedBands;
    h->ec = ec_fields_from(e);
    memcpy(h->buf, e->buf, e->storage);
    const int rc = fail(run_in_place(h.p, sizeof(ca::QabRecord), [](void *d) {
        hipLaunchKernelGGL(ca::quant_all_bands_hook_kernel, dim3(1), dim3(64), 0, 0, (ca::QabRecord *)d);
        return opusgpu_check_launch();
    }));
    if (rc != OPUSGPU_OK) return;
    memcpy(e->buf, h->buf, e->storage);
    ec_fields_to(e, h->ec);
}
