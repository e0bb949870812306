// celt_state.h -- per-stream encoder state and per-batch parameters of the CELT frame path.
//
// CeltEncState is the pointer-free equivalent of everything the reference keeps between frames for one
// stream: the fields of `struct OpusCustomEncoder` past ENCODER_RESET_START plus its trailing arrays
// (opus-fix/celt/celt_encoder.c:82-128) and the Opus layer's dc_reject memory (src/opus_encoder.c:86,
// hp_mem). It lives in HBM (one record per stream); a frame kernel loads it, encodes one 20 ms frame
// and stores it back. A NULL state pointer means "every frame is the first frame of its own stream"
// (SURVEY.md 8d): the reset values below are then materialised in registers/LDS and nothing is stored.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/opusgpu.h"   /* opusgpu_celt_config */

#ifdef __cplusplus
extern "C" {
#endif

#define OPUSGPU_CELT_NBANDS 21
#define OPUSGPU_CELT_OVERLAP 120
#define OPUSGPU_CELT_FRAME 960
#define OPUSGPU_COMBFILTER_MAXPERIOD 1024
#define OPUSGPU_COMBFILTER_MINPERIOD 15

typedef struct opusgpu_celt_state {
    /* Opus layer (src/opus_encoder.c) */
    int32_t hp_mem[4];              /* dc_reject memories, 2 per channel */
    /* CELT layer, scalars (celt_encoder.c:82-120) */
    uint32_t rng;
    int32_t spread_decision;
    int32_t delayedIntra;
    int32_t tonal_average;
    int32_t lastCodedBands;
    int32_t hf_average;
    int32_t tapset_decision;
    int32_t prefilter_period;
    int32_t prefilter_gain;         /* opus_val16 */
    int32_t prefilter_tapset;
    int32_t consec_transient;
    int32_t preemph_memE[2];
    int32_t vbr_reservoir;
    int32_t vbr_drift;
    int32_t vbr_offset;
    int32_t vbr_count;
    int32_t overlap_max;
    int32_t stereo_saving;          /* opus_val16 */
    int32_t intensity;
    int32_t spec_avg;               /* opus_val16 */
    int32_t reserved[5];
    /* CELT layer, arrays (celt_encoder.c:123-127) */
    int16_t oldBandE[2 * OPUSGPU_CELT_NBANDS];
    int16_t oldLogE[2 * OPUSGPU_CELT_NBANDS];
    int16_t oldLogE2[2 * OPUSGPU_CELT_NBANDS];
    int16_t pad16[2];
    int32_t in_mem[2 * OPUSGPU_CELT_OVERLAP];
    int32_t prefilter_mem[2 * OPUSGPU_COMBFILTER_MAXPERIOD];
} opusgpu_celt_state;

/* Decoder counterpart: everything `struct OpusCustomDecoder` keeps past DECODER_RESET_START for a stereo
 * stream (opus-fix/celt/celt_decoder.c:66-97 and the trailing arrays :94-96). `lpc` and `last_pitch_index`
 * belong to the packet loss concealment (celt_decode_lost, celt_plc.h): the synthesis filter of the first lost
 * frame and its pitch, reused by the losses that follow it. `started` is the Opus layer's "prev_mode != 0"
 * (src/opus_decoder.c:259-268): set by every decoded packet, cleared by init/reset; a loss before it is zeros.
 * `last_end` and `last_channels` are the Opus layer's st->bandwidth and st->stream_channels as the CELT decoder sees them
 * (src/opus_decoder.c:431-450, :683-686): the end band (13, 17, 19, 21) and the channel count (1, 2) of the last packet's TOC,
 * which a lost packet is concealed with. 0 (init / reset) reads as 21 / stereo.
 * `last_short` is the Opus layer's st->frame_size as far as it matters here (src/opus_decoder.c:250, :685): LM + 1 of the last
 * packet opusgpu_decode_batch_any decoded when that was shorter than 20 ms, else 0. A loss after such a packet is concealed in
 * steps of that packet's duration. Only opusgpu_decode_batch_any reads or writes it. */
#define OPUSGPU_DECODE_BUFFER_SIZE 2048
#define OPUSGPU_CELT_LPC_ORDER 24
typedef struct opusgpu_celt_dec_state {
    uint32_t rng;
    int32_t error;
    int32_t postfilter_period, postfilter_period_old;
    int32_t postfilter_gain, postfilter_gain_old;          /* opus_val16 */
    int32_t postfilter_tapset, postfilter_tapset_old;
    int32_t preemph_memD[2];
    int32_t loss_count;
    int32_t last_pitch_index;
    int32_t started;
    int32_t last_end, last_channels;
    uint32_t final_range;                                  /* OPUS_GET_FINAL_RANGE: the last accepted packet's, 0 after a concealed frame */
    int16_t oldBandE[2 * OPUSGPU_CELT_NBANDS];
    int16_t oldLogE[2 * OPUSGPU_CELT_NBANDS];
    int16_t oldLogE2[2 * OPUSGPU_CELT_NBANDS];
    int16_t backgroundLogE[2 * OPUSGPU_CELT_NBANDS];
    int16_t lpc[2][OPUSGPU_CELT_LPC_ORDER];
    int32_t decode_mem[2][OPUSGPU_DECODE_BUFFER_SIZE + OPUSGPU_CELT_OVERLAP];
    /* hand-off between the kernels of one opusgpu_decode_batch call (not stream state): the decoded normalised
     * bands, what the synthesis and post-filter kernels need to know about the frame, and the per-stream result */
    int16_t mid_X[2 * OPUSGPU_CELT_FRAME];
    int16_t mid_norm[2 * 624];                             /* the frame's folding source (bands.c norm / norm2): working storage of the lane kernel */
    int32_t mid_valid, mid_isTransient, mid_silence;               /* (the frame's end band is last_end) */
    int32_t mid_pf_period_old, mid_pf_period, mid_pf_period_new;
    int32_t mid_pf_gain_old, mid_pf_gain, mid_pf_gain_new;
    int32_t mid_pf_tapset_old, mid_pf_tapset, mid_pf_tapset_new;
    /* ... of one opusgpu_decode_batch_plc call: what the concealment still owes this stream (OPUSGPU_PLC_*), and the energy
     * S1 of the signal whose excitation the pitch-based branch copied (celt_decoder.c:629-634), per channel */
    int32_t mid_plc;
    int32_t mid_plc_S1[2];
    int32_t mid_mono;                                      /* the frame is one coded channel, synthesised into both (celt_decoder.c:313-325) */
    /* ... of one opusgpu_decode_batch_any call: the frame is 120 << mid_LM samples (3 for a concealed one). The other entry
     * points neither read nor write these four words. */
    int32_t mid_LM;
    int32_t last_short;
    int32_t reserved_any[2];
} opusgpu_celt_dec_state;

/* mid_plc: the stream was received / is lost and not yet looked at / has no history (zeros) / is synthesised from noise by
 * the ordinary synthesis / waits for the per-channel tail of the pitch-based branch (celt_iir onwards) */
#define OPUSGPU_PLC_NONE 0
#define OPUSGPU_PLC_LOST 1
#define OPUSGPU_PLC_ZEROS 2
#define OPUSGPU_PLC_NOISE 3
#define OPUSGPU_PLC_PITCH 4
#define OPUSGPU_PLC_DONE 5    /* opusgpu_decode_batch_any: concealed in steps and already written (celt_plc_short_steps) */

#ifdef __cplusplus
/* the synthesis kernel moves decode_mem in 16-byte units, and the records of a batch lie back to back */
static_assert(offsetof(opusgpu_celt_dec_state, decode_mem) % 16 == 0, "decode_mem must stay 16-byte aligned");
static_assert(sizeof(opusgpu_celt_dec_state) % 16 == 0, "sizeof(opusgpu_celt_dec_state) must stay a multiple of 16");
static_assert(offsetof(opusgpu_celt_dec_state, last_end) == 52 && offsetof(opusgpu_celt_dec_state, oldBandE) == 64,
              "last_end / last_channels / final_range took the reserved words: no offset may move");
static_assert(offsetof(opusgpu_celt_dec_state, mid_LM) == 24240 && sizeof(opusgpu_celt_dec_state) == 24256,
              "mid_LM / last_short were appended behind mid_mono: no offset before them may move");
#endif

#ifdef __cplusplus
}
#endif
