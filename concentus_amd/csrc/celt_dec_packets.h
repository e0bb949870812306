// celt_dec_packets.h -- the frame loop of opus_decode_native (opus-fix/src/opus_decoder.c:598-709) for opusgpu_decode_batch_packets:
// CELT-only packets of 1..48 frames (frame-count codes 0-3, padding), parsed by opus_packet.h.
//
// The loop is unrolled over launches: pass f decodes frame f of every stream that has one, through the four kernels of
// opusgpu_decode_batch_any, into the stream's PCM row at f * frame_samples. What a stream gets is decided ONCE, before pass 0
// (celt_packets_decide): the call's answer d_ret, and in the record's spare byte `pad_` how many passes the stream takes part in --
// so a packet is decoded whole or not at all. A frame of at most one byte is a DTX frame, concealed for the TOC's own duration
// (src/opus_decoder.c:245-251): 20 ms in the one step of opusgpu_decode_batch_plc, shorter in one step of celt_plc_short_steps.
#pragma once
#include "celt_plc.h"
#include "opus_packet.h"

namespace ca {

// fr->pad_ after the decision: 0 = the stream is rejected (no pass touches it), 1..48 = frames to decode, PKT_RUN_LOST = the
// packet is lost and pass 0 conceals 960 samples as opusgpu_decode_batch_any does
enum { PKT_RUN_LOST = 0xFF };

// What the call answers for a stream whose packet parsed to `count` (opus_packet_parse_stream's return value), in the reference's
// order (src/opus_decoder.c:636-680: the parser's error, then the PCM row's size), then this decoder's own limits.
CA_DEV int celt_packets_decide(opusgpu_packet_frames *fr, int count, int frame_size, int max_frames)
{
    fr->pad_ = 0;
    if (count == 0) { fr->pad_ = PKT_RUN_LOST; return FRAME; }
    if (count < 0) return count;
    if (count * fr->frame_samples > frame_size) return OPUSGPU_BUFFER_TOO_SMALL;
    if (!celt_toc_accepted_any(fr->toc & ~3)) { CA_COUNT("multi_not_celt", 1); return OPUSGPU_UNIMPLEMENTED; }   // SILK, hybrid
    if (count > max_frames) { CA_COUNT("multi_over_max_frames", 1); return OPUSGPU_UNIMPLEMENTED; }            // (our limit, not the reference's)
    fr->pad_ = (uint8_t)count;
    return count * fr->frame_samples;
}

CA_DEV bool celt_packets_has_frame(const opusgpu_packet_frames *fr, int f) { return fr->pad_ != PKT_RUN_LOST && f < fr->pad_; }
CA_DEV bool celt_packets_lost(const opusgpu_packet_frames *fr, int f) { return fr->pad_ == PKT_RUN_LOST && f == 0; }

// The lane stage's bookkeeping for a stream that pass f does not decode a coded frame of. Returns true where the lane has nothing
// more to do: the stream has no frame f (every later stage then leaves it alone: mid_valid == 0, mid_plc == OPUSGPU_PLC_NONE), its
// packet is lost, or frame f is a DTX frame; both of the latter are marked for the concealment stage. *rng is the stream's d_rng.
CA_DEV bool celt_packets_lane_skips(opusgpu_celt_dec_state *st, const opusgpu_packet_frames *fr, int f, u32 *rng)
{
    if (celt_packets_lost(fr, f)) {
        st->mid_plc = OPUSGPU_PLC_LOST;
        st->mid_LM = LM3;                                                          // (after a shorter packet: steps of last_short)
        st->mid_valid = 0;
        st->final_range = 0;
        *rng = 0;
        return true;
    }
    if (!celt_packets_has_frame(fr, f)) {
        st->mid_plc = OPUSGPU_PLC_NONE;
        st->mid_valid = 0;
        return true;
    }
    if (fr->size[f] > 1) {
        st->mid_plc = OPUSGPU_PLC_NONE;
        return false;
    }
    // DTX: the stream takes the TOC's bandwidth, channel count and frame size first (src/opus_decoder.c:683-686)
    const int toc = fr->toc & ~3, lm = celt_toc_LM(toc);
    CA_COUNT(lm == 0 ? "multi_dtx_lm0" : lm == 1 ? "multi_dtx_lm1" : lm == 2 ? "multi_dtx_lm2" : "multi_dtx_lm3", 1);
    celt_plc_dtx_toc(st, toc);
    st->mid_plc = OPUSGPU_PLC_LOST;
    st->mid_LM = lm;
    st->last_short = lm != LM3 ? lm + 1 : 0;
    st->mid_valid = 0;
    st->final_range = 0;
    if (f == fr->pad_ - 1) *rng = 0;                                               // src/opus_decoder.c:579-580
    return true;
}

// ... and a coded frame's result: the last frame's final range is the packet's. An error inside a frame (OPUSGPU_INTERNAL_ERROR: the
// range decoder past the frame's end, which no input is known to reach -- the parser bounds every frame) ends the packet there as
// the reference's loop does (:693-694): the frames before it stay decoded, the call answers the error. This is the one way a
// stream's answer changes after the decision.
CA_DEV bool celt_packets_last_frame(const opusgpu_packet_frames *fr, int f) { return f == fr->pad_ - 1; }
CA_DEV void celt_packets_lane_result(opusgpu_packet_frames *fr, int f, bool last, DecResult r, int *ret, u32 *rng)
{
    if (r.samples < 0) {
        *ret = r.samples;
        *rng = r.final_range;
        fr->pad_ = (uint8_t)(f + 1);
    } else if (last) {
        *rng = r.final_range;
    }
}

// The concealment stage of pass f for a stream the lane stage marked lost (one wavefront; one "lane" in the emulation). A lost
// packet: as celt_dec_plc_any_kernel. A DTX frame of 20 ms: the one step of celt_plc_wave, finished by the synthesis and post
// stages. A shorter one: one step of the TOC's size, PCM included, unless the stream has no history yet (zeros, left to the post stage).
template <class LP_, class S>
CA_DEVFN void celt_packets_conceal(LP_ &P, S &L, opusgpu_celt_dec_state *st, const opusgpu_packet_frames *fr, int f, i16 *row)
{
    if (uni(st->mid_plc) != OPUSGPU_PLC_LOST) return;
    if (uni((int)fr->pad_) == PKT_RUN_LOST) {
        if (uni(st->last_short) != 0 && uni(st->started)) celt_plc_short_steps(P, L, st, row);
        else celt_plc_wave(P, st);
        return;
    }
    const int lm = uni(st->mid_LM) & 3;
    if (lm == LM3 || !uni(st->started)) celt_plc_wave(P, st);
    else celt_plc_short_steps<true>(P, L, st, row + (size_t)f * ((FRAME / M8) << lm) * 2, lm, 1);
}

// how many sample pairs of zeros the post stage owes a stream without history: the whole concealed packet, or the DTX frame
CA_DEV int celt_packets_zeros(const opusgpu_packet_frames *fr) { return fr->pad_ == PKT_RUN_LOST ? (int)FRAME : (int)fr->frame_samples; }

#if defined(CA_HOST_EMU)
// One packet of one stream through the parser, the decision and every pass, stage by stage as the kernels run them, for the host
// emulation. pcm: the stream's row of frame_size sample pairs.
template <class D, class LP_, class S>
CA_DEV DecResult celt_decode_packet_emu(D &F, LP_ &P, S &L, opusgpu_celt_dec_state *st, opusgpu_packet_frames *fr, const u8 *data, int len,
                                        int packet_stride, i16 *pcm, int frame_size, int max_frames)
{
    DecResult res;
    const int count = opus_packet_parse_stream(data, len, packet_stride, fr);
    int ret = celt_packets_decide(fr, count, frame_size, max_frames);
    u32 rng = st->final_range;
    for (int f = 0; f < max_frames; f++) {
        if (!celt_packets_lane_skips(st, fr, f, &rng)) {
            CA_COUNT("multi_frame_decoded", 1);
            const bool last = celt_packets_last_frame(fr, f);
            const DecResult r = celt_decode_front_frame<false>(F, st, fr->toc & ~3, data + fr->offset[f], fr->size[f]);
            celt_packets_lane_result(fr, f, last, r, &ret, &rng);
        }
        i16 *out = pcm + (size_t)f * fr->frame_samples * 2;
        celt_packets_conceal(P, L, st, fr, f, pcm);
        celt_decode_synth_any(L, st);
        for (int c = 0; c < 2; c++) {
            if (st->mid_plc == OPUSGPU_PLC_ZEROS) {
                for (int j = 0; j < celt_packets_zeros(fr); j++) out[j * 2 + c] = 0;
            } else if (st->mid_plc == OPUSGPU_PLC_PITCH) {
                celt_plc_tail_channel(st, c);
                celt_deemphasis_channel(st, c, out);
            } else {
                celt_decode_post_channel_any(st, c, out);
            }
        }
    }
    res.samples = ret;
    res.final_range = rng;
    return res;
}
#endif

}  // namespace ca
