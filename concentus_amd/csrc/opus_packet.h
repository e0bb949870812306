// opus_packet.h -- the Opus packet layer of the batched decoder: opus_packet_parse_impl (opus-fix/src/opus.c:190-343, not
// self-delimited) with parse_size (:148-167) and opus_packet_get_samples_per_frame (:169-188) at 48 kHz, one packet into one
// opusgpu_packet_frames record (include/opusgpu.h). The same text runs one lane per stream on the device (opus_packet_kernel.hip)
// and as plain C++ in the host emulation (CA_HOST_EMU; tests/emu).
//
// The frame lengths and the padding chain are whatever the sender wrote. Every byte is read at an index below `len`, and only after
// the reference's own test of the remaining length at that place has passed: the remaining length `rem` below is the reference's
// `len`, the index `pos` its `data - data0`.
#pragma once
#include "wave.h"
#include "../../include/opusgpu.h"

namespace ca {

enum { OPUS_MAX_FRAMES = 48, OPUS_MAX_FRAME_BYTES = 1275, OPUS_MAX_PACKET_SAMPLES = 5760 };
// The record keeps a frame's offset in 16 bits, so a packet may have at most 32767 bytes: every offset is below the packet's length.
// (48 frames of 1275 bytes behind an arbitrarily long padding chain are legal Opus and do not fit; a libopus sender, capped at
// 510 kb/s per stream, puts under 8 KB into 120 ms.) A longer packet is refused unread with OPUSGPU_BAD_ARG, like a
// length past the row.
enum { OPUS_MAX_PARSE_BYTES = 32767 };

// opus_packet_get_samples_per_frame(data, 48000): CELT-only 120 << fs; hybrid 480 / 960; SILK-only 480, 960, 1920, 2880
CA_DEV int opus_toc_frame_samples(int toc)
{
    if (toc & 0x80) return 120 << ((toc >> 3) & 3);
    if ((toc & 0x60) == 0x60) return (toc & 0x08) ? 960 : 480;
    const int a = (toc >> 3) & 3;
    return a == 3 ? 2880 : 480 << a;
}

// parse_size: the one- or two-byte frame length at data[pos], `rem` bytes left. Returns the bytes used and the length, or -1 / -1.
CA_DEV int opus_parse_size(const uint8_t *data, int pos, int rem, int *size)
{
    if (rem < 1) { *size = -1; return -1; }
    const int b0 = data[pos];
    if (b0 < 252) { *size = b0; return 1; }
    if (rem < 2) { *size = -1; return -1; }
    CA_COUNT("pkt_size_two_bytes", 1);
    *size = 4 * data[pos + 1] + b0;
    return 2;
}

// The body of opus_packet_parse_impl behind the TOC byte: the frame count with fr->size[0 .. count) and fr->offset[0 .. count)
// written, or OPUSGPU_INVALID_PACKET (fr->size may then hold the lengths read so far).
CA_DEV int opus_packet_parse_body(const uint8_t *data, int len, int toc, int framesize, opusgpu_packet_frames *fr)
{
    int pos = 1, rem = len - 1;
    int last_size = rem, count, bytes, sz;
    bool cbr = false;
    switch (toc & 3) {
    case 0:
        CA_COUNT("pkt_code0", 1);
        count = 1;
        break;
    case 1:                                                                        // two CBR frames
        CA_COUNT("pkt_code1", 1);
        count = 2;
        cbr = true;
        if (rem & 1) return OPUSGPU_INVALID_PACKET;
        last_size = rem / 2;
        break;
    case 2:                                                                        // two VBR frames
        CA_COUNT("pkt_code2", 1);
        count = 2;
        bytes = opus_parse_size(data, pos, rem, &sz);
        rem -= bytes;
        if (sz < 0 || sz > rem) return OPUSGPU_INVALID_PACKET;
        pos += bytes;
        fr->size[0] = (int16_t)sz;
        last_size = rem - sz;
        break;
    default: {                                                                     // 1..48 frames, CBR or VBR, with or without padding
        CA_COUNT("pkt_code3", 1);
        if (rem < 1) return OPUSGPU_INVALID_PACKET;
        const int ch = data[pos++];
        count = ch & 0x3F;
        if (count <= 0 || framesize * count > OPUS_MAX_PACKET_SAMPLES) return OPUSGPU_INVALID_PACKET;
        rem--;
        if (ch & 0x40) {                                                           // padding: 255 stands for 254 bytes and another length byte
            CA_COUNT("pkt_padding", 1);
            int p;
            do {
                if (rem <= 0) return OPUSGPU_INVALID_PACKET;
                p = data[pos++];
                rem--;
                if (p == 255) CA_COUNT("pkt_padding_chained", 1);
                rem -= p == 255 ? 254 : p;
            } while (p == 255);
        }
        if (rem < 0) return OPUSGPU_INVALID_PACKET;
        cbr = !(ch & 0x80);
        if (!cbr) {
            CA_COUNT("pkt_code3_vbr", 1);
            last_size = rem;
            for (int i = 0; i < count - 1; i++) {
                bytes = opus_parse_size(data, pos, rem, &sz);
                rem -= bytes;
                if (sz < 0 || sz > rem) return OPUSGPU_INVALID_PACKET;
                pos += bytes;
                fr->size[i] = (int16_t)sz;
                last_size -= bytes + sz;
            }
            if (last_size < 0) return OPUSGPU_INVALID_PACKET;
        } else {
            CA_COUNT("pkt_code3_cbr", 1);
            last_size = rem / count;
            if (last_size * count != rem) return OPUSGPU_INVALID_PACKET;
        }
        break;
    }
    }
    // the last frame's length (every frame's, CBR) is not coded, so it alone can exceed 1275
    if (last_size > OPUS_MAX_FRAME_BYTES) return OPUSGPU_INVALID_PACKET;
    if (cbr) for (int i = 0; i < count - 1; i++) fr->size[i] = (int16_t)last_size;
    fr->size[count - 1] = (int16_t)last_size;
    for (int i = 0; i < count; i++) {
        fr->offset[i] = (int16_t)pos;
        pos += fr->size[i];
    }
    return count;
}

// opus_packet_parse(data, len, &toc, frames, size, NULL) for len >= 1: the frame count 1..48 with fr->offset / fr->size filled for
// that many frames (the rest zero), or OPUSGPU_INVALID_PACKET with both tables zero. fr->toc and fr->frame_samples are the TOC's
// in either case; fr->ret is the value returned. fr->pad_ is left alone.
CA_DEV int opus_packet_parse_frames(const uint8_t *data, int len, opusgpu_packet_frames *fr)
{
    const int toc = data[0];
    const int framesize = opus_toc_frame_samples(toc);
    fr->toc = (uint8_t)toc;
    fr->frame_samples = (int16_t)framesize;
    for (int i = 0; i < OPUS_MAX_FRAMES; i++) { fr->offset[i] = 0; fr->size[i] = 0; }
    const int r = opus_packet_parse_body(data, len, toc, framesize, fr);
    if (r < 0) for (int i = 0; i < OPUS_MAX_FRAMES; i++) fr->size[i] = 0;
    fr->ret = r;
    return r;
}

// One stream of opusgpu_packet_parse_batch: the packet's row, its length as the caller gave it, the row's size
CA_DEV int opus_packet_parse_stream(const uint8_t *row, int len, int packet_stride, opusgpu_packet_frames *fr)
{
    if (len <= 0 || len > packet_stride || len > OPUS_MAX_PARSE_BYTES) {
        // nothing may be read: a lost packet (0), or a length that is negative, runs into the next stream's row, or is more than
        // the record's 16-bit offsets can address
        fr->toc = 0;
        fr->frame_samples = 0;
        for (int i = 0; i < OPUS_MAX_FRAMES; i++) { fr->offset[i] = 0; fr->size[i] = 0; }
        fr->ret = len == 0 ? 0 : OPUSGPU_BAD_ARG;
        return fr->ret;
    }
    return opus_packet_parse_frames(row, len, fr);
}

}  // namespace ca
