// tests/emu/packet_parse_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program around the packet parser
// (concentus_amd/csrc/opus_packet.h, host build) for the sanitizers: tests/test_decode_multi_emu_cpu.py compiles it with
// -fsanitize=address,undefined and runs it. Every packet lies in a heap block of exactly its length, so a read at or behind
// d_len[i] is a heap-buffer-overflow; the frame tables are checked against the packet's length as well.
//
//   packet_parse_main [corpus]     corpus: records of <uint32 length, little endian><bytes>, fed after the built-in packets
//
// Built in: the malformed layouts of tests/golden/make_multi_golden.py, every one-, two- and three-byte prefix of interest, and
// random bytes under every TOC. Exit status 0 and a line of counts, or 1 with the offending packet.
#define CA_HOST_EMU 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
extern "C" void emu_tap(const char *, const void *, int) {}
extern "C" void emu_count(const char *, long) {}
#include "../../concentus_amd/csrc/opus_packet.h"

static long g_accepted, g_rejected;

static int feed(const std::vector<uint8_t> &p)
{
    const int len = (int)p.size();
    uint8_t *buf = (uint8_t *)malloc(len ? len : 1);             // exactly len bytes (malloc(0) may return NULL)
    if (len) memcpy(buf, p.data(), len);
    opusgpu_packet_frames *fr = (opusgpu_packet_frames *)malloc(sizeof(opusgpu_packet_frames));
    memset(fr, 0xEE, sizeof(*fr));
    const int r = ca::opus_packet_parse_stream(buf, len, len, fr);
    int bad = 0;
    if (r != fr->ret) bad = 1;
    if (r > 0) {
        g_accepted++;
        if (r > 48 || r * fr->frame_samples > 5760) bad = 2;
        int end = 1;
        for (int i = 0; i < r && !bad; i++) {
            if (fr->size[i] < 0 || fr->size[i] > 1275 || fr->offset[i] < end || fr->offset[i] + fr->size[i] > len) bad = 3;
            end = fr->offset[i] + fr->size[i];
        }
        for (int i = r; i < 48 && !bad; i++) if (fr->size[i] || fr->offset[i]) bad = 4;
    } else {
        g_rejected++;
        if (r != 0 && r != OPUSGPU_INVALID_PACKET && r != OPUSGPU_BAD_ARG) bad = 5;
        for (int i = 0; i < 48 && !bad; i++) if (fr->size[i] || fr->offset[i]) bad = 6;
    }
    if (bad) {
        fprintf(stderr, "packet_parse_main: check %d failed, ret %d, len %d:", bad, r, len);
        for (int i = 0; i < len && i < 32; i++) fprintf(stderr, " %02x", buf[i]);
        fprintf(stderr, "\n");
    }
    free(fr);
    free(buf);
    return bad;
}

static uint32_t g_seed = 12345;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

int main(int argc, char **argv)
{
    int bad = 0;
    std::vector<uint8_t> p;
    // the malformed layouts: odd code 1; code 2 with size[0] past the end / its second length byte cut off; code 3 of one byte, with
    // count 0, with more than 120 ms, with padding past the end, CBR not divisible, VBR overrunning; a frame of 1276 bytes
    const std::vector<std::vector<uint8_t>> heads = {
        {0xFD, 1, 2, 3}, {0xFE, 200, 1, 2, 3}, {0xFE, 252}, {0xFE, 255}, {0xFF}, {0xFF, 0x80, 1, 2}, {0xFF, 0x87, 0, 0, 0, 0, 0, 0, 9},
        {0xF7, 0x42, 255, 255, 10, 1, 2, 3, 4}, {0xF7, 0x42, 255}, {0xF7, 0x42}, {0xF7, 0x43, 3}, {0xF7, 3, 1, 2, 3, 4}, {0xF7, 0x83, 20, 200, 1, 2, 3},
        {0xF7, 0x83, 252}, {0xF7, 0xB0}, {0x03, 0x83, 0, 0, 0}, {0x7B, 0x82, 1, 9}, {0xE3, 0xB0}, {0xE3, 0xF0, 0}, {}};
    for (const auto &h : heads) bad |= feed(h);
    p.assign(1277, 0x5A);
    p[0] = 0xFC;
    bad |= feed(p);
    p[0] = 0xFE;
    p[1] = 0;
    bad |= feed(p);
    p.resize(2 + 2 * 1276);
    p[0] = 0xFD;
    bad |= feed(p);
    // packets whose frame offsets would not fit 16 bits: 48 CBR frames of 700 bytes (33 602 bytes) and the same behind 40 000 bytes
    // of chained padding length are refused unread; 48 x 682 (32 738 bytes, the last offset 32 056) is parsed
    for (int size : {700, 682}) {
        p.assign(2 + 48 * size, 0x11);
        p[0] = 0xE7;
        p[1] = 48;
        const int r0 = g_accepted;
        bad |= feed(p);
        if ((g_accepted - r0 == 1) != (size == 682)) { fprintf(stderr, "packet_parse_main: 48 x %d bytes: wrong answer\n", size); bad |= 1; }
    }
    p.assign(40000, 0xFF);
    p[0] = 0xE7;
    p[1] = 0x40 | 48;
    bad |= feed(p);
    // every TOC with every second byte, alone and with a third
    for (int toc = 0; toc < 256; toc++) {
        bad |= feed({(uint8_t)toc});
        for (int b = 0; b < 256; b++) {
            bad |= feed({(uint8_t)toc, (uint8_t)b});
            bad |= feed({(uint8_t)toc, (uint8_t)b, (uint8_t)rnd()});
        }
    }
    // random bytes, and random bytes with small numbers where the lengths live (so that deep paths are reached)
    for (int k = 0; k < 60000; k++) {
        const int len = 1 + rnd() % (k % 7 == 0 ? 1500 : 80);
        p.resize(len);
        for (int i = 0; i < len; i++) p[i] = (uint8_t)rnd();
        if (k & 1) for (int i = 1; i < len && i < 50; i++) if (rnd() % 3) p[i] = (uint8_t)(rnd() % 6);
        if ((k & 3) == 3 && len > 1) p[1] = (uint8_t)((p[1] & 0xC0) | (1 + rnd() % 6));
        bad |= feed(p);
    }
    if (argc > 1) {
        FILE *f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        uint8_t h[4];
        while (fread(h, 1, 4, f) == 4) {
            const uint32_t len = h[0] | h[1] << 8 | h[2] << 16 | (uint32_t)h[3] << 24;
            p.resize(len);
            if (len && fread(p.data(), 1, len, f) != len) { fprintf(stderr, "short corpus\n"); return 2; }
            bad |= feed(p);
        }
        fclose(f);
    }
    printf("packet_parse_main: %ld accepted, %ld rejected, %s\n", g_accepted, g_rejected, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
