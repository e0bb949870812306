// tests/emu/celt_dec_multi_emu.cpp -- TEST INFRASTRUCTURE: host build (CA_HOST_EMU, one "lane") of the packet parser and the frame loop
// as opusgpu_packet_parse_batch / opusgpu_decode_batch_packets run them (concentus_amd/csrc/opus_packet.h, celt_dec_packets.h):
// CELT-only packets of 1..48 frames, padding and DTX frames, so that they can be compared against the reference on a CPU.
// Not a product path: concentus_amd/ never loads this library.
#define CA_HOST_EMU 1
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>
extern "C" void emu_tap(const char *, const void *, int) {}
// branch counters (CA_COUNT in the decoder sources): name -> events
static std::map<std::string, long> g_counts;
extern "C" void emu_count(const char *name, long n) { g_counts[name] += n; }
extern "C" void emu_multi_counts_reset(void) { g_counts.clear(); }
extern "C" long emu_multi_count(const char *name)
{
    auto it = g_counts.find(name);
    return it == g_counts.end() ? 0 : it->second;
}
#include "../../concentus_amd/csrc/celt_dec_packets.h"

using namespace ca;

static void *emu_alloc(size_t n) { return aligned_alloc(64, (n + 127) & ~(size_t)63); }

static void dec_state_reset(opusgpu_celt_dec_state *st)
{
    memset(st, 0, sizeof(*st));
    for (int i = 0; i < 42; i++) st->oldLogE[i] = st->oldLogE2[i] = -28672;
}

// opusgpu_packet_parse_batch: one record per packet
extern "C" int emu_packet_parse(const unsigned char *packets, int stride, const int *len, int n, opusgpu_packet_frames *frames)
{
    for (int k = 0; k < n; k++) {
        opus_packet_parse_stream(packets + (size_t)k * stride, len[k], stride, frames + k);
        frames[k].pad_ = 0;
    }
    return 0;
}

// npackets packets, stream-major, a fresh decoder every packets_per_stream; packet k is decoded into pcm[k][frame_size[k]][2] of
// rows of max_frame_size sample pairs, of which the first ret[k] are written and the rest is left as the caller filled it
extern "C" int emu_celt_decode_packets(const unsigned char *packets, int stride, const int *len, const int *frame_size, int max_frames,
                                       int npackets, int packets_per_stream, int16_t *pcm, int max_frame_size, uint32_t *rng, int *ret,
                                       opusgpu_packet_frames *frames)
{
    DecWork *F = (DecWork *)emu_alloc(sizeof(DecWork));
    SynthLds *L = (SynthLds *)emu_alloc(sizeof(SynthLds));
    PlcLds *P = (PlcLds *)emu_alloc(sizeof(PlcLds));
    opusgpu_celt_dec_state *st = (opusgpu_celt_dec_state *)emu_alloc(sizeof(opusgpu_celt_dec_state));
    for (int k = 0; k < npackets; k++) {
        if (k % packets_per_stream == 0) dec_state_reset(st);
        memset(F, 0xAB, sizeof(DecWork));
        memset(L, 0xAB, sizeof(SynthLds));
        memset(P, 0xAB, sizeof(PlcLds));
        const DecResult r = celt_decode_packet_emu(*F, *P, *L, st, frames + k, packets + (size_t)k * stride, len[k], stride,
                                                   pcm + (size_t)k * max_frame_size * 2, frame_size[k], max_frames);
        ret[k] = r.samples;
        rng[k] = r.final_range;
    }
    free(F);
    free(L);
    free(P);
    free(st);
    return 0;
}
extern "C" int emu_multi_sizeof_frames(void) { return (int)sizeof(opusgpu_packet_frames); }
