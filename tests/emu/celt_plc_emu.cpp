// tests/emu/celt_plc_emu.cpp -- TEST INFRASTRUCTURE: host build (CA_HOST_EMU, one "lane") of the decoder sources with the packet
// loss concealment (concentus_amd/csrc/celt_plc.h), so that celt_decode_lost can be compared against the reference on a CPU.
// Not a product path: concentus_amd/ never loads this library.
#define CA_HOST_EMU 1
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>
extern "C" void emu_tap(const char *, const void *, int) {}
// branch counters of the concealment (CA_COUNT in celt_plc.h / celt_dec.h): name -> events
static std::map<std::string, long> g_counts;
extern "C" void emu_count(const char *name, long n) { g_counts[name] += n; }
extern "C" void emu_plc_counts_reset(void) { g_counts.clear(); }
extern "C" long emu_plc_count(const char *name)
{
    auto it = g_counts.find(name);
    return it == g_counts.end() ? 0 : it->second;
}
// per-frame view of the counters: after every frame of emu_celt_decode_frames_plc the running totals of the named counters go
// to out[frame * n + i], so that a test can tell which frame reached a branch (names == NULL switches it off)
static const char *const *g_trace_names = nullptr;
static int g_trace_n = 0;
static long *g_trace_out = nullptr;
extern "C" void emu_plc_trace_counts(const char *const *names, int n, long *out) { g_trace_names = names; g_trace_n = names ? n : 0; g_trace_out = out; }
#include "../../concentus_amd/csrc/celt_plc.h"

using namespace ca;

// (aligned_alloc wants a size that is a multiple of the alignment)
static void *emu_alloc(size_t n) { return aligned_alloc(64, (n + 127) & ~(size_t)63); }

static void dec_state_reset(opusgpu_celt_dec_state *st)
{
    memset(st, 0, sizeof(*st));
    for (int i = 0; i < 42; i++) st->oldLogE[i] = st->oldLogE2[i] = -28672;
}

// emu_celt_decode_frames (celt_emu.cpp) with concealment: a packet of length 0 (lost) or the one-byte packet 0xFC (DTX) is concealed
extern "C" int emu_celt_decode_frames_plc(const unsigned char *packets, int stride, const int *len, int nframes,
                                          int frames_per_stream, int16_t *pcm, uint32_t *rng, int *ret)
{
    DecWork *F = (DecWork *)emu_alloc(sizeof(DecWork));
    SynthLds *L = (SynthLds *)emu_alloc(sizeof(SynthLds));
    PlcLds *P = (PlcLds *)emu_alloc(sizeof(PlcLds));
    opusgpu_celt_dec_state *st = (opusgpu_celt_dec_state *)emu_alloc(sizeof(opusgpu_celt_dec_state));
    for (int n = 0; n < nframes; n++) {
        if (n % frames_per_stream == 0) dec_state_reset(st);
        memset(F, 0xAB, sizeof(DecWork));
        memset(L, 0xAB, sizeof(SynthLds));
        memset(P, 0xAB, sizeof(PlcLds));
        const unsigned char *data = packets + (size_t)n * stride;
        int16_t *out = pcm + (size_t)n * 960 * 2;
        DecResult r;
        if (celt_plc_conceals(data, len[n])) {
            r = celt_decode_lost_frame(*P, *L, st, out);
        } else {
            st->mid_plc = OPUSGPU_PLC_NONE;
            r = celt_decode_frame(*F, *L, st, data, len[n], out);
        }
        ret[n] = r.samples;
        rng[n] = r.final_range;
        for (int i = 0; i < g_trace_n; i++) g_trace_out[(size_t)n * g_trace_n + i] = emu_plc_count(g_trace_names[i]);
    }
    free(F);
    free(L);
    free(P);
    free(st);
    return 0;
}
extern "C" int emu_plc_sizeof_dec_state(void) { return (int)sizeof(opusgpu_celt_dec_state); }
extern "C" int emu_plc_sizeof_lds(void) { return (int)sizeof(PlcLds); }
