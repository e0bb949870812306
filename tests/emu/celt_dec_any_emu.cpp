// tests/emu/celt_dec_any_emu.cpp -- TEST INFRASTRUCTURE: host build (CA_HOST_EMU, one "lane") of the decoder sources as
// opusgpu_decode_batch_any runs them (concentus_amd/csrc/celt_dec.h with ANY, celt_plc.h): CELT-only code-0 packets of 2.5, 5, 10
// and 20 ms, so that the short frames can be compared against the reference on a CPU.
// Not a product path: concentus_amd/ never loads this library.
#define CA_HOST_EMU 1
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>
extern "C" void emu_tap(const char *, const void *, int) {}
// branch counters (CA_COUNT in celt_dec.h / celt_plc.h): name -> events
static std::map<std::string, long> g_counts;
extern "C" void emu_count(const char *name, long n) { g_counts[name] += n; }
extern "C" void emu_any_counts_reset(void) { g_counts.clear(); }
extern "C" long emu_any_count(const char *name)
{
    auto it = g_counts.find(name);
    return it == g_counts.end() ? 0 : it->second;
}
#include "../../concentus_amd/csrc/celt_plc.h"

using namespace ca;

// (aligned_alloc wants a size that is a multiple of the alignment)
static void *emu_alloc(size_t n) { return aligned_alloc(64, (n + 127) & ~(size_t)63); }

static void dec_state_reset(opusgpu_celt_dec_state *st)
{
    memset(st, 0, sizeof(*st));
    for (int i = 0; i < 42; i++) st->oldLogE[i] = st->oldLogE2[i] = -28672;
}

// emu_celt_decode_frames_plc (celt_plc_emu.cpp) with every frame size: pcm stays [nframes][960][2], of which frame n's first
// ret[n] sample pairs are written and the rest is left as the caller filled it
extern "C" int emu_celt_decode_frames_any(const unsigned char *packets, int stride, const int *len, int nframes,
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
        if (len[n] > stride) {
            r.samples = OPUSGPU_BAD_ARG;
            r.final_range = st->final_range;
        } else if (celt_plc_conceals(data, len[n])) {
            r = celt_decode_lost_frame_any(*P, *L, st, out);
        } else {
            st->mid_plc = OPUSGPU_PLC_NONE;
            r = celt_decode_frame_any(*F, *L, st, data, len[n], out);
        }
        ret[n] = r.samples;
        rng[n] = r.final_range;
    }
    free(F);
    free(L);
    free(P);
    free(st);
    return 0;
}
extern "C" int emu_any_sizeof_dec_state(void) { return (int)sizeof(opusgpu_celt_dec_state); }
