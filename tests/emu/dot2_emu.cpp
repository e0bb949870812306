// tests/emu/dot2_emu.cpp -- TEST INFRASTRUCTURE: the packed-pair primitives of csrc/fixmath.h (dot2_i16, pair_at, pair_next)
// in their CA_HOST_EMU form, exported element-wise over arrays for tests/test_dot2_cpu.py.
#define CA_HOST_EMU 1
#include "../../concentus_amd/csrc/fixmath.h"

extern "C" void emu_tap(const char *, const void *, int) {}
extern "C" void emu_count(const char *, long) {}

extern "C" void emu_dot2_i16(const uint32_t *a, const uint32_t *b, const int32_t *c, int32_t *out, int n)
{
    for (int i = 0; i < n; i++) out[i] = ca::dot2_i16(a[i], b[i], c[i]);
}

extern "C" void emu_pair_at(const uint32_t *w0, const uint32_t *w1, const int32_t *odd, uint32_t *out, int n)
{
    for (int i = 0; i < n; i++) out[i] = ca::pair_at(w0[i], w1[i], odd[i]);
}

extern "C" void emu_pair_next(const uint32_t *w0, const uint32_t *w1, uint32_t *out, int n)
{
    for (int i = 0; i < n; i++) out[i] = ca::pair_next(w0[i], w1[i]);
}
