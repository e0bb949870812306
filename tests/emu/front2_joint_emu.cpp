// tests/emu/front2_joint_emu.cpp -- TEST INFRASTRUCTURE: host build (CA_HOST_EMU, one "lane") of the second front stage of
// the frame kernel -- MDCT, band energies, normalised bands -- in its two forms: both channels through every loop together
// (Front2Lds, what celt_front2_kernel runs) and one channel at a time through the single-channel routines (FrontLds).
// tests/test_front2_joint_cpu.py compares them. Not a product path.
#define CA_HOST_EMU 1
#include <stdlib.h>
#include <string.h>
extern "C" void emu_tap(const char *, const void *, int) {}
extern "C" void emu_count(const char *, long) {}
#include "../../concentus_amd/csrc/celt_enc.h"

using namespace ca;

// in_ws: [2][1080] time signal as front phase 1 leaves it. Out: coef [2][960] MDCT coefficients, bandE [42], bandLogE [42],
// X [2][960] normalised bands (bins 0..799 of a channel are written).
extern "C" void emu_front2_joint(const int32_t *in_ws, int shortBlocks, int32_t *coef, int32_t *bandE, int16_t *bandLogE, int16_t *X)
{
    Front2Lds *F = (Front2Lds *)aligned_alloc(64, (sizeof(Front2Lds) + 63) / 64 * 64);
    memset(F, 0xAB, sizeof(Front2Lds));
    F->in_g = const_cast<int32_t *>(in_ws);
    F->x_g = X;
    compute_mdcts_joint(*F, shortBlocks);
    memcpy(coef, F->s.xf, sizeof(F->s.xf));
    band_energies_joint(*F, F->bandLogE);
    normalise_bands_joint(*F);
    memcpy(bandE, F->bandE, sizeof(F->bandE));
    memcpy(bandLogE, F->bandLogE, sizeof(F->bandLogE));
    free(F);
}

extern "C" void emu_front2_single(const int32_t *in_ws, int shortBlocks, int32_t *coef, int32_t *bandE, int16_t *bandLogE, int16_t *X)
{
    FrontLds *F = (FrontLds *)aligned_alloc(64, (sizeof(FrontLds) + 63) / 64 * 64);
    memset(F, 0xAB, sizeof(FrontLds));
    memcpy(F->in, in_ws, sizeof(F->in));
    for (int c = 0; c < 2; c++) {
        compute_mdct_channel(*F, c, shortBlocks);
        band_energies_channel(*F, c, F->bandLogE);
    }
    memcpy(coef, F->xf, sizeof(F->xf));
    for (int c = 0; c < 2; c++) normalise_bands_channel(*F, c);      // X takes the place of the time signal
    memcpy(X, frame_X(*F), 2 * 960 * sizeof(int16_t));
    memcpy(bandE, F->bandE, sizeof(F->bandE));
    memcpy(bandLogE, F->bandLogE, sizeof(F->bandLogE));
    free(F);
}

// band energies alone, on given coefficients [2][960] (for values no transform produces, -2^31 among them)
extern "C" void emu_band_energies_joint(const int32_t *coef, int32_t *bandE, int16_t *bandLogE)
{
    Front2Lds *F = (Front2Lds *)aligned_alloc(64, (sizeof(Front2Lds) + 63) / 64 * 64);
    memset(F, 0xAB, sizeof(Front2Lds));
    memcpy(F->s.xf, coef, sizeof(F->s.xf));
    band_energies_joint(*F, F->bandLogE);
    memcpy(bandE, F->bandE, sizeof(F->bandE));
    memcpy(bandLogE, F->bandLogE, sizeof(F->bandLogE));
    free(F);
}

extern "C" void emu_band_energies_single(const int32_t *coef, int32_t *bandE, int16_t *bandLogE)
{
    FrontLds *F = (FrontLds *)aligned_alloc(64, (sizeof(FrontLds) + 63) / 64 * 64);
    memset(F, 0xAB, sizeof(FrontLds));
    memcpy(F->xf, coef, sizeof(F->xf));
    for (int c = 0; c < 2; c++) band_energies_channel(*F, c, F->bandLogE);
    memcpy(bandE, F->bandE, sizeof(F->bandE));
    memcpy(bandLogE, F->bandLogE, sizeof(F->bandLogE));
    free(F);
}

extern "C" int emu_front2_lds_bytes(void) { return (int)sizeof(Front2Lds); }
