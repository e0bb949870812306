// tests/emu/decode_corpus_main.cpp -- TEST INFRASTRUCTURE: a stand-alone program around the host emulation of the decoder with
// concealment (celt_plc_emu.cpp), to be built with -fsanitize=address,undefined and run on corrupt packets
// (tests/test_decode_corrupt_emu_cpu.py). Reads a flat binary: int32 n, fps, stride; int32 len[n]; n * stride packet bytes.
// Every packet is copied into a heap block of exactly its own length, so that a read past the packet's end is a report.
#include "celt_plc_emu.cpp"
#include <stdio.h>
#include <vector>

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[3];
    if (fread(hdr, 4, 3, f) != 3 || hdr[0] < 0 || hdr[1] <= 0 || hdr[2] <= 0) { fprintf(stderr, "bad header\n"); return 2; }
    const int n = hdr[0], fps = hdr[1], stride = hdr[2];
    std::vector<int32_t> len(n);
    std::vector<unsigned char> row(stride);
    if (n && fread(len.data(), 4, n, f) != (size_t)n) { fprintf(stderr, "short lengths\n"); return 2; }
    DecWork *F = (DecWork *)emu_alloc(sizeof(DecWork));
    SynthLds *L = (SynthLds *)emu_alloc(sizeof(SynthLds));
    PlcLds *P = (PlcLds *)emu_alloc(sizeof(PlcLds));
    opusgpu_celt_dec_state *st = (opusgpu_celt_dec_state *)emu_alloc(sizeof(opusgpu_celt_dec_state));
    std::vector<int16_t> pcm(960 * 2);
    long decoded = 0, concealed = 0, rejected = 0;
    for (int k = 0; k < n; k++) {
        if (fread(row.data(), 1, stride, f) != (size_t)stride) { fprintf(stderr, "short packets\n"); return 2; }
        if (k % fps == 0) dec_state_reset(st);
        const int ln = len[k] < 0 ? 0 : len[k] > stride ? stride : len[k];
        unsigned char *data = (unsigned char *)malloc(ln ? ln : 1);
        memcpy(data, row.data(), ln);
        DecResult r;
        if (celt_plc_conceals(data, ln)) {
            r = celt_decode_lost_frame(*P, *L, st, pcm.data());
            concealed++;
        } else {
            st->mid_plc = OPUSGPU_PLC_NONE;
            r = celt_decode_frame(*F, *L, st, data, ln, pcm.data());
            if (r.samples < 0) rejected++; else decoded++;
        }
        free(data);
    }
    fclose(f);
    free(F); free(L); free(P); free(st);
    printf("%ld decoded, %ld concealed, %ld rejected\n", decoded, concealed, rejected);
    return 0;
}
