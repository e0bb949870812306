/* opus_compat.c -- the libopus entry points under their OWN names, for callers that cannot be edited.
 *
 * libopusgpu.so exports the single-stream verbs as opusgpu_encoder_create / _ctl / opusgpu_encode / ... so that it can
 * live in one process with a real libopus (the parity tests load both). A caller written against <opus.h> -- the
 * reference's own src/opus_demo.c, or the P/Invoke harness CSharp/ParityTest/TestDriver.cs:22-41 which binds
 * "opus_encoder_create", "opus_encode", ... by name -- links against THIS library instead: plain C, no HIP types, every
 * function a one-line forward. Built by concentus_amd/csrc/Makefile with gcc into concentus_amd/compat/libopus.so
 * (DT_NEEDED libopusgpu.so, rpath $ORIGIN/..).
 *
 * Signatures: opus-fix/include/opus.h:164-263 (encoder), :438-520 (decoder), :540-590 (packet helpers),
 * include/opus_defines.h:46-60 (error codes, identical to OPUSGPU_*), :770-784 (opus_strerror, opus_get_version_string).
 * Supported region: what libopusgpu.so implements (48 kHz stereo, 20 ms, OPUS_APPLICATION_RESTRICTED_LOWDELAY);
 * everything else returns OPUS_UNIMPLEMENTED exactly where libopus would have returned OPUS_OK. */
#define _DEFAULT_SOURCE 1            /* initstate / setstate */
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../../include/opusgpu.h"

typedef struct OpusGpuEncoder OpusEncoder;
typedef struct OpusGpuDecoder OpusDecoder;

#define OPUS_RESET_STATE_REQUEST 4028

/* libopus never touches the C library's random generator; the HSA runtime under libopusgpu.so does (it imports srand and rand,
 * and a process that has loaded it no longer draws the sequence it would have drawn). A caller may depend on that sequence:
 * opus_demo -loss draws its loss pattern from rand(). So every entry point that can reach the runtime runs on a generator state
 * of this library's own and puts the caller's back, position included, before it returns (rand() and random() share the state
 * that initstate / setstate exchange). Like rand() itself this is not meant for concurrent callers. */
static char g_own_rand_state[128];
#define CALLER_RAND_KEPT(call) do { char *caller_ = initstate(1u, g_own_rand_state, sizeof g_own_rand_state); call; \
                                    if (caller_) setstate(caller_); } while (0)

OpusEncoder *opus_encoder_create(int32_t Fs, int channels, int application, int *error)
{
    OpusEncoder *st;
    CALLER_RAND_KEPT(st = opusgpu_encoder_create(Fs, channels, application, error));
    return st;
}

/* opus_encoder_ctl is variadic. Every request of include/opus_defines.h:130-167 carries exactly one argument: an
 * opus_int32 for the setters (even request numbers), a pointer for the getters (odd); OPUS_RESET_STATE carries none. */
int opus_encoder_ctl(OpusEncoder *st, int request, ...)
{
    va_list ap;
    int ret;
    va_start(ap, request);
    if (request == OPUS_RESET_STATE_REQUEST) CALLER_RAND_KEPT(ret = opusgpu_encoder_ctl(st, request));
    else if (request & 1) CALLER_RAND_KEPT(ret = opusgpu_encoder_ctl(st, request, va_arg(ap, void *)));
    else CALLER_RAND_KEPT(ret = opusgpu_encoder_ctl(st, request, va_arg(ap, int32_t)));
    va_end(ap);
    return ret;
}

int32_t opus_encode(OpusEncoder *st, const int16_t *pcm, int frame_size, unsigned char *data, int32_t max_data_bytes)
{
    int32_t ret;
    CALLER_RAND_KEPT(ret = opusgpu_encode(st, pcm, frame_size, data, max_data_bytes));
    return ret;
}

void opus_encoder_destroy(OpusEncoder *st) { CALLER_RAND_KEPT(opusgpu_encoder_destroy(st)); }

OpusDecoder *opus_decoder_create(int32_t Fs, int channels, int *error)
{
    OpusDecoder *st;
    CALLER_RAND_KEPT(st = opusgpu_decoder_create(Fs, channels, error));
    return st;
}

int opus_decoder_ctl(OpusDecoder *st, int request, ...)
{
    va_list ap;
    int ret;
    va_start(ap, request);
    if (request == OPUS_RESET_STATE_REQUEST) CALLER_RAND_KEPT(ret = opusgpu_decoder_ctl(st, request));
    else if (request & 1) CALLER_RAND_KEPT(ret = opusgpu_decoder_ctl(st, request, va_arg(ap, void *)));
    else CALLER_RAND_KEPT(ret = opusgpu_decoder_ctl(st, request, va_arg(ap, int32_t)));
    va_end(ap);
    return ret;
}

int opus_decode(OpusDecoder *st, const unsigned char *data, int32_t len, int16_t *pcm, int frame_size, int decode_fec)
{
    /* a lost packet is concealed; so is a request for FEC, which a CELT-only stream cannot carry: libopus runs the PLC
     * instead (src/opus_decoder.c:608-649) */
    int ret;
    if (decode_fec < 0 || decode_fec > 1 || len < 0) return OPUSGPU_BAD_ARG;
    if (data == NULL || len == 0 || decode_fec) CALLER_RAND_KEPT(ret = opusgpu_decode_lost(st, pcm, frame_size));
    else CALLER_RAND_KEPT(ret = opusgpu_decode(st, data, len, pcm, frame_size, decode_fec));
    return ret;
}

void opus_decoder_destroy(OpusDecoder *st) { CALLER_RAND_KEPT(opusgpu_decoder_destroy(st)); }

const char *opus_strerror(int error) { return opusgpu_strerror(error); }
const char *opus_get_version_string(void)
{
    const char *v;
    CALLER_RAND_KEPT(v = opusgpu_get_version_string());
    return v;
}

/* ---- packet helpers: pure functions of the TOC byte (RFC 6716 section 3.1; src/opus.c:169-188,
 * src/opus_decoder.c:944-975, :916-942) ---- */
int opus_packet_get_samples_per_frame(const unsigned char *data, int32_t Fs)
{
    const int toc = data[0];
    if (toc & 0x80) return (int)((Fs << ((toc >> 3) & 3)) / 400);          /* CELT-only: 2.5 / 5 / 10 / 20 ms */
    if ((toc & 0x60) == 0x60) return (int)((toc & 0x08) ? Fs / 50 : Fs / 100); /* hybrid: 10 / 20 ms */
    {
        const int sz = (toc >> 3) & 3;                                         /* SILK-only: 10 / 20 / 40 / 60 ms */
        return (int)(sz == 3 ? Fs * 60 / 1000 : (Fs << sz) / 100);
    }
}

int opus_packet_get_nb_frames(const unsigned char packet[], int32_t len)
{
    int count;
    if (len < 1) return OPUSGPU_BAD_ARG;
    count = packet[0] & 3;
    if (count == 0) return 1;
    if (count != 3) return 2;
    if (len < 2) return OPUSGPU_INVALID_PACKET;
    return packet[1] & 0x3F;
}

int opus_packet_get_nb_samples(const unsigned char packet[], int32_t len, int32_t Fs)
{
    const int count = opus_packet_get_nb_frames(packet, len);
    int samples;
    if (count < 0) return count;
    samples = count * opus_packet_get_samples_per_frame(packet, Fs);
    return samples * 25 > Fs * 3 ? OPUSGPU_INVALID_PACKET : samples;           /* at most 120 ms */
}

int opus_packet_get_nb_channels(const unsigned char *data) { return (data[0] & 0x4) ? 2 : 1; }

int opus_packet_get_bandwidth(const unsigned char *data)
{
    /* OPUS_BANDWIDTH_NARROWBAND 1101 .. OPUS_BANDWIDTH_FULLBAND 1105 (include/opus_defines.h:194-198) */
    int bw;
    if (data[0] & 0x80) {
        bw = 1102 + ((data[0] >> 5) & 3);
        if (bw == 1102) bw = 1101;
    } else if ((data[0] & 0x60) == 0x60) {
        bw = (data[0] & 0x10) ? 1105 : 1104;
    } else {
        bw = 1101 + ((data[0] >> 5) & 3);
    }
    return bw;
}
