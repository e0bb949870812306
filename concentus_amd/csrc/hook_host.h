// hook_host.h -- host plumbing of the per-call hooks (include/opusgpu_hooks.h and the older ones of opusgpu.h / opusgpu_silk.h).
// Every hook does the same six steps -- check the arguments, pack a record, allocate device memory, copy in, launch one batch
// entry on one record, copy out / map the status / set the last error / free -- and this header holds the one definition of
// each piece: field access into the reference's structs, the mirrors of the reference layouts the hooks look into, the device
// buffer, the heap record, the one-record runner and the range coder's marshalling -- and, at the end, the one record that two
// hook units share. Only the hook translation units include it; what all units share stays in opusgpu_internal.h.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include "rangecoder.h"
#include "opusgpu_internal.h"

// the calling thread's last error (opusgpu_get_last_error): every exit of a hook goes through here
static inline int fail(int rc) { opusgpu_set_last_error(rc); return rc; }

// ---- unaligned field access at a byte offset (the OPUSGPU_REF_OFF_* of include/opusgpu_hooks.h) -----------------------------
static inline int rd_int(const void *base, int off) { int v; memcpy(&v, (const char *)base + off, sizeof(v)); return v; }
static inline void wr_int(void *base, int off, int v) { memcpy((char *)base + off, &v, sizeof(v)); }
static inline int16_t rd_i16(const void *base, int off) { int16_t v; memcpy(&v, (const char *)base + off, sizeof(v)); return v; }
static inline void wr_i16(void *base, int off, int16_t v) { memcpy((char *)base + off, &v, sizeof(v)); }
static inline int rd_i8(const void *base, int off) { return (int)*((const int8_t *)base + off); }

// ---- mirrors of the reference's layouts, x86-64 (a mistake here corrupts a caller's state without any error) ------------------
// the tree's ec_ctx (celt/entcode.h:63-94, with the trailing EC_DIFF of this tree)
struct ref_ec_ctx {
    unsigned char *buf;
    uint32_t storage, end_offs, end_window;
    int nend_bits, nbits_total;
    uint32_t offs, rng, val, ext;
    int rem, error, EC_DIFF;
};
// head of kiss_fft_state (celt/kiss_fft.h:76-87)
struct ref_kiss_fft_state_head { int nfft; int16_t scale; int scale_shift; int shift; };
// head of mdct_lookup (celt/mdct.h:49-54)
struct ref_mdct_lookup_head { int n; int maxshift; };
// head of CELTMode (celt/modes.h:52-60)
struct ref_celt_mode_head { int32_t Fs; int overlap; int nbEBands; int effEBands; };

// which of the four kiss_fft_state of the static 48 kHz mode `cfg` is (nfft 480 >> k, scale 17476, scale_shift 8 - k): k, or -1.
// The head is validated, the tables behind it are not read.
static inline int kiss_fft_shift(const void *cfg)
{
    const ref_kiss_fft_state_head *h = (const ref_kiss_fft_state_head *)cfg;
    for (int k = 0; h && k < 4; k++)
        if (h->nfft == (480 >> k) && h->scale == 17476 && h->scale_shift == 8 - k) return k;
    return -1;
}

// ---- device memory of one call ------------------------------------------------------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    explicit DevBuf(size_t bytes) { if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) p = nullptr; }
    ~DevBuf() { if (p) (void)hipFree(p); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
};
template <class... B> static inline int allocated(const B &...b) { return (... && (b.p != nullptr)) ? OPUSGPU_OK : OPUSGPU_ALLOC_FAIL; }
static inline int h2d(void *d, const void *h, size_t n) { return hipMemcpy(d, h, n, hipMemcpyHostToDevice) == hipSuccess ? OPUSGPU_OK : OPUSGPU_INTERNAL_ERROR; }
static inline int d2h(void *h, const void *d, size_t n) { return hipMemcpy(h, d, n, hipMemcpyDeviceToHost) == hipSuccess ? OPUSGPU_OK : OPUSGPU_INTERNAL_ERROR; }

// One buffer a kernel works on in place: host -> device, launch(d) (returns an OPUSGPU_* code), device -> host on success.
template <class Launch> static int run_in_place(void *h, size_t bytes, Launch launch)
{
    DevBuf d(bytes);
    int rc = allocated(d);
    if (rc == OPUSGPU_OK) rc = h2d(d.p, h, bytes);
    if (rc == OPUSGPU_OK) rc = launch(d.p);
    if (rc == OPUSGPU_OK) rc = d2h(h, d.p, bytes);
    return rc;
}

// f(std::integral_constant<int, shift>()) for shift 0 .. 3: picks the <SHIFT> instance of a transform kernel
template <class F> static inline void for_shift(int shift, F f)
{
    switch (shift) {
    case 0: f(std::integral_constant<int, 0>()); break;
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    default: f(std::integral_constant<int, 3>()); break;
    }
}

// a zeroed record on the heap: the large records are kept off a codec thread's stack. p == nullptr: the allocation failed.
template <class T> struct HeapRec {
    T *p;
    HeapRec() : p((T *)calloc(1, sizeof(T))) {}
    ~HeapRec() { free(p); }
    HeapRec(const HeapRec &) = delete;
    HeapRec &operator=(const HeapRec &) = delete;
    T *operator->() const { return p; }
};

// ---- one record through a batch entry -----------------------------------------------------------------------------------------
// Scope of a one-record hook: the record kernels it launches count rejected records into a counter of the calling thread
// (runtime.hip), never into the device's shared one that concurrent batch callers read through opusgpu_silk_bad_records().
struct OpusgpuHookBadScope {
    int rc;
    bool open;
    explicit OpusgpuHookBadScope(bool on = true) : rc(on ? opusgpu_private_bad_counter_begin() : OPUSGPU_OK), open(on) {}
    int take() { open = false; return opusgpu_private_bad_counter_end(); }
    ~OpusgpuHookBadScope() { if (open) (void)opusgpu_private_bad_counter_end(); }
};

// how run_record learns that the kernel rejected the record
struct ByStatus {};      // the out record carries a status word
struct ByCounter {};     // it carries none (silk_NSQ, silk_NSQ_del_dec): the thread's private counter is read
struct Unchecked {};     // the kernel rejects nothing and the out record has no status (silk_burg_modified): no scope is opened
struct NoState { int unused; };

// Host in -> device -> host out, with an optional in/out state record (h_state == nullptr: none); launch(d_in, d_state, d_out)
// returns an OPUSGPU_* code. Steps: bad-record scope, allocate, copy in, launch, copy out, the record's status, state copy-back;
// the first one that fails decides the code, and h_state is written only on success.
template <class Check = ByStatus, class In, class Out, class State, class Launch>
static int run_record(const In *h_in, Out *h_out, State *h_state, Launch launch)
{
    OpusgpuHookBadScope bad(!std::is_same<Check, Unchecked>::value);
    if (bad.rc != OPUSGPU_OK) return bad.rc;
    DevBuf din(sizeof(In)), dout(sizeof(Out)), dst(h_state ? sizeof(State) : 1);       // (no state: a one-byte placeholder)
    int rc = allocated(din, dout, dst);
    if (rc == OPUSGPU_OK) rc = h2d(din.p, h_in, sizeof(In));
    if (rc == OPUSGPU_OK && h_state) rc = h2d(dst.p, h_state, sizeof(State));
    if (rc == OPUSGPU_OK) rc = launch((const In *)din.p, h_state ? (State *)dst.p : nullptr, (Out *)dout.p);
    if constexpr (std::is_same<Check, ByCounter>::value) {
        const int n_bad = bad.take();
        if (rc == OPUSGPU_OK && n_bad != 0) rc = n_bad < 0 ? n_bad : OPUSGPU_BAD_ARG;      // header outside the kernels' bounds
    }
    if (rc == OPUSGPU_OK) rc = d2h(h_out, dout.p, sizeof(Out));
    if constexpr (std::is_same<Check, ByStatus>::value)
        if (rc == OPUSGPU_OK) rc = h_out->status;
    if (rc == OPUSGPU_OK && h_state) rc = d2h(h_state, dst.p, sizeof(State));
    return rc;
}

// ---- the range coder's scalars ------------------------------------------------------------------------------------------------
// The eleven of them, field by field, between any two of ca::EcFields (the private records), ref_ec_ctx and the public
// opusgpu_ec_state: same names, three layouts. The one list on the host.
template <class D, class S> static inline void ec_copy_fields(D &d, const S &s)
{
    d.storage = s.storage; d.end_offs = s.end_offs; d.end_window = s.end_window; d.offs = s.offs; d.rng = s.rng; d.val = s.val;
    d.ext = s.ext; d.nend_bits = s.nend_bits; d.nbits_total = s.nbits_total; d.rem = s.rem; d.error = s.error;
}
static inline ca::EcFields ec_fields_from(const ref_ec_ctx *e) { ca::EcFields f; ec_copy_fields(f, *e); return f; }
// every field but storage, which only ec_enc_shrink changes (the script runner writes it back itself)
static inline void ec_fields_to(ref_ec_ctx *e, const ca::EcFields &f)
{
    const uint32_t storage = e->storage;
    ec_copy_fields(*e, f);
    e->storage = storage;
}

// quant_all_bands(encode = 0) as a per-call hook: the record the host entry (quant_bands_hook.hip) hands to the decoder's lane
// build (celt_dec_kernel.hip), and the launcher. In: pulses, tf_res, the scalars, seed, the range decoder's fields + the packet
// bytes; out: X (both channels), collapse_masks, seed, the decoder's fields.
struct opusgpu_qab_dec_record {
    int16_t X[2 * 960];
    int16_t norm[2 * 624];             // working storage (the folding source), not an output
    int32_t pulses[21], tf_res[21];
    int32_t shortBlocks, spread, dual_stereo, intensity, total_bits, balance, codedBands;
    uint32_t seed;
    ca::EcFields ec;
    int32_t pad;
    unsigned char collapse_masks[2 * 21 + 6];
    unsigned char buf[1280];
};
extern "C" int opusgpu_launch_quant_all_bands_dec(opusgpu_qab_dec_record *d_rec);
