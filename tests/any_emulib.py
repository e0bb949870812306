"""ctypes access to the host-emulation build of the decoder sources as opusgpu_decode_batch_any runs them
(tests/emu/celt_dec_any_emu.cpp) -- TEST INFRASTRUCTURE, in the style of plc_emulib.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "emu", "libcelt_dec_any_emu.so")
_lib = None

# what the sources count under CA_HOST_EMU for the short frames
COUNTERS = ("fs_lm0", "fs_lm1", "fs_lm2", "fs_lm3", "fs_transient_lm0", "fs_transient_lm1", "fs_transient_lm2", "fs_transient_lm3",
            "fs_anti_collapse_lm2", "fs_mono_lm0", "fs_mono_lm1", "fs_mono_lm2", "fs_loss_after_short", "fs_short_step_pitch", "fs_short_step_noise",
            "plc_no_history", "plc_pitch_first", "plc_pitch_repeat", "plc_noise", "corrupt_silence_long", "corrupt_dec_error")

SENTINEL = 0x5A5A          # what a PCM row holds where the decoder did not write


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "emu", "celt_dec_any_emu.cpp")
        d = os.path.join(ROOT, "concentus_amd", "csrc")
        newest = max(os.path.getmtime(f) for f in [os.path.join(d, f) for f in os.listdir(d) if f.endswith(".h")] + [src])
        if not os.path.exists(PATH) or os.path.getmtime(PATH) < newest:
            if any(k.startswith(("ROCP", "ROCPROFILER", "HSA_TOOLS")) for k in os.environ):
                raise RuntimeError("%s must be built before the profiler starts (a plain python3 run does it)" % PATH)
            subprocess.check_call(["g++", "-O2", "-fwrapv", "-std=c++17", "-shared", "-fPIC", "-w", "-o", PATH, src])
        _lib = C.CDLL(PATH)
        _lib.emu_any_count.restype = C.c_long
        _lib.emu_any_count.argtypes = [C.c_char_p]
    return _lib


def decode(packets, lens, frames_per_stream, fill=SENTINEL):
    """emu_celt_decode_frames_any: packets uint8 [n][stride], lens int32 [n] (0: lost), stream-major.
    Returns pcm [n][960][2] (pre-filled with `fill`: frame i's first ret[i] sample pairs are written), final range [n], ret [n]."""
    packets = np.ascontiguousarray(packets)
    lens = np.ascontiguousarray(lens.astype(np.int32))
    n = packets.shape[0]
    pcm = np.full((n, 960, 2), fill, np.int16)
    rng = np.zeros(n, np.uint32)
    ret = np.zeros(n, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib().emu_celt_decode_frames_any(p(packets), packets.shape[1], p(lens), n, frames_per_stream, p(pcm), p(rng), p(ret))
    return pcm, rng, ret


def counts():
    return {k: int(lib().emu_any_count(k.encode())) for k in COUNTERS}


def counts_reset():
    lib().emu_any_counts_reset()
