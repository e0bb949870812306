"""ctypes access to the host-emulation build of the decoder sources with packet loss concealment (tests/emu/celt_plc_emu.cpp)
-- TEST INFRASTRUCTURE, in the style of emulib.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "emu", "libcelt_plc_emu.so")
_lib = None

# the branches of a concealed frame that the sources count under CA_HOST_EMU
COUNTERS = ("plc_no_history", "plc_pitch_first", "plc_pitch_repeat", "plc_noise", "plc_pitch_postfilter_gain",
            "plc_explosion_zeroed", "plc_explosion_attenuated", "plc_recover_after_10")


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "emu", "celt_plc_emu.cpp")
        d = os.path.join(ROOT, "concentus_amd", "csrc")
        newest = max(os.path.getmtime(f) for f in [os.path.join(d, f) for f in os.listdir(d) if f.endswith(".h")] + [src])
        if not os.path.exists(PATH) or os.path.getmtime(PATH) < newest:
            if any(k.startswith(("ROCP", "ROCPROFILER", "HSA_TOOLS")) for k in os.environ):
                raise RuntimeError("%s must be built before the profiler starts (a plain python3 run does it)" % PATH)
            subprocess.check_call(["g++", "-O2", "-fwrapv", "-std=c++17", "-shared", "-fPIC", "-w", "-o", PATH, src])
        _lib = C.CDLL(PATH)
        _lib.emu_plc_count.restype = C.c_long
        _lib.emu_plc_count.argtypes = [C.c_char_p]
    return _lib


def decode(packets, lens, frames_per_stream):
    """emu_celt_decode_frames_plc: packets uint8 [n][stride], lens int32 [n] (0, or 1 with TOC 0xFC: concealed), stream-major.
    Returns pcm [n][960][2], final range [n], ret [n]."""
    packets = np.ascontiguousarray(packets)
    lens = np.ascontiguousarray(lens.astype(np.int32))
    n = packets.shape[0]
    pcm = np.zeros((n, 960, 2), np.int16)
    rng = np.zeros(n, np.uint32)
    ret = np.zeros(n, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib().emu_celt_decode_frames_plc(p(packets), packets.shape[1], p(lens), n, frames_per_stream, p(pcm), p(rng), p(ret))
    return pcm, rng, ret


def counts():
    return {k: int(lib().emu_plc_count(k.encode())) for k in COUNTERS}


def counts_reset():
    lib().emu_plc_counts_reset()
