"""ctypes access to the host-emulation build of the packet parser and the frame loop as opusgpu_packet_parse_batch /
opusgpu_decode_batch_packets run them (tests/emu/celt_dec_multi_emu.cpp) -- TEST INFRASTRUCTURE, in the style of any_emulib.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "emu", "libcelt_dec_multi_emu.so")
_lib = None

# what the sources count under CA_HOST_EMU for the packet layer and the frame loop
COUNTERS = ("pkt_code0", "pkt_code1", "pkt_code2", "pkt_code3", "pkt_code3_vbr", "pkt_code3_cbr", "pkt_padding", "pkt_padding_chained",
            "pkt_size_two_bytes", "multi_frame_decoded", "multi_dtx_lm0", "multi_dtx_lm1", "multi_dtx_lm2", "multi_dtx_lm3",
            "multi_dtx_short", "multi_not_celt", "multi_over_max_frames", "fs_loss_after_short", "fs_short_step_pitch",
            "fs_short_step_noise", "plc_no_history", "plc_pitch_first", "plc_pitch_repeat", "plc_noise")

SENTINEL = 0x5A5A          # what a PCM row holds where the decoder did not write

# opusgpu_packet_frames (include/opusgpu.h)
FRAMES_DTYPE = np.dtype([("ret", np.int32), ("frame_samples", np.int16), ("toc", np.uint8), ("pad_", np.uint8),
                         ("offset", np.int16, 48), ("size", np.int16, 48)])


def lib():
    global _lib
    if _lib is None:
        src = os.path.join(ROOT, "tests", "emu", "celt_dec_multi_emu.cpp")
        d = os.path.join(ROOT, "concentus_amd", "csrc")
        newest = max(os.path.getmtime(f) for f in [os.path.join(d, f) for f in os.listdir(d) if f.endswith(".h")] +
                     [src, os.path.join(ROOT, "include", "opusgpu.h")])
        if not os.path.exists(PATH) or os.path.getmtime(PATH) < newest:
            if any(k.startswith(("ROCP", "ROCPROFILER", "HSA_TOOLS")) for k in os.environ):
                raise RuntimeError("%s must be built before the profiler starts (a plain python3 run does it)" % PATH)
            subprocess.check_call(["g++", "-O2", "-fwrapv", "-std=c++17", "-shared", "-fPIC", "-w", "-o", PATH, src])
        _lib = C.CDLL(PATH)
        _lib.emu_multi_count.restype = C.c_long
        _lib.emu_multi_count.argtypes = [C.c_char_p]
        assert _lib.emu_multi_sizeof_frames() == FRAMES_DTYPE.itemsize == 200
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def parse(packets, lens):
    """emu_packet_parse: packets uint8 [n][stride], lens int32 [n] -> records [n] of FRAMES_DTYPE"""
    packets = np.ascontiguousarray(packets)
    lens = np.ascontiguousarray(lens.astype(np.int32))
    fr = np.zeros(packets.shape[0], FRAMES_DTYPE)
    lib().emu_packet_parse(_p(packets), packets.shape[1], _p(lens), packets.shape[0], _p(fr))
    return fr


def decode(packets, lens, packets_per_stream, frame_size=5760, max_frames=48, fill=SENTINEL):
    """emu_celt_decode_packets: packets uint8 [n][stride], lens int32 [n] (0: lost), stream-major; frame_size an int or int [n].
    Returns pcm [n][max frame_size][2] (pre-filled with `fill`: packet i's first ret[i] sample pairs are written), final range [n],
    ret [n], the frame tables [n]."""
    packets = np.ascontiguousarray(packets)
    lens = np.ascontiguousarray(lens.astype(np.int32))
    n = packets.shape[0]
    fs = np.ascontiguousarray(np.broadcast_to(np.asarray(frame_size, np.int32), (n,)))
    rows = int(fs.max()) if n else 960
    pcm = np.full((n, rows, 2), fill, np.int16)
    rng = np.zeros(n, np.uint32)
    ret = np.zeros(n, np.int32)
    fr = np.zeros(n, FRAMES_DTYPE)
    lib().emu_celt_decode_packets(_p(packets), packets.shape[1], _p(lens), _p(fs), int(max_frames), n, int(packets_per_stream), _p(pcm), rows,
                                  _p(rng), _p(ret), _p(fr))
    return pcm, rng, ret, fr


def counts():
    return {k: int(lib().emu_multi_count(k.encode())) for k in COUNTERS}


def counts_reset():
    lib().emu_multi_counts_reset()
