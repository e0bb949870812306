"""Timing of opusgpu_decode_batch_packets beside opusgpu_decode_batch_any ("Multi-frame packets").

    python tools/decode_packets_bench.py [--streams 65536] [--runs 3] [--steps 5]

Legs, each `runs` times in turn (so that drift hits all alike), one JSON line per leg and run:
  any        bench.py's decode batch (fresh-decoder 0xFC packets, GPU-encoded) through decode(any_frame_size=True)
  packets1   the same batch through decode_packets(max_frames=1, frame_size=960)
  multi3x20  the same frames, three to a VBR code-3 packet, decode_packets(max_frames=3, frame_size=2880)
  multi8x2p5 the 2.5 ms stereo packets of tests/golden/any_golden.npz, eight to a packet, decode_packets(max_frames=8, frame_size=960)
Whole-call time is taken with HIP events around `steps` calls (state reset outside the events); the per-kernel times come from the
library's timing hooks in a separate pass, since their events sit between the launches."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import concentus_amd as ca  # noqa: E402


def _header_ids():
    """OPUSGPU_KERNEL_* of include/opusgpu.h: the decoder's four timing ids and the table's length"""
    import re
    text = open(os.path.join(ROOT, "include", "opusgpu.h")).read()
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define OPUSGPU_KERNEL_(\w+)\s+(\d+)", text)}
    return {d["DEC_LANE"]: "lane", d["DEC_SYNTH"]: "synth", d["DEC_POST"]: "post", d["DEC_PLC"]: "plc"}, d["COUNT"]


KNAMES, NK = _header_ids()


def size_bytes(n):
    return bytes([n]) if n < 252 else bytes([252 + (n & 3), (n - (252 + (n & 3))) >> 2])


def code3_vbr(frames):
    """frames: code-0 packets of one TOC -> one VBR code-3 packet"""
    toc = frames[0][0]
    body = [f[1:] for f in frames]
    return bytes([toc | 3, 0x80 | len(frames)]) + b"".join(size_bytes(len(b)) for b in body[:-1]) + b"".join(body)


def slab(packets):
    stride = max(len(p) for p in packets) + 3 & ~3
    pk = np.zeros((len(packets), stride), np.uint8)
    for k, p in enumerate(packets):
        pk[k, :len(p)] = np.frombuffer(p, np.uint8)
    return torch.from_numpy(pk).cuda(), torch.tensor([len(p) for p in packets], dtype=torch.int32).cuda()


def measure(dec, call, steps, frames_per_call):
    L = ca.lib.load()
    dec.reset()
    call()                                                   # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        dec.reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _pcm, ret = call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    assert (ret > 0).all().item(), "a stream was rejected"
    dec.reset()
    L.opusgpu_kernel_timing_enable(1)
    call()
    ksum, kcnt = (C.c_double * NK)(), (C.c_int * NK)()
    ca.lib.check(L.opusgpu_kernel_timing_read(ksum, kcnt, NK), "opusgpu_kernel_timing_read")
    L.opusgpu_kernel_timing_enable(0)
    med = float(np.median(ms))
    return {"call_ms_median": round(med, 4), "call_ms": [round(m, 4) for m in ms], "frames_per_s": round(frames_per_call / (med * 1e-3)),
            "kernel_ms_per_call": {KNAMES[i]: round(ksum[i], 4) for i in KNAMES if kcnt[i]},
            "launches": {KNAMES[i]: kcnt[i] for i in KNAMES if kcnt[i]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--legs", default="any,packets1,multi3x20,multi8x2p5", help="comma-separated (`any` alone also runs on a library without the packet entry points)")
    a = ap.parse_args()
    F = a.streams
    host = np.random.default_rng(3).integers(-8192, 8192, size=(F, 960, 2), dtype=np.int16)
    pk, ln, _r = ca.encode_independent(torch.from_numpy(host).cuda(), ca.default_config(2, 96000))
    torch.cuda.synchronize()
    hpk, hln = pk.cpu().numpy(), ln.cpu().numpy()
    code0 = [hpk[k, :hln[k]].tobytes() for k in range(F)]
    assert all(p[0] == 0xFC for p in code0)
    pk3, ln3 = slab([code3_vbr([code0[k], code0[(k + 1) % F], code0[(k + 2) % F]]) for k in range(F)])
    g = np.load(os.path.join(ROOT, "tests", "golden", "any_golden.npz"))
    spk, sln = g["static_e4_packets"], g["static_e4_len"]
    short = [spk[k, :sln[k]].tobytes() for k in range(len(sln))]
    pk8, ln8 = slab([code3_vbr([short[(k + j) % len(short)] for j in range(8)]) for k in range(F)])
    dec = ca.OpusDecoderBatch(F)
    legs = [("any", lambda: dec.decode(pk, ln, any_frame_size=True), F),
            ("packets1", lambda: dec.decode_packets(pk, ln, frame_size=960, max_frames=1), F),
            ("multi3x20", lambda: dec.decode_packets(pk3, ln3, frame_size=2880, max_frames=3), 3 * F),
            ("multi8x2p5", lambda: dec.decode_packets(pk8, ln8, frame_size=960, max_frames=8), 8 * F)]
    legs = [leg for leg in legs if leg[0] in a.legs.split(",")]
    for run in range(a.runs):
        for name, call, frames in legs:
            r = measure(dec, call, a.steps, frames)
            r.update({"leg": name, "run": run, "streams": F})
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
