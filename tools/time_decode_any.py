"""Throughput of opusgpu_decode_batch_any: N streams (default 65 536) of one packet kind -- 0xF4 (10 ms), 0xEC (5 ms), 0xE4 (2.5 ms),
0xFC (20 ms) -- and an even mix of the four, each packet through a fresh decoder. HIP events around the call, median of 7
after a warm-up; prints one JSON line per batch: ms per call, packets/s and decoded audio seconds per second.

    python tools/time_decode_any.py [--streams N]

The packets are the fixture's (tests/golden/any_golden.npz: static_f4, static_ec, static_e4; 0xFC from fs_switch_stream), tiled."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def packets_of(g, case, toc):
    pk, ln = g[case + "_packets"], g[case + "_len"]
    sel = (pk[:, 0] == toc) & (ln > 2)
    return pk[sel], ln[sel]


def main():
    import torch
    import concentus_amd as ca
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    a = ap.parse_args()
    n = a.streams
    g = np.load(os.path.join(ROOT, "tests", "golden", "any_golden.npz"))
    kinds = {"0xF4": packets_of(g, "static_f4", 0xF4), "0xEC": packets_of(g, "static_ec", 0xEC), "0xE4": packets_of(g, "static_e4", 0xE4),
             "0xFC": packets_of(g, "fs_switch_stream", 0xFC)}
    stride = max(p.shape[1] for p, _l in kinds.values()) + 3 & ~3
    ca.lib.load()

    def batch(names):
        pk = np.zeros((n, stride), np.uint8)
        ln = np.zeros(n, np.int32)
        for s in range(len(names)):
            p, l = kinds[names[s]]
            idx = np.arange(s, n, len(names))
            src = (idx // len(names)) % len(l)
            pk[idx, :p.shape[1]] = p[src]
            ln[idx] = l[src]
        return torch.from_numpy(pk).cuda(), torch.from_numpy(ln).cuda()

    for label, names in (("0xF4", ["0xF4"]), ("0xEC", ["0xEC"]), ("0xE4", ["0xE4"]), ("0xFC", ["0xFC"]), ("mix", ["0xF4", "0xEC", "0xE4", "0xFC"])):
        d_pk, d_ln = batch(names)
        dec = ca.OpusDecoderBatch(n)
        pcm = torch.zeros((n, 960, 2), dtype=torch.int16, device="cuda")
        ms = []
        for it in range(8):                        # the first is the warm-up
            dec.reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _p, ret = dec.decode(d_pk, d_ln, any_frame_size=True, out=pcm)
            e1.record()
            torch.cuda.synchronize()
            if it:
                ms.append(e0.elapsed_time(e1))
        r = ret.cpu().numpy()
        assert (r > 0).all(), r[r <= 0][:8]
        med = float(np.median(ms))
        print(json.dumps({"batch": label, "streams": n, "ms_per_call": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                          "packets_per_s": round(n / (med * 1e-3)), "audio_s_per_s": round(float(r.sum()) / 48000 / (med * 1e-3), 1)}))


if __name__ == "__main__":
    main()
