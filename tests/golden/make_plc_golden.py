"""Golden vectors of the packet loss concealment: the compiled reference's opus_decode() output (PCM, final range) for existing
golden streams with some packets lost (length 0) or replaced by the one-byte DTX packet 0xFC. The packets themselves are not
stored again: they come from encode_golden.npz / decode_golden.npz. Writes tests/golden/plc_golden.npz.

    python tests/golden/make_plc_golden.py        (needs oracle/_ref/librefdrv.so)
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "plc_golden.npz")


def _runs(*spans):
    out = []
    for s in spans:
        out += [s] if isinstance(s, int) else list(range(s[0], s[1] + 1))
    return out


# name -> (npz with the packets, frames per stream, per stream: (lost frames, frames replaced by a one-byte 0xFC packet)).
# gmusic: single, double, seven and twelve losses in a row (pitch-based, then noise-based from the sixth, loss_count >= 10 at the
# recovery) and DTX; its second stream loses its very first packet (no history: zeros). The other three carry runs of 1, 2 and 6
# at different places in each stream; the 8-frame edge streams have no room for all three, so 1 and 2 go to one and 6 to the other.
PLC_CASES = {
    "gmusic_cvbr_stream": ("encode_golden.npz", 48, [
        (_runs(5, (9, 10), (14, 20), (25, 36)), [40]),
        (_runs(0, (3, 4), (8, 13), 20, (24, 34)), [44]),
    ]),
    "music_vbr_stream": ("encode_golden.npz", 16, [
        (_runs(2, (5, 6), (9, 14)), []),
        (_runs((1, 6), 9, (12, 13)), []),
    ]),
    "noise_cvbr_stream": ("encode_golden.npz", 16, [
        (_runs((1, 2), 5, (8, 13)), []),
        (_runs((3, 8), (11, 12), 14), []),
    ]),
    "dec_edge_40k_cbr_stream": ("decode_golden.npz", 8, [
        (_runs(1, (3, 4), 6), []),
        (_runs((2, 7)), []),
    ]),
}


def case_packets(name):
    """(packets [n][stride], lengths [n] with the case's losses applied: 0 = lost, 1 = DTX, frames per stream)."""
    src, fps, streams = PLC_CASES[name]
    g = np.load(os.path.join(HERE, src))
    pk = np.ascontiguousarray(g[name + "_packets"])
    ln = g[name + "_len"].astype(np.int32).copy()
    assert pk.shape[0] == fps * len(streams)
    for s, (lost, dtx) in enumerate(streams):
        ln[s * fps + np.asarray(lost, int)] = 0
        if dtx:
            assert (pk[s * fps + np.asarray(dtx, int), 0] == 0xFC).all()
            ln[s * fps + np.asarray(dtx, int)] = 1
    return pk, ln, fps


def plc_vectors():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    gm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gm)
    out = {}
    for name in PLC_CASES:
        pk, ln, fps = case_packets(name)
        pcm, rng, ret = gm.ref_decode(pk, ln, fps)
        assert (ret == 960).all(), name
        assert (rng[ln <= 1] == 0).all(), name
        out[name + "_len"] = ln                    # the loss mask, as the lengths handed to opus_decode
        out[name + "_pcm"] = pcm
        out[name + "_rng"] = rng
    # the frame that opus_decode(st, NULL, 0, ...) gives after all 16 packets of music_vbr_stream's first stream
    pk, ln, fps = after16_packets()
    pcm, rng, ret = gm.ref_decode(pk, ln, fps)
    assert (ret == 960).all() and rng[-1] == 0
    out["music_vbr_stream_after16_pcm"] = pcm[-1]
    return out


def after16_packets():
    """music_vbr_stream's first stream, received whole, and a 17th packet that is lost."""
    g = np.load(os.path.join(HERE, "encode_golden.npz"))
    pk = np.ascontiguousarray(g["music_vbr_stream_packets"][:16])
    ln = g["music_vbr_stream_len"][:16].astype(np.int32)
    return np.concatenate([pk, pk[:1]]), np.concatenate([ln, np.zeros(1, np.int32)]), 17


if __name__ == "__main__":
    np.savez_compressed(OUT, **plc_vectors())
    print("wrote plc_golden.npz (%d bytes)" % os.path.getsize(OUT))
