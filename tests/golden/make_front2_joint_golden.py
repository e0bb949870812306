#!/usr/bin/env python3
"""Records tests/golden/front2_joint_golden.npz: what the compiled reference (oracle/_ref, built where the reference sources
exist) encodes from the inputs of tests/front2_joint_cases.py -- packets, lengths, final ranges -- and a digest of each
input. Also runs the host build of the kernel sources on the same inputs and refuses to write unless the short-block path
and the transient patch's second transform both ran a fair number of times."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import emulib                      # noqa: E402
import encode_cases as ec          # noqa: E402
import front2_joint_cases as fj    # noqa: E402


def emu_counts(pcm, fps):
    emu = emulib.lib()
    emu.emu_counts_reset()
    n = pcm.shape[0]
    cfg = emulib.Config(2, fj.CFG[0], fj.CFG[1], fj.CFG[2], fj.CFG[3], 16, 0, 1500)
    out, lens, rng = np.zeros((n, 1280), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    st = emulib.fresh_states(n // fps) if fps > 1 else None
    emu.emu_celt_encode_frames_split(C.byref(cfg), p(st) if st is not None else None, p(np.ascontiguousarray(pcm)), n, fps,
                                     p(out), 1280, p(lens), p(rng))
    buf = C.create_string_buffer(1 << 16)
    emu.emu_counts_dump(buf, len(buf))
    cnt = {l.split()[0]: int(l.split()[1]) for l in buf.value.decode().splitlines()}
    return (out, lens, rng), cnt.get("front_mdct_short", 0), cnt.get("front_mdct_redo", 0)


def main():
    gm = ec.golden_module()
    cfg = gm._Cfg(2, fj.CFG[0], fj.CFG[1], fj.CFG[2], fj.CFG[3], 16, 0, 1500)
    out = {}
    sets = [(name, fn(), 1) for name, fn in fj.INDEPENDENT] + [("streams", fj.streams(), fj.STREAM_FRAMES)]
    for name, pcm, fps in sets:
        pk, ln, rg = gm.ref_encode(cfg, pcm, fps, threads=8)
        got, short, redo = emu_counts(pcm, fps)
        ec.assert_packets_equal(got[0], got[1], got[2], pk, ln, rg, name + " (host build)")
        print("%-18s %4d frames: short-block transforms %d, second transforms after the patch %d" % (name, len(ln), short, redo))
        if name == "attack":
            assert short >= 32, "the attack frames do not reach the short-block path"
        if name == "streams":
            assert redo >= 32 and len(ln) - short - redo >= 32, "the streams do not reach the transient patch and plain long blocks"
        w = int(ln.max())
        out[name + "_packets"], out[name + "_len"], out[name + "_rng"] = pk[:, :w].copy(), ln, rg
        out[name + "_pcm_sha256"] = np.array(fj.digest(pcm))
    np.savez_compressed(os.path.join(HERE, "front2_joint_golden.npz"), **out)
    print("wrote front2_joint_golden.npz")


if __name__ == "__main__":
    main()
