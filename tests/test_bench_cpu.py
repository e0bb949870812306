"""CPU tier: bench.py's command line (--full, --dump-outputs) and the writer behind --dump-outputs."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bench  # noqa: E402


def test_a_plain_run_asks_for_neither_baseline_nor_parity_and_full_is_off_by_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    a = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert a.full is True and a.dump_outputs == "somewhere"


def test_masked_packets_keeps_only_the_bytes_of_each_packet():
    out = torch.full((3, 10), 7, dtype=torch.uint8)
    lens = torch.tensor([0, 4, 6], dtype=torch.int32)
    got = bench.masked_packets(out, lens).numpy()
    assert got.shape == (3, 6)
    assert np.array_equal(got, [[0] * 6, [7] * 4 + [0] * 2, [7] * 6])


def test_dump_outputs_is_exact_bounded_and_repeatable(tmp_path):
    g = torch.Generator().manual_seed(1)
    arrays = {
        "bytes": torch.randint(0, 256, (6000, 1500), generator=g, dtype=torch.uint8),          # 36 MB as float32
        "shorts": torch.randint(-32768, 32768, (4000, 960, 2), generator=g, dtype=torch.int16),  # 30.7 MB as float32
        "words": torch.randint(-2 ** 31, 2 ** 31 - 1, (5000,), generator=g, dtype=torch.int32),
        "window": torch.randint(0, 256, (64, 40), generator=g, dtype=torch.uint8)[:, :36],     # a view, as the SILK outputs are
    }
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, arrays)
    bench.dump_outputs(b, arrays)
    assert sorted(os.listdir(a)) == ["bytes.npy", "shorts.npy", "window.npy", "words.npy"]
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 64 * 1000 * 1000
    got = {f[:-4]: np.load(os.path.join(a, f)) for f in os.listdir(a)}
    for f in os.listdir(a):
        assert np.array_equal(got[f[:-4]], np.load(os.path.join(b, f)))
    assert got["bytes"].dtype == np.float32 and got["shorts"].dtype == np.float32 and got["words"].dtype == np.float64
    # small outputs are whole and exact
    assert np.array_equal(got["words"].astype(np.int64), arrays["words"].numpy().astype(np.int64))
    assert np.array_equal(got["window"], arrays["window"].numpy().astype(np.float32))
    # large ones keep rows of the original, in order
    for name in ("bytes", "shorts"):
        full = arrays[name].numpy().astype(np.float32)
        assert 0 < got[name].shape[0] < full.shape[0] and got[name].shape[1:] == full.shape[1:]
        row = 0
        for r in got[name][:16]:
            while not np.array_equal(full[row], r):
                row += 1
            row += 1
