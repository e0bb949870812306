"""GPU tier: a plain `bench.py --gpus 1` run -- the result line carries what the steps need and nothing that takes a run of its
own, --steps sets the number of timed steps, and --dump-outputs writes what the timed path returned: the files are compared
with encode_independent() called directly on the same seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 512


def test_plain_run_dumps_the_packets_of_the_last_step(tmp_path):
    import concentus_amd as ca
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--frames", str(F), "--steps", "3", "--warmup", "1",
                        "--dump-outputs", d], cwd=ROOT, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stderr[-3000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["higher_is_better"] is True and line["unit"] == "frames/s" and line["config"]["frames_per_gpu"] == F
    assert abs(line["value"] - F * 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"]
    assert "cpu_baseline" not in line and line["parity_checked"] == 0            # those belong to --full

    pcm = np.random.default_rng(3).integers(-8192, 8192, size=(F, 960, 2), dtype=np.int16)      # the batch bench.py draws for rank 0
    out, lens, rng = ca.encode_independent(torch.from_numpy(pcm).to("cuda:0"), ca.default_config(2, 96000))
    torch.cuda.synchronize()
    out, lens, rng = out.cpu().numpy(), lens.cpu().numpy(), rng.cpu().numpy()
    assert sorted(os.listdir(d)) == ["final_range.npy", "lengths.npy", "packets.npy"]
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert got["packets"].dtype == np.float32 and got["lengths"].dtype == np.float64 and got["final_range"].dtype == np.float64
    assert np.array_equal(got["lengths"], lens) and np.array_equal(got["final_range"], rng)
    w = int(lens.max())
    assert got["packets"].shape == (F, w)
    assert np.array_equal(got["packets"], np.where(np.arange(w)[None, :] < lens[:, None], out[:, :w], 0))
