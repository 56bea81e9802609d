"""bench.py's contract: a plain run times --steps steps and prints the headline line only; --dump-outputs DIR writes what the last timed
step computed as float32 / float64 .npy files, under 64 MB in all, the same in every run with the same arguments."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    def run(out):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "64",
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    out = tmp_path / "dump"
    line = run(out)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "molecules/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert abs(line["value"] - 64 * 1e3 / line["ms_per_step"]) <= 1e-2 * line["value"]
    # what only --full measures is not in a plain run
    assert not {"roofline", "site_roofline", "step_roofline", "padded_layout", "cpu_baseline", "batch_sweep"} & set(line)
    files = {os.path.basename(f)[:-4]: f for f in glob.glob(str(out / "*.npy"))}
    assert set(files) == {"h_e3gnn", "h_smiles", "bad_rows", "ar_loss", "clip_loss", "loss", "grad_norm", "n_targets", "n_valid"}
    assert sum(os.path.getsize(f) for f in files.values()) <= 64 << 20
    arrays = {k: np.load(f) for k, f in files.items()}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert arrays["h_e3gnn"].shape == arrays["h_smiles"].shape == (64, 256)
    assert all(np.isfinite(a).all() for a in arrays.values())
    assert abs(float(arrays["ar_loss"][0]) - line["loss"]["ar_loss"]) < 1e-3
    # a second run with the same arguments: same inputs, so the same outputs up to the rounding of the engine's f32 atomic sums
    run(tmp_path / "again")
    for k, a in arrays.items():
        b = np.load(str(tmp_path / "again" / (k + ".npy")))
        assert float(np.abs(b.astype(np.float64) - a).max()) <= 1e-5 * max(float(np.abs(a).max()), 1e-30), k
