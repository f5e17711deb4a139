"""bench.py as every change runs it: a plain run (`--gpus 1 --steps K --warmup W`) times exactly K steps, prints the
contract keys and runs no side measurement; `--dump-outputs DIR` writes what the last timed step computed -- a fixed,
seeded sample of the rows of the float64 moment matrix -- and those rows are the batch path's moments of the bench's own
synthetic frame (against the CPU oracle)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_close

pytestmark = pytest.mark.gpu


def test_plain_run_times_k_steps_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "outputs"
    frame, K = 512, 32
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--frame", str(frame), "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert line["roofline"]["launches"] >= 3
    for side in ("cpu_baseline", "clustering", "dense_frame", "host_api", "north_star_4096", "symmetry_pipeline"):
        assert side not in line
    assert "this_box" not in line["roofline"]

    n_side = frame - K + 1
    n = n_side * n_side
    rows = np.load(out / "moment_rows.npy")
    got = np.load(out / "moments.npy")
    assert rows.dtype == np.float64 and got.dtype == np.float64
    assert got.shape == (rows.size, 45) and got.nbytes + rows.nbytes <= 64 << 20
    assert 0 < rows.size < n and np.all(np.diff(rows) > 0) and rows[-1] < n         # a sample: the matrix is larger
    want = np.sort(np.random.default_rng(0).choice(n, size=_bench().DUMP_BYTES // (8 * 46), replace=False))
    np.testing.assert_array_equal(rows, want)                                         # the same rows on every run

    from mtflearn_amd import ZPs
    from mtflearn_amd.synthetic import honeycomb_frame
    from oracle import zernike_oracle as zo
    img = honeycomb_frame(frame, seed=0)
    pick = np.linspace(0, rows.size - 1, 2000).astype(np.int64)
    r = rows[pick].astype(np.int64)
    patches = np.stack([img[i // n_side:i // n_side + K, i % n_side:i % n_side + K] for i in r])
    rel_close(got[pick], zo.moments_patches(patches, ZPs(n_max=8, size=K).polynomials))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod
