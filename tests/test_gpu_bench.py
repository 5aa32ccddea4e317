"""GPU test of the benchmark's plain run: `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` in a fresh process times exactly one
region of K iterations, prints the headline line without the --full legs, and dumps what the timed path computed -- the same iterate and
inverse Hessian rows as the same sequence of calls (reset, W iterations, K iterations) made here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(qn, tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    steps, warmup = 12, 3
    cp = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                         "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert cp.returncode == 0, cp.stderr[-2000:]
    line = json.loads(cp.stdout.strip().splitlines()[-1])
    assert line["unit"] == "iterations/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == steps and line["warmup"] == warmup and line["timing"]["regions"] == 1
    assert line["iteration_accounting"]["h_passes"] > 0 and line["value"] > 0
    assert abs(line["ms_per_step"] - 1e3 / line["value"]) <= 1e-9 * line["ms_per_step"]
    assert line["roofline"] is None and not ({"cpu_baseline", "extra_configs", "strong_scaling_ref"} & set(line))

    n = line["config"]["n"]
    diag, b, x0 = bench.synth_inputs(n)
    obj = qn.Quadratic.synthetic(n, bench.SEED, diag, b)
    s = qn.BFGS(1e-10, x0)
    ls = qn.MoreThuente()
    s.reset(x0)
    bench.run_iterations(qn, s, ls, obj, x0, warmup)
    bench.run_iterations(qn, s, ls, obj, x0, steps)
    x = np.load(tmp_path / "x.npy")
    assert x.dtype == np.float64 and x.shape == (n,)
    assert np.linalg.norm(x - s.x()) <= 1e-12 * max(1.0, np.linalg.norm(s.x()))
    assert np.load(tmp_path / "k.npy").tolist() == [float(s.k())]
    rows = np.load(tmp_path / "inv_hessian_row_index.npy").astype(np.int64)
    hr = np.load(tmp_path / "inv_hessian_rows.npy")
    h = s.approx_inv_hessian()[rows]
    assert hr.shape == (len(rows), n) and np.abs(hr - h).max() <= 1e-12 * np.abs(h).max()
