"""GPU test: the C++ host mirror (include/qn_solver.hpp) of PnormDescent, CoordinateDescent and NoSearch running the reference's own
pnorm_morethuente / coordinate_descent_morethuente problems (examples/pnorm_example.cpp, built by __graft_entry__.build())."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_examples_pnorm_cpp():
    exe = os.path.join(ROOT, "examples", "pnorm_example.bin")
    assert os.path.exists(exe), "examples/pnorm_example.bin is missing: run __graft_entry__.build() first"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "|f| < 1e-6" in p.stdout and "iterations: 1" in p.stdout  # pnorm_descent.rs:139 assert!((eval.f() - 0.0).abs() < 1e-6)
    assert "PnormDescent + NoSearch: iterations: 1" in p.stdout and p.stdout.strip().endswith("pnorm example ok")
