"""GPU test: the C++ host mirror (include/qn_solver.hpp) of the sparse quadratic objective -- LBFGS + StrongWolfe on the five-point Laplacian of a
64 x 64 grid plus a shift, the matrix on the device as CSR (examples/sparse_lbfgs_example.cpp, built by __graft_entry__.build())."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_examples_sparse_lbfgs_cpp():
    exe = os.path.join(ROOT, "examples", "sparse_lbfgs_example.bin")
    assert os.path.exists(exe), "examples/sparse_lbfgs_example.bin is missing: run __graft_entry__.build() first"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "n: 4096 nnz: 20224 " in p.stdout and "symmetric: 1" in p.stdout
    m = re.search(r"k: (\d+) f: (\S+) \|\|g\|\|_inf: (\S+)", p.stdout)
    assert m and 0 < int(m.group(1)) < 1000 and float(m.group(2)) < 0.0 and float(m.group(3)) < 1e-6
    assert p.stdout.strip().endswith("sparse lbfgs example ok")
