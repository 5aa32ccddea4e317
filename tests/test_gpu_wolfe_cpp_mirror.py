"""GPU test: the C++ host mirror (include/qn_solver.hpp) of the StrongWolfe line search -- LBFGS on the ill-conditioned quadratic of
examples/lbfgs_example.cpp, then ProjectedLBFGS with the search holding the solver's box (examples/wolfe_example.cpp, built by
__graft_entry__.build())."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_examples_wolfe_cpp():
    exe = os.path.join(ROOT, "examples", "wolfe_example.bin")
    assert os.path.exists(exe), "examples/wolfe_example.bin is missing: run __graft_entry__.build() first"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "LBFGS + StrongWolfe: |f| < 1e-6" in p.stdout and "resets: 0" in p.stdout
    assert "ProjectedLBFGS + StrongWolfe (boxed): x: [" in p.stdout and p.stdout.strip().endswith("wolfe example ok")
