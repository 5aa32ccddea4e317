"""GPU test: the C++ host mirror (include/qn_solver.hpp) of NewtonCG's Jacobi preconditioner -- examples/precond_example.cpp, built by
__graft_entry__.build(): NewtonCG + BackTracking on a 257 x 200 logistic regression whose columns differ in scale by three decades, with and without
the preconditioner, to ||g||_inf < 1e-7; the outer and inner counts printed, Jacobi's inner steps at most half the plain run's."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_examples_precond_cpp():
    exe = os.path.join(ROOT, "examples", "precond_example.bin")
    if not os.path.exists(exe):
        import __graft_entry__ as ge
        ge.build()
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    runs = re.findall(r"NewtonCG \((none|jacobi)\).*outer iterations: (\d+) inner steps: (\d+) diagonal passes: (\d+) .*\|\|g\|\|_inf: ([0-9.eE+-]+)", p.stdout)
    assert [r[0] for r in runs] == ["none", "jacobi"], p.stdout
    (_, _, inner0, diag0, g0), (_, outer1, inner1, diag1, g1) = runs
    assert float(g0) < 1e-7 and float(g1) < 1e-7 and int(diag0) == 0 and int(diag1) == int(outer1), p.stdout
    assert 2 * int(inner1) <= int(inner0), p.stdout
    assert p.stdout.strip().endswith("precond example ok")
