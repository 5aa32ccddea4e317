"""GPU test: the C++ host mirror (include/qn_solver.hpp) on the device Multinomial objective -- examples/multinomial_example.cpp, built by
__graft_entry__.build(): NewtonCG + BackTracking on a 257 x 40 problem with 5 classes to ||g||_inf < 1e-7, the iteration counts printed."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_examples_multinomial_cpp():
    exe = os.path.join(ROOT, "examples", "multinomial_example.bin")
    if not os.path.exists(exe):
        import __graft_entry__ as ge
        ge.build()
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"outer iterations: (\d+) inner steps: (\d+) .*\|\|g\|\|_inf: ([0-9.eE+-]+)", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) >= 1 and int(m.group(2)) >= int(m.group(1)) and float(m.group(3)) < 1e-7, p.stdout
    assert p.stdout.strip().endswith("multinomial example ok")
