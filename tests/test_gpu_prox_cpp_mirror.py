"""examples/lasso_example.cpp through the C++ host mirror (include/qn_solver.hpp): SpectralProximalGradient + GLLQuadratic(1e-4, 10) on the device
Logistic objective at 257 x 200 with an unpenalised intercept column, to 1e-7 at l1 = 4 and on from the same solver at l1 = 2.  The test builds the
example against the library and runs it."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lasso_example_cpp(tmp_path):
    lib = os.path.join(ROOT, "optimization-solvers_amd", "lib")
    assert os.path.exists(os.path.join(lib, "libqn_hip.so")), "libqn_hip.so is missing: run __graft_entry__.build() first"
    exe = str(tmp_path / "lasso_example.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "lasso_example.cpp"),
                           "-o", exe, "-L" + lib, "-lqn_hip", "-Wl,-rpath," + lib])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout.strip().splitlines()
    assert out[-1] == "lasso example ok"
    runs = [re.match(r"l1 = (\d): iterations: (\d+) nonzeros: (\d+) of 200 F: (\S+) measure: (\S+)", line) for line in out[:2]]
    assert all(runs), out
    (l4, it4, nz4, f4, m4), (l2, it2, nz2, f2, m2) = (r.groups() for r in runs)
    assert (l4, l2) == ("4", "2")
    assert float(m4) < 1e-7 and float(m2) < 1e-7
    assert 0 < int(nz4) < 200 and 0 < int(nz2) < 200
    assert float(f2) < float(f4)  # F at the smaller penalty is below F at the larger one: h only shrinks at any fixed x
    assert 0 < int(it4) <= 2000 and 0 < int(it2) <= 2000
