"""examples/owlqn_example.cpp through the C++ host mirror (include/qn_solver.hpp): OWLQN(m = 5) + BackTracking(1e-4, 0.5) on the device Logistic
objective at 257 x 200 with an unpenalised intercept column, to 1e-5 at l1 = 4 and on from the same solver at l1 = 2.  The test builds the example
against the library, runs it, and makes the same two runs through the Python class on the same data: the nonzero counts must agree."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def example_data():
    """the example's data, number for number: the same 64-bit linear congruential generator and the same left-to-right sums"""
    m, n, state, mask, root3 = 257, 200, 2027, (1 << 64) - 1, math.sqrt(3.0)

    def nxt():
        nonlocal state
        state = (state * 6364136223846793005 + 1442695040888963407) & mask
        return (float(state >> 11) / 9007199254740992.0 * 2.0 - 1.0) * root3
    a = np.array([nxt() for _ in range(m * n)]).reshape(m, n)
    a[:, 0] = 1.0
    xs = np.array([nxt() if j % 5 == 0 else 0.0 for j in range(n)])
    y, w = np.empty(m), np.empty(m)
    for i in range(m):
        z = 0.5 * nxt()
        for j in range(n):
            z += a[i, j] * xs[j]
        y[i] = 1.0 if z >= 0 else -1.0
        w[i] = 0.0 if i % 7 == 3 else (3.0 if i % 3 == 0 else 1.0)
    return a, y, w


def test_owlqn_example_cpp(qn, tmp_path):
    lib = os.path.join(ROOT, "optimization-solvers_amd", "lib")
    assert os.path.exists(os.path.join(lib, "libqn_hip.so")), "libqn_hip.so is missing: run __graft_entry__.build() first"
    exe = str(tmp_path / "owlqn_example.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "owlqn_example.cpp"),
                           "-o", exe, "-L" + lib, "-lqn_hip", "-Wl,-rpath," + lib])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout.strip().splitlines()
    assert out[-1] == "owlqn example ok"
    pat = r"l1 = (\d): iterations: (\d+) nonzeros: (\d+) of 200 F: (\S+) measure: (\S+) stored pairs: (\d+)"
    runs = [re.match(pat, line) for line in (out[0], out[2])]
    assert all(runs), out
    (l4, it4, nz4, f4, m4, p4), (l2, it2, nz2, f2, m2, p2) = (r.groups() for r in runs)
    assert (l4, l2) == ("4", "2")
    assert float(m4) < 1e-5 and float(m2) < 1e-5
    assert 0 < int(nz4) < int(nz2) < 200
    assert float(f2) < float(f4)  # F at the smaller penalty is below F at the larger one: h only shrinks at any fixed x
    assert 0 < int(it4) <= 2000 and 0 < int(it2) <= 2000
    assert out[1] == f"set_l1: stored pairs: {p4}" and int(p4) == 5  # the memory survives the new penalty
    # the same two runs through the Python class
    a, y, w = example_data()
    obj = qn.Logistic(a, y, 1e-3, weights=w)
    l1 = np.full(200, 4.0)
    l1[0] = 0.0
    s = qn.OWLQN(1e-5, np.zeros(200), l1)
    try:
        ls = qn.BackTracking(1e-4, 0.5)
        s.minimize(ls, obj, 2000, 50)
        assert s.nonzeros() == int(nz4)
        l1[1:] = 2.0
        s.set_l1(l1)
        s.minimize(ls, obj, 2000, 50)
        assert s.nonzeros() == int(nz2)
    finally:
        s.close()
        obj.close()
