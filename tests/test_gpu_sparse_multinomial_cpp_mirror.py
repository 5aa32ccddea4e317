"""GPU test: the C++ host mirror (include/qn_solver.hpp) on the device SparseMultinomial objective -- examples/sparse_multinomial_example.cpp, built by
__graft_entry__.build(): NewtonCG + BackTracking on a 400 x 20000 problem (8 nonzeros per row plus an intercept column) with 12 classes, N = 240 000,
to ||g||_inf < 1e-7.  The same problem is drawn here by the example's linear congruence and run through the Python layer: the example prints the Python
run's iteration counts."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, N_FEATURES, K, PER_ROW = 400, 20000, 12, 8


def example_problem():
    """the example's problem, draw for draw: (indptr, indices, data, y, w)"""
    state = 2031
    mask = (1 << 64) - 1

    def next_u():
        nonlocal state
        state = (state * 6364136223846793005 + 1442695040888963407) & mask
        return state >> 11

    def nxt():
        return (next_u() / 9007199254740992.0 * 2.0 - 1.0) * math.sqrt(3.0)
    ws = np.array([nxt() for _ in range(K * N_FEATURES)]).reshape(K, N_FEATURES)
    indptr, indices, data, y, w = [0], [], [], [], []
    for i in range(M):
        cols = []
        while len(cols) < PER_ROW:
            c = 1 + next_u() % (N_FEATURES - 1)
            if c not in cols:
                cols.append(c)
        cols.sort()
        vals = [nxt() for _ in range(PER_ROW)]
        indices += [0] + cols
        data += [1.0] + vals
        indptr.append(len(indices))
        best, label = -math.inf, 0
        for k in range(K):
            z = ws[k, 0] + 0.5 * nxt()
            for e in range(PER_ROW):
                z += vals[e] * ws[k, cols[e]]
            if z > best:
                best, label = z, k
        y.append(label)
        w.append(0.0 if i % 7 == 3 else (3.0 if i % 3 == 0 else 1.0))
    return np.array(indptr, dtype=np.int32), np.array(indices, dtype=np.int32), np.array(data), np.array(y, dtype=np.int32), np.array(w)


def test_examples_sparse_multinomial_cpp(qn):
    exe = os.path.join(ROOT, "examples", "sparse_multinomial_example.bin")
    if not os.path.exists(exe):
        import __graft_entry__ as ge
        ge.build()
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"outer iterations: (\d+) inner steps: (\d+) .*products: (\d+) f: ([0-9.eE+-]+) \|\|g\|\|_inf: ([0-9.eE+-]+)", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) >= 1 and int(m.group(2)) >= int(m.group(1)) and float(m.group(5)) < 1e-7, p.stdout
    assert p.stdout.strip().endswith("sparse multinomial example ok")
    # the Python layer on the same problem: the same counts, the same f
    indptr, indices, data, y, w = example_problem()
    obj = qn.SparseMultinomial(indptr, indices, data, y, K, 0.5, N_FEATURES, weights=w)
    s = qn.NewtonCG(1e-7, np.zeros(K * N_FEATURES))
    try:
        assert (obj.nnz, obj.n, obj.kp, obj.n_long_cols) == (M * (PER_ROW + 1), K * N_FEATURES, 16, 0)
        s.minimize(qn.BackTracking(1e-4, 0.5), obj, 60, 30)
        assert (s.k(), s.inner_iterations()[1], s.hv_passes()) == (int(m.group(1)), int(m.group(2)), int(m.group(3))), p.stdout
        assert abs(obj(s.x()).f() - float(m.group(4))) <= 1e-11 * abs(float(m.group(4)))
    finally:
        s.close()
        obj.close()
