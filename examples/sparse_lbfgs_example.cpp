// examples/sparse_lbfgs_example.cpp -- the sparse quadratic objective through the C++ host mirror (qn_solver.hpp): LBFGS + StrongWolfe on
// min 1/2 x'Qx - b'x with Q the 2-D five-point Laplacian of a 64 x 64 grid plus a shift of 0.05 (SPD, 20 224 nonzeros in CSR), b = 1.  The
// matrix lives on the device as CSR; no evaluation crosses the bus.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "qn_solver.hpp"

using namespace optimization_solvers;

int main() {
    const int32_t side = 64, n = side * side;
    const Floating shift = 0.05;
    std::vector<int32_t> indptr(1, 0), indices;
    DVector data;
    for (int32_t i = 0; i < side; ++i)
        for (int32_t j = 0; j < side; ++j) { // row i * side + j, its columns in increasing order
            const int32_t r = i * side + j;
            if (i > 0) { indices.push_back(r - side); data.push_back(-1.0); }
            if (j > 0) { indices.push_back(r - 1); data.push_back(-1.0); }
            indices.push_back(r); data.push_back(4.0 + shift);
            if (j + 1 < side) { indices.push_back(r + 1); data.push_back(-1.0); }
            if (i + 1 < side) { indices.push_back(r + side); data.push_back(-1.0); }
            indptr.push_back((int32_t)indices.size());
        }
    const DVector b(n, 1.0), x0(n, 0.0);
    SparseQuadratic objective(indptr, indices, data, b);
    std::printf("n: %d nnz: %zu lanes per row: %d long rows: %zu symmetric: %d\n", n, objective.nnz(), objective.lanes_per_row(), objective.n_long_rows(),
                (int)objective.symmetric());
    if (objective.nnz() != data.size() || !objective.symmetric() || objective.n_long_rows() != 0) { std::printf("unexpected shape\n"); return 1; }

    const Floating tol = 1e-6; // (f is -3e4 here: a decrease of ||g||^2 / L below 1e-12 is under f's last bit, so the searches cannot go on much further)
    auto sw = StrongWolfe::new_(1e-4, 0.9);
    auto solver = LBFGS::new_(tol, x0).with_memory(5);
    Result r = solver.minimize(sw, objective, 1000, 100);
    if (r.is_err()) { std::printf("optimization failed: %s\n", r.unwrap_err().what()); return 1; }
    const auto eval = objective(solver.x());
    Floating ginf = 0.0;
    for (Floating v : eval.g()) ginf = std::fmax(ginf, std::fabs(v));
    std::printf("k: %zu f: %.12e ||g||_inf: %.3e\n", solver.k(), eval.f(), ginf);
    // at the minimiser f = -1/2 b'x with Q x = b; the constant vector 1 / shift solves the problem without its boundary, so 0 < x < 1 / shift
    Floating bx = 0.0;
    bool inside = true;
    for (Floating v : solver.x()) { bx += v; inside = inside && v > 0.0 && v < 1.0 / shift; }
    if (!(ginf < tol) || !solver.has_converged(eval) || !inside || std::fabs(eval.f() + 0.5 * bx) > 1e-6 * std::fabs(eval.f())) {
        std::printf("not at the minimum\n");
        return 1;
    }
    std::printf("sparse lbfgs example ok\n");
    return 0;
}
