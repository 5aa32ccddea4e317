// examples/exact_cg_example.cpp -- linear conjugate gradients through the C++ host mirror (qn_solver.hpp): NonlinearCG (Fletcher-Reeves) with the
// ExactQuadratic line search on the problem of cg_example.cpp: min 1/2 x'Qx - b'x with Q the 2-D five-point Laplacian of a 64 x 64 grid plus a
// shift of 0.05 (SPD, 20 224 nonzeros in CSR), b = 1.  The step along d is -g.d / d'Qd: one product with Q per iteration (the curvature pass), and
// with refresh_every = 0 the gradient follows g + t Q d -- the objective itself evaluates the start, and the point at which the run wants to stop.
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

    const Floating tol = 1e-8;
    auto exact = ExactQuadratic::new_(0);
    auto cg = NonlinearCG::new_(tol, x0).with_variant(NonlinearCG::Variant::FR);
    Result r = cg.minimize(exact, objective, 2000, 0);
    if (r.is_err()) { std::printf("optimization failed: %s\n", r.unwrap_err().what()); return 1; }
    const ExactState st = cg.exact_state();
    const auto eval = objective(cg.x());
    Floating ginf = 0.0;
    for (Floating v : eval.g()) ginf = std::fmax(ginf, std::fabs(v));
    // the curvature pass on its own: v'Qv of the solution is b'x at the minimiser (Q x = b)
    const auto qx = objective.hess_vec(cg.x());
    Floating bx = 0.0;
    for (Floating v : cg.x()) bx += v;
    std::printf("n: %d nnz: %zu\niterations: %zu curvature_passes: %zu refreshes: %zu\n||g||_inf: %.3e x'Qx: %.12e b'x: %.12e\n", n, objective.nnz(), cg.k(),
                st.curvature_passes, st.refreshes, ginf, qx.second, bx);
    if (!(ginf < tol) || st.curvature_passes != cg.k() || st.refreshes < 1 || std::fabs(qx.second - bx) > 1e-6 * std::fabs(bx)) {
        std::printf("not at the minimum\n");
        return 1;
    }
    std::printf("exact cg example ok\n");
    return 0;
}
