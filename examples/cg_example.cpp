// examples/cg_example.cpp -- nonlinear conjugate gradient through the C++ host mirror (qn_solver.hpp): NonlinearCG (Hager-Zhang, then the default
// Polak-Ribiere+) + StrongWolfe(1e-4, 0.1) on the problem of sparse_lbfgs_example.cpp: min 1/2 x'Qx - b'x with Q the 2-D five-point Laplacian of a
// 64 x 64 grid plus a shift of 0.05 (SPD, 20 224 nonzeros in CSR), b = 1.  The matrix lives on the device as CSR and the method keeps ONE vector
// beside the machine's own: no evaluation and no direction crosses the bus.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "qn_solver.hpp"

using namespace optimization_solvers;

static bool at_minimum(const char* name, NonlinearCG& solver, const SparseQuadratic& objective, Floating tol, Floating shift) {
    const auto eval = objective(solver.x());
    Floating ginf = 0.0;
    for (Floating v : eval.g()) ginf = std::fmax(ginf, std::fabs(v));
    std::printf("%s k: %zu f: %.12e ||g||_inf: %.3e restarts: %zu beta: %.3e\n", name, solver.k(), eval.f(), ginf, solver.restarts(), solver.beta());
    // at the minimiser f = -1/2 b'x with Q x = b; the constant vector 1 / shift solves the problem without its boundary, so 0 < x < 1 / shift
    Floating bx = 0.0;
    bool inside = true;
    for (Floating v : solver.x()) { bx += v; inside = inside && v > 0.0 && v < 1.0 / shift; }
    return ginf < tol && solver.has_converged(eval) && inside && std::fabs(eval.f() + 0.5 * bx) <= 1e-6 * std::fabs(eval.f());
}

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
    std::printf("n: %d nnz: %zu\n", n, objective.nnz());

    const Floating tol = 1e-6;
    auto sw = StrongWolfe::new_(1e-4, 0.1);
    auto hz = NonlinearCG::new_(tol, x0).with_variant(NonlinearCG::Variant::HZ);
    Result r = hz.minimize(sw, objective, 1000, 100);
    if (r.is_err()) { std::printf("optimization failed: %s\n", r.unwrap_err().what()); return 1; }
    if (hz.variant() != NonlinearCG::Variant::HZ || !at_minimum("hz ", hz, objective, tol, shift)) { std::printf("not at the minimum\n"); return 1; }

    auto pr = NonlinearCG::new_(tol, x0); // Polak-Ribiere+, powell_nu = 0.2
    r = pr.minimize(sw, objective, 1000, 100);
    if (r.is_err()) { std::printf("optimization failed: %s\n", r.unwrap_err().what()); return 1; }
    if (pr.variant() != NonlinearCG::Variant::PR_PLUS || !at_minimum("pr+", pr, objective, tol, shift)) { std::printf("not at the minimum\n"); return 1; }
    std::printf("cg example ok\n");
    return 0;
}
