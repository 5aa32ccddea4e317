// examples/owlqn_example.cpp -- L1-regularised logistic regression through the C++ host mirror (qn_solver.hpp): OWLQN(m = 5) + BackTracking(1e-4, 0.5)
// on the device Logistic objective, F = sum_i w_i log(1 + exp(-y_i a_i'x)) + mu/2 ||x||^2 + l1 sum_{j >= 1} |x_j| with m = 257 rows and n = 200 columns
// (lasso_example.cpp's data; mu = 1e-3).  Column 0 is the intercept's and carries no penalty.  The run goes to 1e-5 at l1 = 4, then the SAME solver
// continues at l1 = 2 -- the regularisation-path use: the pairs (differences of the smooth gradient), x and the memoised evaluation are kept, and
// stored_pairs() is printed across the change.  The weights the orthant projection switches off are exactly 0.0.
#include <cmath>
#include <cstdio>

#include "qn_solver.hpp"

using namespace optimization_solvers;

int main() {
    const size_t m = 257, n = 200;
    unsigned long long state = 2027;
    auto next = [&state]() { state = state * 6364136223846793005ULL + 1442695040888963407ULL; return ((Floating)(state >> 11) / 9007199254740992.0 * 2.0 - 1.0) * std::sqrt(3.0); };
    DVector a(m * n), y(m), w(m), xs(n), x0(n, 0.0);
    for (auto& v : a) v = next();
    for (size_t i = 0; i < m; ++i) a[i * n] = 1.0; // the intercept's column
    for (size_t j = 0; j < n; ++j) xs[j] = j % 5 == 0 ? next() : 0.0; // a sparse planted model
    for (size_t i = 0; i < m; ++i) {
        Floating z = 0.5 * next();
        for (size_t j = 0; j < n; ++j) z += a[i * n + j] * xs[j];
        y[i] = z >= 0 ? 1.0 : -1.0;
        w[i] = i % 7 == 3 ? 0.0 : (i % 3 == 0 ? 3.0 : 1.0);
    }
    Logistic objective(a, y, n, 1e-3, w);

    const Floating tol = 1e-5;
    DVector l1(n, 4.0);
    l1[0] = 0.0;
    auto ls = BackTracking::new_(1e-4, 0.5);
    auto solver = OWLQN::new_(tol, x0, l1);
    Result r = solver.minimize(ls, objective, 2000, 50);
    if (r.is_err()) { std::printf("optimization failed at l1 = 4: %s\n", r.unwrap_err().what()); return 1; }
    auto eval = objective(solver.x());
    const size_t it4 = solver.k(), nz4 = solver.nonzeros(), pairs4 = solver.stored_pairs();
    std::printf("l1 = 4: iterations: %zu nonzeros: %zu of %zu F: %.12e measure: %.3e stored pairs: %zu\n", it4, nz4, n, solver.composite(eval), solver.measure(eval), pairs4);
    if (!solver.has_converged(eval) || nz4 == 0 || nz4 >= n || solver.x()[0] == 0.0) { std::printf("not at a sparse minimum\n"); return 1; }

    for (size_t j = 1; j < n; ++j) l1[j] = 2.0;
    solver.set_l1(l1);
    std::printf("set_l1: stored pairs: %zu\n", solver.stored_pairs());
    if (solver.stored_pairs() != pairs4) { std::printf("the memory did not survive set_l1\n"); return 1; }
    r = solver.minimize(ls, objective, 2000, 50);
    if (r.is_err()) { std::printf("optimization failed at l1 = 2: %s\n", r.unwrap_err().what()); return 1; }
    eval = objective(solver.x());
    const size_t it2 = solver.k(), nz2 = solver.nonzeros();
    std::printf("l1 = 2: iterations: %zu nonzeros: %zu of %zu F: %.12e measure: %.3e stored pairs: %zu\n", it2, nz2, n, solver.composite(eval), solver.measure(eval), solver.stored_pairs());
    if (!solver.has_converged(eval) || nz2 == 0 || nz2 >= n) { std::printf("not at a sparse minimum\n"); return 1; }
    std::printf("owlqn example ok\n");
    return 0;
}
