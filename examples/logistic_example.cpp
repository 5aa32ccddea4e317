// examples/logistic_example.cpp -- regularised logistic regression through the C++ host mirror (qn_solver.hpp): NewtonCG + BackTracking(1e-4, 0.5) on the
// device Logistic objective, f = sum_i w_i log(1 + exp(-y_i a_i'x)) + mu/2 ||x||^2 with m = 257 rows and n = 200 columns (entries from a fixed linear
// congruence in [-1, 1), scaled to unit variance; labels from a planted x* plus noise; every seventh row masked by a weight of 0; mu = 0.5), to
// ||g||_inf < 1e-7.  One evaluation is two launches; the Hessian weights d_i = w_i s_i (1 - s_i) cost one pass of A per outer iteration, each inner
// conjugate-gradient step one more -- never the 200 x 200 matrix, and no vector crosses the bus inside the run.
#include <cmath>
#include <cstdio>

#include "qn_solver.hpp"

using namespace optimization_solvers;

int main() {
    const size_t m = 257, n = 200;
    unsigned long long state = 2027;
    auto next = [&state]() { state = state * 6364136223846793005ULL + 1442695040888963407ULL; return ((Floating)(state >> 11) / 9007199254740992.0 * 2.0 - 1.0) * std::sqrt(3.0); };
    DVector a(m * n), y(m), w(m), xs(n), x0(n);
    for (auto& v : a) v = next();
    for (auto& v : xs) v = next() / std::sqrt((Floating)n);
    for (auto& v : x0) v = next();
    for (size_t i = 0; i < m; ++i) {
        Floating z = 0.5 * next(); // the planted margin plus noise
        for (size_t j = 0; j < n; ++j) z += a[i * n + j] * xs[j];
        y[i] = z >= 0 ? 1.0 : -1.0;
        w[i] = i % 7 == 3 ? 0.0 : (i % 3 == 0 ? 3.0 : 1.0);
    }
    Logistic objective(a, y, n, 0.5, w);

    const Floating tol = 1e-7;
    auto ls = BackTracking::new_(1e-4, 0.5);
    auto solver = NewtonCG::new_(tol, x0); // eta_max = 0.5, max_inner = min(n, 100), 8 inner steps per batch
    Result r = solver.minimize(ls, objective, 60, 30);
    if (r.is_err()) { std::printf("optimization failed: %s\n", r.unwrap_err().what()); return 1; }
    const auto eval = objective(solver.x());
    Floating ginf = 0.0;
    for (Floating v : eval.g()) ginf = std::fmax(ginf, std::fabs(v));
    std::printf("NewtonCG on Logistic (%zu x %zu): outer iterations: %zu inner steps: %zu (last direction: %zu) products: %zu f: %.12e ||g||_inf: %.3e\n",
                m, n, solver.k(), solver.inner_total(), solver.inner_last(), solver.hv_passes(), eval.f(), ginf);
    if (!(ginf < tol) || !solver.has_converged(eval) || solver.hv_passes() != solver.inner_total() || solver.negative_curvature() != 0) {
        std::printf("not at the minimum\n");
        return 1;
    }
    // the product on its own at the minimiser: v'Hv >= mu v'v for any v (H = A' diag(d) A + mu I, d >= 0)
    const auto hv = objective.hess_vec_at(solver.x(), x0);
    Floating vv = 0.0;
    for (Floating v : x0) vv += v * v;
    if (!(hv.second > 0.5 * vv)) { std::printf("v'Hv = %g is not above mu v'v = %g\n", hv.second, 0.5 * vv); return 1; }
    std::printf("logistic example ok\n");
    return 0;
}
