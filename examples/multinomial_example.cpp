// examples/multinomial_example.cpp -- softmax regression through the C++ host mirror (qn_solver.hpp): NewtonCG + BackTracking(1e-4, 0.5) on the device
// Multinomial objective, f = sum_i w_i (logsumexp_k a_i.W_k - a_i.W_{y_i}) + mu/2 ||x||^2 with m = 257 rows, n = 40 columns and K = 5 classes (entries
// from a fixed linear congruence in [-1, 1), scaled to unit variance; labels the argmax of a planted W plus noise; every seventh row masked by a weight
// of 0; mu = 0.5), to ||g||_inf < 1e-7.  The parameter vector is class-major, x[k n + j] = W[k, j], N = 200 entries.  One evaluation is two launches
// and one stream of A for all five classes; P costs one pass of A per outer iteration, each inner conjugate-gradient step one more.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "qn_solver.hpp"

using namespace optimization_solvers;

int main() {
    const size_t m = 257, n = 40, K = 5, N = K * n;
    unsigned long long state = 2029;
    auto next = [&state]() { state = state * 6364136223846793005ULL + 1442695040888963407ULL; return ((Floating)(state >> 11) / 9007199254740992.0 * 2.0 - 1.0) * std::sqrt(3.0); };
    DVector a(m * n), w(m), ws(N), x0(N);
    std::vector<int32_t> y(m);
    for (auto& v : a) v = next();
    for (auto& v : ws) v = next();
    for (auto& v : x0) v = next();
    for (size_t i = 0; i < m; ++i) {
        Floating best = -INFINITY;
        for (size_t k = 0; k < K; ++k) {
            Floating z = 0.5 * next(); // the planted margin plus noise
            for (size_t j = 0; j < n; ++j) z += a[i * n + j] * ws[k * n + j];
            if (z > best) { best = z; y[i] = (int32_t)k; }
        }
        w[i] = i % 7 == 3 ? 0.0 : (i % 3 == 0 ? 3.0 : 1.0);
    }
    Multinomial objective(a, y, n, K, 0.5, w);

    const Floating tol = 1e-7;
    auto ls = BackTracking::new_(1e-4, 0.5);
    auto solver = NewtonCG::new_(tol, x0); // eta_max = 0.5, max_inner = min(N, 100), 8 inner steps per batch
    Result r = solver.minimize(ls, objective, 60, 30);
    if (r.is_err()) { std::printf("optimization failed: %s\n", r.unwrap_err().what()); return 1; }
    const auto eval = objective(solver.x());
    Floating ginf = 0.0;
    for (Floating v : eval.g()) ginf = std::fmax(ginf, std::fabs(v));
    std::printf("NewtonCG on Multinomial (%zu x %zu, %zu classes): outer iterations: %zu inner steps: %zu (last direction: %zu) products: %zu f: %.12e ||g||_inf: %.3e\n",
                m, n, K, solver.k(), solver.inner_total(), solver.inner_last(), solver.hv_passes(), eval.f(), ginf);
    if (!(ginf < tol) || !solver.has_converged(eval) || solver.hv_passes() != solver.inner_total() || solver.negative_curvature() != 0) {
        std::printf("not at the minimum\n");
        return 1;
    }
    // the product on its own at the minimiser: v'Hv >= mu v'v for any v (the data part of H is positive semidefinite)
    const auto hv = objective.hess_vec_at(solver.x(), x0);
    Floating vv = 0.0;
    for (Floating v : x0) vv += v * v;
    if (!(hv.second > 0.5 * vv)) { std::printf("v'Hv = %g is not above mu v'v = %g\n", hv.second, 0.5 * vv); return 1; }
    std::printf("multinomial example ok\n");
    return 0;
}
