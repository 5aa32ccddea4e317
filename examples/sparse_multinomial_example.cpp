// examples/sparse_multinomial_example.cpp -- sparse softmax regression through the C++ host mirror (qn_solver.hpp): NewtonCG + BackTracking(1e-4, 0.5)
// on the device SparseMultinomial objective, f = sum_i w_i (logsumexp_k a_i.W_k - a_i.W_{y_i}) + mu/2 ||x||^2 with m = 400 samples, n = 20000 features
// and K = 12 classes: N = K n = 240 000 parameters, class-major -- far beyond the dense Multinomial's padded K n <= 16384.  Every row has an intercept
// entry of 1 in column 0 and 8 more nonzeros in distinct columns drawn by a fixed linear congruence (values in [-1, 1) scaled to unit variance); labels
// the argmax of a planted W plus noise; every seventh row masked by a weight of 0; mu = 0.5; to ||g||_inf < 1e-7.  The device keeps A and A': the
// intercept column is a row of 400 entries of A'.  No vector crosses the bus inside the run.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "qn_solver.hpp"

using namespace optimization_solvers;

int main() {
    const size_t m = 400, n = 20000, K = 12, N = K * n, per_row = 8;
    unsigned long long state = 2031;
    auto next_u = [&state]() { state = state * 6364136223846793005ULL + 1442695040888963407ULL; return state >> 11; };
    auto next = [&next_u]() { return ((Floating)next_u() / 9007199254740992.0 * 2.0 - 1.0) * std::sqrt(3.0); };
    DVector ws(N), x0(N, 0.0), w(m), data;
    for (auto& v : ws) v = next();
    std::vector<int32_t> indptr(1, 0), indices, y(m);
    for (size_t i = 0; i < m; ++i) {
        std::vector<int32_t> cols;
        while (cols.size() < per_row) {
            const int32_t c = 1 + (int32_t)(next_u() % (n - 1));
            if (std::find(cols.begin(), cols.end(), c) == cols.end()) cols.push_back(c);
        }
        std::sort(cols.begin(), cols.end());
        DVector vals(per_row);
        for (auto& v : vals) v = next();
        indices.push_back(0);
        data.push_back(1.0);
        for (size_t e = 0; e < per_row; ++e) { indices.push_back(cols[e]); data.push_back(vals[e]); }
        indptr.push_back((int32_t)indices.size());
        Floating best = -INFINITY;
        for (size_t k = 0; k < K; ++k) {
            Floating z = ws[k * n] + 0.5 * next(); // the intercept, plus noise
            for (size_t e = 0; e < per_row; ++e) z += vals[e] * ws[k * n + (size_t)cols[e]];
            if (z > best) { best = z; y[i] = (int32_t)k; }
        }
        w[i] = i % 7 == 3 ? 0.0 : (i % 3 == 0 ? 3.0 : 1.0);
    }
    SparseMultinomial objective(indptr, indices, data, y, n, K, 0.5, w);
    if (objective.nnz() != m * (per_row + 1) || objective.size() != N || objective.kp() != 16) {
        std::printf("nnz = %zu, N = %zu, Kp = %d\n", objective.nnz(), objective.size(), objective.kp());
        return 1;
    }

    const Floating tol = 1e-7;
    auto ls = BackTracking::new_(1e-4, 0.5);
    auto solver = NewtonCG::new_(tol, x0); // eta_max = 0.5, max_inner = min(N, 100), 8 inner steps per batch
    Result r = solver.minimize(ls, objective, 60, 30);
    if (r.is_err()) { std::printf("optimization failed: %s\n", r.unwrap_err().what()); return 1; }
    const auto eval = objective(solver.x());
    Floating ginf = 0.0;
    for (Floating v : eval.g()) ginf = std::fmax(ginf, std::fabs(v));
    std::printf("NewtonCG on SparseMultinomial (%zu x %zu, %zu classes, %zu nonzeros): outer iterations: %zu inner steps: %zu (last direction: %zu) products: %zu f: %.12e ||g||_inf: %.3e\n",
                m, n, K, objective.nnz(), solver.k(), solver.inner_total(), solver.inner_last(), solver.hv_passes(), eval.f(), ginf);
    if (!(ginf < tol) || solver.hv_passes() != solver.inner_total() || solver.negative_curvature() != 0) {
        std::printf("not at the minimum\n");
        return 1;
    }
    // the probabilities at the minimiser: every live row's sum to 1, the masked rows' are zeros
    const DVector p = objective.probabilities(solver.x());
    for (size_t i = 0; i < m; ++i) {
        Floating s = 0.0;
        for (size_t k = 0; k < K; ++k) s += p[i * K + k];
        if (std::fabs(s - (w[i] == 0.0 ? 0.0 : 1.0)) > 1e-14) { std::printf("row %zu: sum p = %.17g\n", i, s); return 1; }
    }
    // the product on its own at the minimiser: v'Hv >= mu v'v for any v (the data part of H is positive semidefinite)
    const auto hv = objective.hess_vec_at(solver.x(), ws);
    Floating vv = 0.0;
    for (Floating v : ws) vv += v * v;
    if (!(hv.second > 0.5 * vv * (1.0 - 1e-12))) { std::printf("v'Hv = %g is not above mu v'v = %g\n", hv.second, 0.5 * vv); return 1; }
    std::printf("sparse multinomial example ok\n");
    return 0;
}
