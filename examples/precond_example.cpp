// examples/precond_example.cpp -- NewtonCG's Jacobi preconditioner through the C++ host mirror (qn_solver.hpp): logistic regression on a BADLY SCALED
// design matrix, m = 257 rows and n = 200 columns, column j of a unit-variance A (entries from a fixed linear congruence) multiplied by 10^u_j with
// u_j uniform in [-1.5, 1.5): counts next to indicators.  Unit weights, mu = 1e-3, x0 = 0, BackTracking(1e-4, 0.5) to ||g||_inf < 1e-7, once with plain
// conjugate gradients in the inner loop and once with QN_PRECOND_JACOBI: the diagonal of H(x_k), one more stream of A per outer iteration (about the
// price of one inner step), for an inner loop that needs a fraction of the steps.  On well-scaled columns the same switch buys nothing.
#include <cmath>
#include <cstdio>

#include "qn_solver.hpp"

using namespace optimization_solvers;

int main() {
    const size_t m = 257, n = 200;
    unsigned long long state = 2033;
    auto next = [&state]() { state = state * 6364136223846793005ULL + 1442695040888963407ULL; return ((Floating)(state >> 11) / 9007199254740992.0 * 2.0 - 1.0) * std::sqrt(3.0); };
    DVector a(m * n), y(m), xs(n), scale(n), x0(n, 0.0);
    for (auto& v : a) v = next();
    for (auto& v : xs) v = next() / std::sqrt((Floating)n);
    for (auto& v : scale) v = std::pow(10.0, 1.5 * next() / std::sqrt(3.0));
    for (size_t i = 0; i < m; ++i) {
        Floating z = 0.3 * next(); // the planted margin on the unscaled columns, plus noise
        for (size_t j = 0; j < n; ++j) z += a[i * n + j] * xs[j];
        y[i] = z >= 0 ? 1.0 : -1.0;
        for (size_t j = 0; j < n; ++j) a[i * n + j] *= scale[j];
    }
    const Floating mu = 1e-3, tol = 1e-7;
    Logistic objective(a, y, n, mu);

    size_t inner[2] = {0, 0};
    for (int kind : {QN_PRECOND_NONE, QN_PRECOND_JACOBI}) {
        auto ls = BackTracking::new_(1e-4, 0.5);
        auto solver = NewtonCG::new_(tol, x0);
        solver.set_preconditioner(kind);
        Result r = solver.minimize(ls, objective, 100, 30);
        if (r.is_err()) { std::printf("optimization failed: %s\n", r.unwrap_err().what()); return 1; }
        const auto eval = objective(solver.x());
        Floating ginf = 0.0;
        for (Floating v : eval.g()) ginf = std::fmax(ginf, std::fabs(v));
        std::printf("NewtonCG (%s) on a scaled Logistic (%zu x %zu): outer iterations: %zu inner steps: %zu diagonal passes: %zu f: %.12e ||g||_inf: %.3e\n",
                    kind == QN_PRECOND_JACOBI ? "jacobi" : "none", m, n, solver.k(), solver.inner_total(), solver.diag_passes(), eval.f(), ginf);
        if (!(ginf < tol) || solver.preconditioner() != kind || solver.diag_passes() != (kind == QN_PRECOND_JACOBI ? solver.k() : 0) || solver.diag_floored() != 0) {
            std::printf("not at the minimum, or the counters are off\n");
            return 1;
        }
        inner[kind] = solver.inner_total();
        if (kind == QN_PRECOND_JACOBI) { // the diagonal on its own at the minimiser: M_j >= mu (H = A' diag(d) A + mu I, d >= 0)
            const DVector diag = objective.hess_diag_at(solver.x());
            for (Floating v : diag)
                if (!(v >= mu)) { std::printf("H_jj = %g is below mu\n", v); return 1; }
        }
    }
    if (!(2 * inner[1] <= inner[0])) { std::printf("Jacobi took %zu inner steps, plain %zu: not half\n", inner[1], inner[0]); return 1; }
    std::printf("precond example ok\n");
    return 0;
}
