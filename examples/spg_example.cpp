// examples/spg_example.cpp -- the problem of the reference's examples/spg_example.rs through the C++ host mirror (qn_solver.hpp):
// SpectralProjectedGradient + BackTracking on f(x, y) = x^2 + y^2 + exp(x^2 + y^2) in the box [-1, 1]^2 from (0.5, 0.5); the
// minimum is (0, 0) with f = 1.  A second run pairs the solver with GLLQuadratic, the search it is meant for (spg.rs:6).
#include <cmath>
#include <cstdio>

#include "qn_solver.hpp"

using namespace optimization_solvers;

int main() {
    auto f_and_g = [](const DVector& v) -> FuncEvalMultivariate {
        const Floating r2 = v[0] * v[0] + v[1] * v[1];
        const Floating e = std::exp(r2);
        return FuncEvalMultivariate(r2 + e, {2.0 * v[0] * (1.0 + e), 2.0 * v[1] * (1.0 + e)});
    };
    const Floating tol = 1e-6;
    const DVector x0 = {0.5, 0.5}, lower_bound = {-1.0, -1.0}, upper_bound = {1.0, 1.0};
    const size_t max_iter_solver = 100, max_iter_line_search = 20;

    auto bt = BackTracking::new_(1e-4, 0.5);
    auto solver = SpectralProjectedGradient::new_(tol, x0, f_and_g, lower_bound, upper_bound);
    std::printf("lambda0: %g\n", solver.lambda());
    Result r = solver.minimize(bt, f_and_g, max_iter_solver, max_iter_line_search, std::nullopt);
    if (r.is_err()) { std::printf("optimization failed: %s\n", r.unwrap_err().what()); return 1; }
    const DVector x = solver.x();
    const auto eval = f_and_g(x);
    std::printf("x: [%g, %g]\nf(x): %.6f\niterations: %zu\n", x[0], x[1], eval.f(), solver.k());
    for (size_t i = 0; i < x.size(); ++i)
        if (x[i] < lower_bound[i] || x[i] > upper_bound[i]) { std::printf("constraint %zu violated\n", i); return 1; }
    if (!solver.has_converged(eval) || std::hypot(x[0], x[1]) > 1e-5 || std::fabs(eval.f() - 1.0) > 1e-9) { std::printf("not at the minimum\n"); return 1; }

    auto gll = GLLQuadratic::new_(1e-4, 10);
    auto solver2 = SpectralProjectedGradient::new_(tol, x0, f_and_g, lower_bound, upper_bound);
    solver2.minimize(gll, f_and_g, max_iter_solver, max_iter_line_search, std::nullopt).unwrap();
    if (!solver2.has_converged(f_and_g(solver2.x()))) { std::printf("GLLQuadratic run did not converge\n"); return 1; }
    std::printf("GLLQuadratic: iterations: %zu\n", solver2.k());

    // the same box through ProjectedGradientDescent + BackTrackingB (projected_gradient_descent.rs)
    BackTrackingB btb(1e-4, 0.5, lower_bound, upper_bound);
    auto pgd = ProjectedGradientDescent::new_(tol, x0, lower_bound, upper_bound);
    pgd.minimize(btb, f_and_g, 1000, max_iter_line_search, std::nullopt).unwrap();
    if (!pgd.has_converged(f_and_g(pgd.x()))) { std::printf("projected gradient run did not converge\n"); return 1; }
    std::printf("ProjectedGradientDescent: iterations: %zu\nspg example ok\n", pgd.k());
    return 0;
}
