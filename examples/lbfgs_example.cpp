// examples/lbfgs_example.cpp -- limited-memory BFGS through the C++ host mirror (qn_solver.hpp), in the style of spg_example.cpp: the
// ill-conditioned quadratic f(x, y) = 1/2 (x^2 + gamma y^2), gamma = 90, from (180, 152) with BackTracking; the minimum is (0, 0) with f = 0.
// A second run puts the same function into a box whose lower face y >= 47 is active at the solution (ProjectedLBFGS + BackTrackingB).
#include <cmath>
#include <cstdio>

#include "qn_solver.hpp"

using namespace optimization_solvers;

int main() {
    const Floating gamma = 90.0;
    auto f_and_g = [gamma](const DVector& v) -> FuncEvalMultivariate {
        return FuncEvalMultivariate(0.5 * (v[0] * v[0] + gamma * v[1] * v[1]), {v[0], gamma * v[1]});
    };
    const Floating tol = 1e-8;
    const DVector x0 = {180.0, 152.0};
    const size_t max_iter_solver = 1000, max_iter_line_search = 100;

    auto bt = BackTracking::new_(1e-4, 0.5);
    auto solver = LBFGS::new_(tol, x0).with_memory(5);
    Result r = solver.minimize(bt, f_and_g, max_iter_solver, max_iter_line_search, std::nullopt);
    if (r.is_err()) { std::printf("optimization failed: %s\n", r.unwrap_err().what()); return 1; }
    const DVector x = solver.x();
    const auto eval = f_and_g(x);
    std::printf("x: [%g, %g]\nf(x): %.3e\niterations: %zu\nstored pairs: %zu of %zu, gamma: %g, resets: %zu\n", x[0], x[1], eval.f(), solver.k(),
                solver.stored_pairs(), solver.memory(), solver.gamma(), solver.resets());
    if (!solver.has_converged(eval) || !(std::fabs(eval.f()) < 1e-6)) { std::printf("not at the minimum\n"); return 1; }
    std::printf("LBFGS + BackTracking: |f| < 1e-6\n");

    const DVector lower_bound = {-1.0, 47.0}, upper_bound = {INFINITY, INFINITY};
    BackTrackingB btb(1e-4, 0.5, lower_bound, upper_bound);
    auto boxed = ProjectedLBFGS::new_(tol, x0, lower_bound, upper_bound).with_memory(3);
    boxed.minimize(btb, f_and_g, max_iter_solver, max_iter_line_search, std::nullopt).unwrap();
    const DVector xb = boxed.x();
    if (!boxed.has_converged(f_and_g(xb)) || xb[1] != 47.0 || std::fabs(xb[0]) > 1e-6) { std::printf("boxed run is not at the constrained minimum\n"); return 1; }
    std::printf("ProjectedLBFGS + BackTrackingB: x: [%g, %g] iterations: %zu\nlbfgs example ok\n", xb[0], xb[1], boxed.k());
    return 0;
}
