// examples/wolfe_example.cpp -- the StrongWolfe line search (MINPACK-2 dcsrch) through the C++ host mirror (qn_solver.hpp), on lbfgs_example.cpp's
// problem: f(x, y) = 1/2 (x^2 + gamma y^2), gamma = 90, from (180, 152).  Free LBFGS: the curvature condition keeps s.y > 0, so a pair is committed in
// every iteration.  Then ProjectedLBFGS in a box whose lower face y >= 47 is active at the solution, the search holding the same box: no trial leaves it.
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

    auto sw = StrongWolfe::new_(1e-4, 0.9);
    auto solver = LBFGS::new_(tol, x0).with_memory(5);
    Result r = solver.minimize(sw, f_and_g, max_iter_solver, max_iter_line_search, std::nullopt);
    if (r.is_err()) { std::printf("optimization failed: %s\n", r.unwrap_err().what()); return 1; }
    const auto eval = f_and_g(solver.x());
    std::printf("f(x): %.3e\niterations: %zu\nstored pairs: %zu of %zu, resets: %zu\n", eval.f(), solver.k(), solver.stored_pairs(), solver.memory(), solver.resets());
    if (!solver.has_converged(eval) || !(std::fabs(eval.f()) < 1e-6) || solver.resets() != 0) { std::printf("not at the minimum\n"); return 1; }
    std::printf("LBFGS + StrongWolfe: |f| < 1e-6\n");

    const DVector lower_bound = {-1.0, 47.0}, upper_bound = {INFINITY, INFINITY};
    bool inside = true;
    auto checked = [&](const DVector& v) -> FuncEvalMultivariate {
        if (v[0] < lower_bound[0] || v[1] < lower_bound[1]) inside = false;
        return f_and_g(v);
    };
    auto swb = StrongWolfe::new_(1e-4, 0.9).with_t_max(1e6).with_lower_bound(lower_bound).with_upper_bound(upper_bound);
    auto boxed = ProjectedLBFGS::new_(tol, x0, lower_bound, upper_bound).with_memory(3);
    boxed.minimize(swb, checked, max_iter_solver, max_iter_line_search, std::nullopt).unwrap();
    const DVector xb = boxed.x();
    if (!boxed.has_converged(f_and_g(xb)) || xb[1] != 47.0 || std::fabs(xb[0]) > 1e-6 || !inside || swb.t_max() != 1e6) {
        std::printf("boxed run is not at the constrained minimum\n");
        return 1;
    }
    std::printf("ProjectedLBFGS + StrongWolfe (boxed): x: [%g, %g] iterations: %zu\nwolfe example ok\n", xb[0], xb[1], boxed.k());
    return 0;
}
