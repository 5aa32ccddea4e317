// examples/broyden_example.cpp -- the reference's own test `broyden_morethuente` (quasi_newton/broyden.rs:135-184) through the C++ host mirror
// (qn_solver.hpp): Broyden + MoreThuente on f(x) = 1/2 ((x0 + 1)^2 + gamma (x1 - 1)^2) from (180, 152), tol 1e-12; then `broyden_b_backtracking`
// (broyden_b.rs) -- BroydenB + BackTrackingB with an infinite box.  Both assert what the reference asserts: f < 1e-6 at the final iterate.
#include <cmath>
#include <cstdio>

#include "qn_solver.hpp"

using namespace optimization_solvers;

int main() {
    const Floating gamma = 1.0;
    auto f_and_g = [gamma](const DVector& x) -> FuncEvalMultivariate {
        const Floating f = 0.5 * ((x[0] + 1.0) * (x[0] + 1.0) + gamma * (x[1] - 1.0) * (x[1] - 1.0));
        return FuncEvalMultivariate(f, {x[0] + 1.0, gamma * (x[1] - 1.0)});
    };
    const Floating tol = 1e-12;
    const DVector x0 = {180.0, 152.0};
    const size_t max_iter_solver = 1000, max_iter_line_search = 100000;

    auto ls = MoreThuente::default_();
    auto solver = Broyden::new_(tol, x0);
    Result r = solver.minimize(ls, f_and_g, max_iter_solver, max_iter_line_search, std::nullopt);
    if (r.is_err()) { std::printf("optimization failed: %s\n", r.unwrap_err().what()); return 1; }
    const DVector x = solver.x();
    const auto eval = f_and_g(x);
    std::printf("Iterate: [%.15g, %.15g]\nFunction eval: %.3e\niterations: %zu\nConvergence: %s\n", x[0], x[1], eval.f(), solver.k(),
                solver.has_converged(eval) ? "true" : "false");
    if (!(std::fabs(eval.f() - 0.0) < 1e-6) || !solver.has_converged(eval)) { std::printf("not at the minimum\n"); return 1; }

    const DVector lower_bound = {-INFINITY, -INFINITY}, upper_bound = {INFINITY, INFINITY};
    BackTrackingB btb(1e-4, 0.5, lower_bound, upper_bound);
    auto bounded = BroydenB::new_(tol, x0, lower_bound, upper_bound);
    bounded.minimize(btb, f_and_g, max_iter_solver, max_iter_line_search, std::nullopt).unwrap();
    const auto eval_b = f_and_g(bounded.x());
    std::printf("BroydenB: iterations: %zu  f: %.3e\n", bounded.k(), eval_b.f());
    if (!(std::fabs(eval_b.f()) < 1e-6)) { std::printf("BroydenB not at the minimum\n"); return 1; }
    std::printf("broyden example ok\n");
    return 0;
}
