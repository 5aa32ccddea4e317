// examples/pnorm_example.cpp -- the reference's own test `pnorm_morethuente` (steepest_descent/pnorm_descent.rs:92-140) through the C++ host mirror
// (qn_solver.hpp): PnormDescent + MoreThuente on f(x) = 1/2 (x0^2 + gamma x1^2), gamma = 90, from (180, 152), inverse_p = diag(1, 1/gamma), tol 1e-12;
// then `coordinate_descent_morethuente` (coordinate_descent.rs:102-148) and a pure step x + d with NoSearch.  It asserts what the reference
// asserts: |f| < 1e-6 at the final iterate.
#include <cmath>
#include <cstdio>

#include "qn_solver.hpp"

using namespace optimization_solvers;

int main() {
    const Floating gamma = 90.0;
    auto f_and_g = [gamma](const DVector& x) -> FuncEvalMultivariate {
        const Floating f = 0.5 * (x[0] * x[0] + gamma * x[1] * x[1]);
        return FuncEvalMultivariate(f, {x[0], gamma * x[1]});
    };
    const DVector inv_hessian = {1.0, 0.0, 0.0, 1.0 / gamma}; // DMatrix::from_iterator(2, 2, ..): column-major
    const Floating tol = 1e-12;
    const DVector x0 = {180.0, 152.0};
    const size_t max_iter_solver = 1000, max_iter_line_search = 100;

    auto ls = MoreThuente::default_();
    auto gd = PnormDescent::new_(tol, x0, inv_hessian);
    Result r = gd.minimize(ls, f_and_g, max_iter_solver, max_iter_line_search, std::nullopt);
    if (r.is_err()) { std::printf("optimization failed: %s\n", r.unwrap_err().what()); return 1; }
    const DVector x = gd.xk();
    const auto eval = f_and_g(x);
    std::printf("Iterate: [%.15g, %.15g]\nFunction eval: %.3e\niterations: %zu\nConvergence: %s\n", x[0], x[1], eval.f(), gd.k(),
                gd.has_converged(eval) ? "true" : "false");
    if (!(std::fabs(eval.f() - 0.0) < 1e-6)) { std::printf("not at the minimum\n"); return 1; }
    std::printf("|f| < 1e-6\n");
    if (gd.inverse_p() != inv_hessian) { std::printf("inverse_p does not round-trip\n"); return 1; }

    auto ls2 = MoreThuente::default_();
    auto sdl1 = CoordinateDescent::new_(tol, x0);
    sdl1.minimize(ls2, f_and_g, max_iter_solver, max_iter_line_search, std::nullopt).unwrap();
    const auto eval_cd = f_and_g(sdl1.xk());
    std::printf("CoordinateDescent: iterations: %zu  f: %.3e\n", sdl1.k(), eval_cd.f());
    if (!(std::fabs(eval_cd.f()) < 1e-6)) { std::printf("CoordinateDescent not at the minimum\n"); return 1; }

    NoSearch none; // with inverse_p the inverse Hessian of a quadratic, x + d is the Newton step: one iteration reaches the minimum
    auto full = PnormDescent::new_(tol, x0, inv_hessian);
    full.minimize(none, f_and_g, max_iter_solver, max_iter_line_search, std::nullopt).unwrap();
    std::printf("PnormDescent + NoSearch: iterations: %zu  f: %.3e\n", full.k(), f_and_g(full.xk()).f());
    if (full.k() != 1 || !(std::fabs(f_and_g(full.xk()).f()) < 1e-6)) { std::printf("NoSearch did not take the full step\n"); return 1; }
    std::printf("pnorm example ok\n");
    return 0;
}
