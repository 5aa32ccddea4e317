// examples/pnewton_example.cpp -- the second-order box-constrained pair through the C++ host mirror (qn_solver.hpp): ProjectedNewton and
// SpectralProjectedNewton + GLLQuadratic on f(x, y) = 1/2 (x^2 + gamma y^2), whose closure hands over its Hessian with the evaluation
// (FuncEvalMultivariate::with_hessian).  Free, the minimum is (0, 0); in the box x >= -1, y >= 47 it is (0, 47).
#include <cmath>
#include <cstdio>
#include <limits>

#include "qn_solver.hpp"

using namespace optimization_solvers;

int main() {
    const Floating gamma = 90.0, inf = std::numeric_limits<Floating>::infinity();
    auto f_g_h = [gamma](const DVector& v) -> FuncEvalMultivariate {
        return FuncEvalMultivariate(0.5 * (v[0] * v[0] + gamma * v[1] * v[1]), {v[0], gamma * v[1]}).with_hessian({1.0, 0.0, 0.0, gamma});
    };
    const DVector x0 = {180.0, 152.0};
    const size_t max_iter_solver = 10000, max_iter_line_search = 1000;

    auto gll = GLLQuadratic::new_(1e-4, 15);
    auto pn = ProjectedNewton::new_(1e-6, x0, {-inf, -inf}, {inf, inf});
    Result r = pn.minimize(gll, f_g_h, max_iter_solver, max_iter_line_search, std::nullopt);
    if (r.is_err()) { std::printf("optimization failed: %s\n", r.unwrap_err().what()); return 1; }
    DVector x = pn.x();
    std::printf("ProjectedNewton: x: [%g, %g] iterations: %zu\n", x[0], x[1], pn.k());
    if (!pn.has_converged(f_g_h(x)) || std::hypot(x[0], x[1]) > 1e-6) { std::printf("not at the minimum\n"); return 1; }

    const DVector lower_bound = {-1.0, 47.0}, upper_bound = {inf, inf};
    auto gll2 = GLLQuadratic::new_(1e-4, 10);
    auto spn = SpectralProjectedNewton::new_(1e-12, x0, f_g_h, lower_bound, upper_bound);
    std::printf("lambda0: %g\n", spn.lambda());
    spn.minimize(gll2, f_g_h, max_iter_solver, max_iter_line_search, std::nullopt).unwrap();
    x = spn.x();
    std::printf("SpectralProjectedNewton: x: [%g, %g] iterations: %zu\n", x[0], x[1], spn.k());
    for (size_t i = 0; i < x.size(); ++i)
        if (x[i] < lower_bound[i] || x[i] > upper_bound[i]) { std::printf("constraint %zu violated\n", i); return 1; }
    if (!spn.has_converged(f_g_h(x)) || std::fabs(x[0]) > 1e-9 || x[1] != 47.0) { std::printf("not at the minimum\n"); return 1; }
    std::printf("pnewton example ok\n");
    return 0;
}
