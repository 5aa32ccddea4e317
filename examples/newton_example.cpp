// examples/newton_example.cpp -- Newton through the C++ host mirror (qn_solver.hpp): the reference's newton_morethuente test
// (newton/mod.rs:76-119: f(x, y) = 1/2 (x^2 + gamma y^2), gamma = 1222, the closure hands over its Hessian), then Newton on a device-resident
// log-sum-exp objective, whose Hessian the library forms on the GPU at every iterate, beside the same problem as a host closure
// written out in plain C++ (f, g and the analytic Hessian), and LogSumExp::hessian beside that closure's matrix.
#include <cmath>
#include <cstdio>

#include "qn_solver.hpp"

using namespace optimization_solvers;

int main() {
    std::setvbuf(stdout, nullptr, _IOLBF, 0);
    const Floating gamma = 1222.0;
    auto f_g_h = [gamma](const DVector& v) -> FuncEvalMultivariate {
        return FuncEvalMultivariate(0.5 * (v[0] * v[0] + gamma * v[1] * v[1]), {v[0], gamma * v[1]}).with_hessian({1.0, 0.0, 0.0, gamma});
    };
    auto ls = MoreThuente::default_();
    auto nt = Newton::new_(1e-8, {1.0, 1.0});
    Result r = nt.minimize(ls, f_g_h, 1000, 100, std::nullopt);
    if (r.is_err()) { std::printf("optimization failed: %s\n", r.unwrap_err().what()); return 1; }
    DVector x = nt.x();
    std::printf("Newton: x: [%g, %g] iterations: %zu\n", x[0], x[1], nt.k());
    if (!nt.has_converged(f_g_h(x)) || f_g_h(x).f() > 1e-6) { std::printf("not at the minimum\n"); return 1; }

    // log-sum-exp, m = 48 rows, n = 20 columns, entries from a fixed linear congruence in [-1, 1)
    const size_t m = 48, n = 20;
    unsigned long long state = 12345;
    auto next = [&state]() { state = state * 6364136223846793005ULL + 1442695040888963407ULL; return (Floating)(state >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
    DVector a(m * n), c(m), x0(n);
    for (auto& v : a) v = next();
    for (auto& v : c) v = next();
    for (auto& v : x0) v = next();
    LogSumExp objective(a, c, n, 0.5);
    auto dev = Newton::new_(1e-10, x0);
    r = dev.minimize(ls, objective, 50, 20);
    if (r.is_err()) { std::printf("Newton on the device objective failed: %s\n", r.unwrap_err().what()); return 1; }
    // the same problem as a host closure in plain C++: f, g and H = A'(diag(p) - p p')A + mu I (column-major; symmetric)
    auto closure = [&a, &c, m, n](const DVector& v) -> FuncEvalMultivariate {
        DVector z(m), g(n, 0.0), h(n * n, 0.0);
        Floating zmax = -INFINITY, sum = 0, xx = 0;
        for (size_t k = 0; k < m; ++k) {
            z[k] = c[k];
            for (size_t j = 0; j < n; ++j) z[k] += a[k * n + j] * v[j];
            zmax = std::fmax(zmax, z[k]);
        }
        for (size_t k = 0; k < m; ++k) { z[k] = std::exp(z[k] - zmax); sum += z[k]; }
        for (size_t k = 0; k < m; ++k) {
            const Floating p = z[k] / sum;
            for (size_t j = 0; j < n; ++j) {
                g[j] += p * a[k * n + j];
                for (size_t i = 0; i < n; ++i) h[i + j * n] += p * a[k * n + i] * a[k * n + j];
            }
        }
        for (size_t j = 0; j < n; ++j)
            for (size_t i = 0; i < n; ++i) h[i + j * n] += (i == j ? 0.5 : 0.0) - g[i] * g[j];
        for (size_t j = 0; j < n; ++j) { xx += v[j] * v[j]; g[j] += 0.5 * v[j]; }
        return FuncEvalMultivariate(zmax + std::log(sum) + 0.25 * xx, std::move(g)).with_hessian(std::move(h));
    };
    auto host = Newton::new_(1e-10, x0);
    r = host.minimize(ls, closure, 50, 20, std::nullopt);
    if (r.is_err()) { std::printf("Newton on the host closure failed: %s\n", r.unwrap_err().what()); return 1; }
    const DVector xd = dev.x(), xh = host.x();
    const FuncEvalMultivariate ev = objective(xd);
    const DVector hd = objective.hessian(xd);
    const FuncEvalMultivariate evh = closure(xd);
    Floating dist = 0, gmax = 0, hdiff = 0;
    for (size_t i = 0; i < n; ++i) dist = std::fmax(dist, std::fabs(xd[i] - xh[i]));
    for (Floating v : ev.g()) gmax = std::fmax(gmax, std::fabs(v));
    for (size_t i = 0; i < n * n; ++i) hdiff = std::fmax(hdiff, std::fabs(hd[i] - (*evh.hessian())[i]));
    std::printf("Newton on LogSumExp: iterations: %zu (host closure: %zu) |g|_inf: %g max |x_dev - x_host|: %g max |H_dev - H_host|: %g\n",
                dev.k(), host.k(), gmax, dist, hdiff);
    // (the two runs go in lock step and differ by rounding only; entries of H are O(1) sums of 48 terms)
    if (!dev.has_converged(ev) || dev.k() != host.k() || dev.k() < 2 || gmax > 1e-4 || dist > 1e-9 || hdiff > 1e-12) { std::printf("runs disagree\n"); return 1; }
    std::printf("newton example ok\n");
    return 0;
}
