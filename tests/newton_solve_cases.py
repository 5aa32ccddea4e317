"""The matrices and case lists of the Newton solve tests (tests/test_ref_newton_solve.py licenses them on the CPU, tests/test_gpu_newton_solve.py
runs them through csrc/qn_newton.hip.h, qn_lu.hip.h and qn_lu_split.hip.h).  Pure NumPy, seeded; every matrix is built once and kept.

What is measured is the normwise backward error of one Newton direction x = -(H^-1 g),

    eta(H, x, g) = ||H x + g||_inf / (||H||_inf ||x||_inf + ||g||_inf),

with the residual in extended precision, against B(n) = max(n, 64) 2^-53: the practical form of the bounds for Cholesky and for LU with
partial pivoting (Higham, Accuracy and Stability of Numerical Algorithms, Thms 9.4 and 10.4: of order n gamma_3n times the growth factor).
It is a condition on the kernels, not a measurement of them: LAPACK stays under B(n) / 8 on every case (the licence), a structural error -- a
stale tile, a term dropped from a block inverse, a row swap not replayed -- lands 1e4 and more above it, and eta does not grow with the
condition number, which a forward tolerance does.

Sizes are the smallest that reach each branch of csrc/qn_host_newton.hip.h:
    n <= 5                 newton_small_kernel (family I)
    6                      first blocked size, 58 padding rows
    63, 64, 65             one 64-block, exact multiple, ragged second block
    257                    second outer Cholesky block (KB = 256): the depth-256 trailing update and its fused diagonal step
    512, 513               n64 > 512 switches on the 512-wide block inverses (newton_big); the padding jumps from 512 to 1024
    769                    nblocks >= 4: the Cholesky look-ahead on the second stream
    1100                   three 512-blocks, a bulk update beside the chain
    449                    8 LU panels: the LU look-ahead
    513, 1025, 2049        panel heights past 512, 1024, 2048: 2, 4 and 8 rows per thread of the panel kernels"""
import functools

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
HAVE_LONGDOUBLE = np.finfo(LD).nmant >= 63  # x87 extended (64-bit significand) or better
MPMATH_MAX_N = 257


def bound(n):
    return max(n, 64) * U


# ---- the measure ----
def _residual_mp(H, x, g):
    import mpmath
    with mpmath.workdps(40):
        r = 0.0
        for i in range(len(g)):
            r = max(r, abs(float(mpmath.fsum([mpmath.mpf(float(a)) * mpmath.mpf(float(b)) for a, b in zip(H[i], x)] + [mpmath.mpf(float(g[i]))]))))
    return r


def residual_inf(H, x, g):
    """||H x + g||_inf with products and sums in extended precision (np.longdouble where it has a 64-bit significand, else mpmath up to n = 257)"""
    if HAVE_LONGDOUBLE:
        return float(np.max(np.abs(H.astype(LD) @ np.asarray(x, dtype=LD) + g.astype(LD))))
    if len(g) > MPMATH_MAX_N:
        import pytest
        pytest.skip(f"np.longdouble has a {np.finfo(LD).nmant + 1}-bit significand here and n = {len(g)} > {MPMATH_MAX_N} is too large for the mpmath residual")
    return _residual_mp(H, np.asarray(x, dtype=np.float64), g)


def eta(H, x, g):
    x64 = np.asarray(x, dtype=np.float64)
    den = float(np.max(np.sum(np.abs(H), axis=1))) * float(np.max(np.abs(x64))) + float(np.max(np.abs(g)))
    return residual_inf(H, x, g) / den


def norm_inf(H):
    return float(np.max(np.sum(np.abs(H), axis=1)))


@functools.lru_cache(maxsize=None)
def _inverse(key):
    return np.linalg.inv(matrix(key))


def kappa_inf(key):
    """||H||_inf ||H^-1||_inf (the inverse from LAPACK: good to kappa * 2^-53 relative, used only where kappa_inf * B(n) < 1e-3)"""
    return norm_inf(matrix(key)) * norm_inf(_inverse(key))


def solve_extended(key, d, sweeps=6):
    """H z = d to extended precision: LAPACK's inverse as the preconditioner of an iterative refinement whose residuals are formed in
    np.longdouble (contraction kappa * 2^-53 per sweep: used where that is below 1e-3 / 64).  Returns z as np.longdouble."""
    assert HAVE_LONGDOUBLE
    H = matrix(key).astype(LD)
    inv = _inverse(key)
    dl = np.asarray(d, dtype=LD)
    z = (inv @ np.asarray(d, dtype=np.float64)).astype(LD)
    for _ in range(sweeps):
        r = dl - H @ z
        z = z + (inv @ r.astype(np.float64)).astype(LD)
    return z


# ---- families ----
def _rng(*key):
    return np.random.default_rng([abs(hash_int(k)) for k in key])


def hash_int(k):
    """a stable integer of a key part (no str hash: that one changes from process to process)"""
    if isinstance(k, str):
        return int.from_bytes(k.encode(), "little") % (1 << 61)
    if isinstance(k, float):
        return int(round(np.log2(k) * 1024)) if k > 0 else 0
    return int(k)


def spd(n, kappa):
    """A: H = Q diag(logspace(0, -log10 kappa, n)) Q', symmetrised bit for bit"""
    rng = _rng("spd", n, float(kappa))
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    h = (q * np.logspace(0.0, -np.log10(kappa), n)) @ q.T
    return 0.5 * (h + h.T)


def gaussian(n):
    """C: dense standard normal entries, seed = n: a row swap in nearly every column"""
    return np.random.default_rng(n).standard_normal((n, n))


PERMS = ("reversal", "cyclic", "random")


def permutation(n, kind):
    if kind == "reversal":  # the pivot of column k is the farthest row
        return np.arange(n)[::-1].copy()
    if kind == "cyclic":  # row i holds column i - 1: row 0 is swapped n - 1 times
        return (np.arange(n) - 1) % n
    return _rng("perm", n).permutation(n)


def scaled_permutation(n, kind):
    """D: H[i, p[i]] = sigma_i 2^e_i, sigma = +-1, e in [-20, 20]; returns (H, p, d)"""
    rng = _rng("scaledperm", n, kind)
    p = permutation(n, kind)
    d = rng.choice([-1.0, 1.0], n) * np.exp2(rng.integers(-20, 21, n).astype(np.float64))
    h = np.zeros((n, n))
    h[np.arange(n), p] = d
    return h, p, d


def late_failure(n, c):
    """E: 4 I + 0.5 (S + S'), S = triu(U(-1, 1) / sqrt(n), 1) -- SPD, cond about 1.3 -- with H[c, c] = -4: an unblocked Cholesky meets its first
    non-positive pivot exactly at column c"""
    rng = _rng("late", n)
    s = np.triu(rng.uniform(-1.0, 1.0, (n, n)) / np.sqrt(n), 1)
    h = 4.0 * np.eye(n) + 0.5 * (s + s.T)
    h[c, c] = -4.0
    return h


def small_swapped(n):
    """I (2 <= n <= 5): the dominant entries (+-4) on a cyclic shift, small entries elsewhere, and a zero at H[0, 0]: swaps are required"""
    rng = _rng("small", n)
    h = 0.25 * rng.uniform(-1.0, 1.0, (n, n))
    p = (np.arange(n) + 1) % n
    h[np.arange(n), p] = 4.0 * rng.choice([-1.0, 1.0], n)
    h[0, 0] = 0.0
    return h


@functools.lru_cache(maxsize=None)
def matrix(key):
    """key: ("spd", n, kappa) | ("gauss", n) | ("perm", n, kind) | ("late", n, c) | ("small", n) | ("ulp", n, kappa) | ("scaled", key, exponent)"""
    kind = key[0]
    if kind == "spd":
        h = spd(key[1], key[2])
    elif kind == "gauss":
        h = gaussian(key[1])
    elif kind == "perm":
        h = scaled_permutation(key[1], key[2])[0]
    elif kind == "late":
        h = late_failure(key[1], key[2])
    elif kind == "small":
        h = small_swapped(key[1])
    elif kind == "ulp":  # G: one ulp of asymmetry in the far corner of the lower triangle
        h = spd(key[1], key[2]).copy()
        h[key[1] - 1, 0] = np.nextafter(h[key[1] - 1, 0], np.inf)
    elif kind == "scaled":  # H: a power of two times another case's matrix (exact)
        h = np.ldexp(matrix(key[1]), key[2])
    else:
        raise KeyError(key)
    h.setflags(write=False)
    return h


RHS = ("normal", "range")


@functools.lru_cache(maxsize=None)
def rhs(key, kind="normal"):
    """g of a case: "normal" -- standard normal entries; "range" -- g = -(H x_true), x_true standard normal: g lies in the large
    eigen-directions, where a solve through explicit inverses shows its weakness; "ints" -- integers in [1, 2^20) (family D)"""
    if key[0] == "scaled":
        g = np.ldexp(rhs(key[1], kind), key[2])
    else:
        h = matrix(key)
        n = h.shape[0]
        rng = _rng("rhs", n, kind, *[k for k in key[1:] if not isinstance(k, tuple)])
        if kind == "normal":
            g = rng.standard_normal(n)
        elif kind == "range":
            g = -(h @ rng.standard_normal(n))
        elif kind == "ints":
            g = rng.integers(1, 1 << 20, n).astype(np.float64)
        else:
            raise KeyError(kind)
    g.setflags(write=False)
    return g


def perm_exact(n, kind):
    """D's answer: x[p] = -g / d, exact (a power of two divides an integer below 2^20)"""
    _, p, d = scaled_permutation(n, kind)
    x = np.empty(n)
    x[p] = -rhs(("perm", n, kind), "ints") / d
    return x


# ---- case lists: (matrix key, rhs kind, via, options) ----
LU = (("newton_pivoted_lu", 1),)
SPLIT = (("lu_split_min_rows", 0),)

A_SIZES = (6, 63, 64, 65, 257, 512, 513, 769, 1100)
KAPPAS = (1e2, 1e6, 1e10)
A_CASES = [(("spd", n, k), r, "host", ()) for n in A_SIZES for k in KAPPAS for r in RHS]
A_QUAD_SIZES = (65, 777)
A_QUAD_CASES = [(("spd", n, 1e2), "normal", "quadratic", ()) for n in A_QUAD_SIZES]

B_SIZES = (65, 513, 769)
B_KAPPAS = (1e2, 1e10)
B_CASES = [(("spd", n, k), r, "host", LU) for n in B_SIZES for k in B_KAPPAS for r in RHS]

C_SIZES = (6, 65, 449, 513, 1025, 2049)
C_SPLIT_SIZES = (449, 1025)
C_CASES = [(("gauss", n), "normal", "host", ()) for n in C_SIZES] + [(("gauss", n), "normal", "host", SPLIT) for n in C_SPLIT_SIZES]

D_SIZES = (70, 449, 1025)
D_CASES = [(("perm", n, p), "ints", "host", ()) for n in D_SIZES for p in PERMS]

E_PAIRS = ((130, 0), (130, 63), (130, 64), (130, 129), (300, 255), (300, 256), (300, 299), (900, 600), (900, 768), (900, 899))
E_CASES = [(("late", n, c), "normal", "host", ()) for n, c in E_PAIRS]

# F: two factorisations in one solver, in both orders.  The SPD one takes the "range" right-hand side: its step is then of order 1, as the
# other's, and the rounding of x_2 = x_1 + d_2 (2^-53 ||x_2||, which eta sees because d_2 is recovered as x_2 - x_1) stays a few units of B
F_LATE = (("late", 300, 256), "normal")
F_SPD = (("spd", 300, 1e2), "range")
F_ORDERS = ((F_LATE, F_SPD), (F_SPD, F_LATE))

G_CASE = (("ulp", 257, 1e2), "normal", "host", ())
G_SYMMETRIC = (("spd", 257, 1e2), "normal", "host", ())

H_EXPONENTS = (200, -200)
H_BASES = ((("spd", 257, 1e2), "normal"), (("gauss", 449), "normal"))
H_CASES = [(("scaled", k, e), r, "host", ()) for k, r in H_BASES for e in H_EXPONENTS]

I_SIZES = (2, 3, 4, 5)
I_CASES = [(("small", n), "normal", "host", ()) for n in I_SIZES]

ETA_CASES = A_CASES + A_QUAD_CASES + B_CASES + C_CASES + H_CASES + I_CASES + [G_CASE]
J_CANDIDATES = A_CASES + A_QUAD_CASES + B_CASES + C_CASES
J_LIMIT = 1e-3  # the second solve is checked where kappa_inf(H) B(n) is below this: everywhere but kappa = 1e10 from n = 257 up (2.6e-3 ... 3.2e-2;
# tests/test_ref_newton_solve.py::test_second_solve_cases_are_the_ones_inside_the_limit holds the list to the rule)
J_CASES = [c for c in J_CANDIDATES if not (c[0][0] == "spd" and c[0][2] == 1e10 and c[0][1] >= 257)]
ALL_CASES = ETA_CASES + D_CASES + E_CASES


def case_id(case):
    key, r, via, options = case

    def flat(k):
        return "-".join(flat(p) if isinstance(p, tuple) else (f"{p:g}" if isinstance(p, float) else str(p)) for p in k)
    tail = "".join(f"-{name}{value}" for name, value in options)
    return f"{flat(key)}-{r}-{via}{tail}"


def size(case):
    return matrix(case[0]).shape[0]


def decrement_bound(n, d_inf, z_inf, kb):
    """|dec - dec*| for dec = z . d, z a solve of H z = d with backward error B: the forward bound ||z - z*|| <= 2 kappa B / (1 - kappa B) ||z*||
    (Higham Thm 7.2) in every term of the dot product, plus the dot product's own rounding n 2^-53"""
    return n * d_inf * z_inf * (2.0 * kb / (1.0 - kb) + n * U)
