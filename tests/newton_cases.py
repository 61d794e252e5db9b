"""Matrices, right-hand sides, references and bounds of the Newton-matrix probe tests (test_newton_reference_host.py
proves on the CPU that every input does what the GPU test relies on, test_gpu_newton.py runs ckmi_newton_probe on
them).

A system is (J [n][n] float32, gamma): the kernels form M = I - gamma J from the parked FP32 Jacobian.  Two
references, both numpy: (a) the solution of M x = b with M formed and the residual accumulated in np.longdouble,
(b) a plain FP64 restatement of the kernels' algorithm (gauss_jordan: Gauss-Jordan to the explicit inverse of the
row-permuted matrix, pivots by the largest |a| rounded to FP32 among the unused rows, ties to the lowest row).
"""
import functools

import numpy as np

from mechanism_variants import newton_like_parts, tie_matrix

EPS64 = 2.0 ** -52
EPS32S = 2.0 ** -24 * (1.0 + 1e-3)  # rounding of one FP32-stored element of the inverse
MARGIN = 10.0                       # the project's margin for reordered and contracted sums (test_gpu_equilibrium.py)
KEY_GAP = 0.7                       # forced-order family: second-largest FP32 key below this x the largest

# (kernel, size, f32_stored): the 14 matrix classes visit_wave_variant / visit_big_variant compile
WAVE_CLASSES = [(1, 32, 1), (1, 54, 1), (1, 54, 0), (1, 64, 1), (1, 64, 0)]
BIG_CLASSES = [(2, nb, 0) for nb in range(4, 13)]
CLASSES = WAVE_CLASSES + BIG_CLASSES
FAMILIES = ("newton", "real", "forced", "tie", "singular", "tiny")
PERMS = ("identity", "reversal", "shift1", "shift17", "random")
REAL_GAMMAS = (1e-9, 1e-6, 1e-4)
NRAND = 3  # seeded random right-hand sides behind the n unit vectors


def class_id(cls):
    k, size, f32 = cls
    return f"wave{size}-{'f32s' if f32 else 'f64'}" if k == 1 else f"wg{size}"


def sizes(cls):
    """The block edges of a class."""
    k, size, _ = cls
    if k == 1:
        return {32: (2, 11, 31, 32), 54: (33, 53, 54), 64: (54, 55, 63, 64)}[size]
    if size == 4:
        return (2, 5, 17, 49, 61, 63, 64)
    if size == 12:
        return (177, 191, 192)
    return (16 * (size - 1) + 1, 16 * (size - 1) + 4, 16 * size - 3, 16 * size - 1, 16 * size)


def families(cls, n):
    return tuple(f for f in FAMILIES if f != "real" or (cls[0] == 1 and n == 54))


def nmax(cls):
    return cls[1] if cls[0] == 1 else 16 * cls[1]


# ---------------------------------------------------------------------- references
def matrix(J, gamma, dtype=np.float64):
    """M = I - gamma float32(J), formed in dtype."""
    J = np.asarray(J, np.float32)
    return np.eye(J.shape[0], dtype=dtype) - dtype(gamma) * J.astype(dtype)


def extended_solution(J, gamma, B):
    """Reference (a): X [nrhs][n] of M x = b, M and the residuals in np.longdouble (LAPACK's solution, three steps of
    refinement: the correction is then below the FP64 rounding of x on every family here)."""
    Ml = matrix(J, gamma, np.longdouble)
    M = Ml.astype(np.float64)
    Bl = np.asarray(B, np.float64).T.astype(np.longdouble)
    x = np.linalg.solve(M, Bl.astype(np.float64)).astype(np.longdouble)
    for _ in range(3):
        r = (Bl - Ml @ x).astype(np.float64)
        x = x + np.linalg.solve(M, r).astype(np.longdouble)
    return x.astype(np.float64).T


def gauss_jordan(M, fault=None):
    """Reference (b): the kernels' factorisation restated in FP64.  Returns (Binv, perm, ok, gaps): Binv the explicit
    inverse of the row-permuted matrix held by rows of M (row perm[k] of Binv is row k of (P M)^-1), perm[k] the
    pivot row of step k, ok False if a step's largest FP32 key was 0 (Binv is then garbage), gaps[k] the
    second-largest key over the largest of step k.

    fault plants what this code can plausibly get wrong (test_newton_reference_host.py's sharpness test):
    ("unmasked", k) the search of step k does not mask the used rows; ("multiplier", k) column k of the inverse is
    left as the multiplier g instead of -g / rcp; ("skip", k0) the four steps from k0 are skipped as if they were
    identity padding."""
    a = np.array(M, np.float64)
    n = a.shape[0]
    used = np.zeros(n, bool)
    perm = np.arange(n)
    gaps = np.zeros(n)
    ok = True
    kind, at = fault if fault else (None, -1)
    for k in range(n):
        if kind == "skip" and at <= k < at + 4:  # pivots on its own row and changes nothing
            used[k] = True
            continue
        with np.errstate(over="ignore"):
            key = np.abs(a[:, k]).astype(np.float32)
        cand = np.ones(n, bool) if (kind == "unmasked" and k == at) else ~used
        kk = np.where(cand, key, np.float32(-1.0))
        p = int(np.argmax(kk))  # the first of equal keys: the lowest row
        if kk[p] == 0.0:
            return a, perm, False, gaps
        rest = np.delete(kk, p)
        gaps[k] = float(rest.max() / kk[p]) if rest.size and rest.max() > 0 else 0.0
        piv = a[p, k]
        rcp = 1.0 / piv
        g = a[:, k] * rcp
        g[p] = (piv - 1.0) * rcp  # the pivot row becomes row / piv by the same update
        a -= np.outer(g, a[p].copy())
        if kind == "multiplier" and k == at:
            a[:, k] = g
        else:
            a[:, k] = -g
            a[p, k] = rcp
        used[p] = True
        perm[k] = p
    return a, perm, ok, gaps


def gj_solve(Binv, perm, B, once=False):
    """x_k = sum_j Binv[p_k][j] b[p_j] for the rows of B; once: the fault 'perm applied once' (b not permuted)."""
    B = np.asarray(B, np.float64)
    return (Binv[perm] @ (B if once else B[:, perm]).T).T


def solve_scale(Binv, perm, B):
    """(|Binv| |P b|)_k [nrhs][n]: what a solve's rounding is proportional to."""
    return (np.abs(Binv[perm]) @ np.abs(np.asarray(B, np.float64)[:, perm]).T).T


# ---------------------------------------------------------------------- right-hand sides
def rhs(n, seed):
    """The n unit vectors (they read out the inverse entry by entry) and NRAND seeded random vectors."""
    rng = np.random.default_rng(9000 + 17 * n + seed)
    return np.concatenate([np.eye(n), rng.standard_normal((NRAND, n))])


# ---------------------------------------------------------------------- matrix families
def _f32(x):
    return np.asarray(x, np.float32)


def newton_systems(n):
    """mechanism_variants.newton_like's J (entries over nine decades) at its own gamma (1e-9..1e-5) and the same J
    at gamma = 1e-3 and 1e-2, where the matrix is far from the identity (condition numbers 1e2..1e6)."""
    J, g = newton_like_parts(np.random.default_rng(4100 + n), 2, n)
    return [(_f32(J[0]), float(g[0, 0, 0])), (_f32(J[1]), float(g[1, 0, 0])), (_f32(J[0]), 1e-3), (_f32(J[1]), 1e-2)]


@functools.lru_cache(maxsize=None)
def real_systems():
    """I - gamma J with J the oracle's GRI-3.0 Jacobian at the max_dTdt and burnt states of jacobian_cases."""
    import jacobian_cases as jc

    st, orc = jc.states("gri"), jc.oracle("gri")
    out = []
    for i in (2, 3):
        _, J = orc.rhs_jac(st["y"][i], problem=1, energy=1, P0=jc.P_CTX)
        out += [(_f32(J), g) for g in REAL_GAMMAS]
    return out


def permutation(kind, n):
    """pi with (P D)[i] = D[pi[i]]."""
    i = np.arange(n)
    if kind == "identity":
        return i
    if kind == "reversal":
        return i[::-1].copy()
    if kind.startswith("shift"):
        return (i + int(kind[5:])) % n
    return np.random.default_rng(77 + n).permutation(n)


def forced_system(kind, n):
    """M = P D with D strictly diagonally dominant (|d_ii| in [1, 1.5], off-diagonal row sums <= 0.3): the pivot
    of step k is the row i with pi[i] = k, whatever the rounding.  gamma = 1, J = I - M rounded to FP32."""
    rng = np.random.default_rng(5200 + 31 * n + PERMS.index(kind))
    D = rng.uniform(-1.0, 1.0, (n, n))
    np.fill_diagonal(D, 0.0)
    D *= 0.3 * rng.uniform(0.2, 1.0, (n, 1)) / np.maximum(np.abs(D).sum(axis=1, keepdims=True), 1e-300)
    D += np.diag(rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 1.5, n))
    pi = permutation(kind, n)
    return _f32(np.eye(n) - D[pi]), 1.0


def forced_pivots(kind, n):
    """perm[k] = the row i with pi[i] = k: P^-1."""
    return np.argsort(permutation(kind, n))


def tie_system(n):
    """mechanism_variants.tie_matrix: the first column is all +-1 (exact in FP32), the first pivot must be row 0."""
    return _f32(np.eye(n) - tie_matrix(n)), 1.0


def regular_system(n, seed=0):
    """A well-conditioned neighbour: gamma = 1, |J_ij| <= 0.5 / n."""
    rng = np.random.default_rng(6300 + 13 * n + seed)
    return _f32(rng.uniform(-0.5, 0.5, (n, n)) / n), 1.0


def singular_columns(n):
    """Column 0, a middle column, the last one and the first column of the last panel of four (partly padding in
    the workgroup kernel unless n is a multiple of 4)."""
    return sorted({0, n // 2, n - 1, (n - 1) & ~3})


def singular_system(n, k):
    """gamma = 1 and J[:, k] = e_k: column k of M is exactly zero."""
    J, _ = regular_system(n, seed=100 + k)
    J = J.copy()
    J[:, k] = 0.0
    J[k, k] = 1.0
    return J, 1.0


TINY_GAMMA = 2.0 ** -100


def tiny_system(n):
    """Column n // 2 of M is 0 on the diagonal (gamma 2^-100 x J 2^100) and ~1e-61 elsewhere: nonzero in FP64, below
    the smallest FP32 subnormal, so every key of the column rounds to 0.  The other columns are regular_system's."""
    J0, _ = regular_system(n, seed=7)
    J = (J0.astype(np.float64) * 2.0 ** 100).astype(np.float32)
    k = n // 2
    J[:, k] = _f32(1e-30 * (1.0 + np.arange(n) % 5))
    J[k, k] = np.float32(2.0 ** 100)
    return J, TINY_GAMMA


def systems(family, n):
    """[(J, gamma)] of a family at order n, the launch of one test; and the indices that must come back ok."""
    if family == "newton":
        s = newton_systems(n)
    elif family == "real":
        assert n == 54
        s = list(real_systems())
    elif family == "forced":
        s = [forced_system(kind, n) for kind in PERMS]
    elif family == "tie":
        s = [tie_system(n)]
    elif family == "singular":  # regular neighbours around every singular system
        s = [regular_system(n)]
        for k in singular_columns(n):
            s += [singular_system(n, k), regular_system(n, seed=1 + k)]
    elif family == "tiny":
        s = [regular_system(n), tiny_system(n), regular_system(n, seed=1)]
    else:
        raise KeyError(family)
    return s


def expect_ok(family, n):
    ns = len(systems(family, n))
    if family in ("singular", "tiny"):
        return np.array([i % 2 == 0 for i in range(ns)])
    return np.ones(ns, bool)


# ---------------------------------------------------------------------- a case: inputs, references, bounds
class Case:
    """The launch of one (n, family) and what the references say about it (shared by every class that takes n)."""

    def __init__(self, family, n):
        self.family, self.n = family, n
        sy = systems(family, n)
        self.J = np.stack([s[0] for s in sy])
        self.gamma = np.array([s[1] for s in sy])
        self.ok = expect_ok(family, n)
        ns = len(sy)
        self.B = np.stack([rhs(n, i) for i in range(ns)])
        nr = self.B.shape[1]
        self.Xa = np.full((ns, nr, n), np.nan)      # reference (a)
        self.Xb = np.full((ns, nr, n), np.nan)      # reference (b)
        self.scale = np.full((ns, nr, n), np.nan)   # (|Binv| |P b|)_k of (b)
        self.perm = np.zeros((ns, n), int)
        self.gaps = np.zeros((ns, n))
        self.ok_b = np.zeros(ns, bool)
        self.Binv = [None] * ns
        for i in range(ns):
            Bi, self.perm[i], self.ok_b[i], self.gaps[i] = gauss_jordan(matrix(self.J[i], self.gamma[i]))
            if not self.ok_b[i]:
                continue
            self.Binv[i] = Bi
            self.Xa[i] = extended_solution(self.J[i], self.gamma[i], self.B[i])
            self.Xb[i] = gj_solve(Bi, self.perm[i], self.B[i])
            self.scale[i] = solve_scale(Bi, self.perm[i], self.B[i])

    def err_b(self, i):
        """Error of restatement (b) against (a) on system i."""
        return float(np.max(np.abs(self.Xb[i] - self.Xa[i])))

    def bound64(self, i):
        """FP64 forms, per system: MARGIN x the error of (b) against (a), plus the rounding bound of the solve's
        dot product alone, n 2^-52 max_k (|Binv| |P b|)_k."""
        return MARGIN * self.err_b(i) + self.n * EPS64 * float(np.max(self.scale[i]))

    def bound32(self, i):
        """FP32-stored form, componentwise [nrhs][n]: the rounding of each stored element, plus the FP64 bound."""
        return EPS32S * self.scale[i] + self.bound64(i)

    def ratio64(self, i, X):
        return float(np.max(np.abs(X - self.Xa[i]))) / self.bound64(i)

    def ratio32(self, i, X):
        return float(np.max(np.abs(X - self.Xa[i]) / self.bound32(i)))

    def ratio(self, i, X, f32):
        return self.ratio32(i, X) if f32 else self.ratio64(i, X)


@functools.lru_cache(maxsize=None)
def case(family, n):
    return Case(family, n)


def all_cases():
    """(family, n) of every test, each once."""
    seen = []
    for cls in CLASSES:
        for n in sizes(cls):
            for f in families(cls, n):
                if (f, n) not in seen:
                    seen.append((f, n))
    return seen


def fp32_stored_solution(Binv, perm, B):
    """Restatement (b) with the inverse rounded to FP32 element by element, as NewtonMatrixF32S stores it."""
    return gj_solve(Binv.astype(np.float32).astype(np.float64), perm, B)
