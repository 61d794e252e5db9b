"""CPU-side preconditions of tests/test_gpu_newton.py: every matrix family does what the GPU test relies on (the
forced pivot orders have their key gap, the tie is a tie, the singular columns are exactly zero, the tiny column is
nonzero in FP64 and zero in every FP32 key), the two references agree, the FP32-stored bound is sharp, and the
faults this code can plausibly have, planted into the restatement, fail the bounds the GPU test applies.
"""
import numpy as np
import pytest

import newton_cases as nc

HOST_N = sorted({n for cls in nc.CLASSES for n in nc.sizes(cls)})
# the restatement is held to the bounds at one size per block structure (the references of the largest orders take
# seconds each in extended precision; test_gpu_newton.py computes them all on the GPU machine)
BOUND_N = (2, 11, 32, 54, 61, 64, 113, 192)


def test_classes_and_sizes():
    """The 14 classes ckmi_dispatch.hpp's visitors compile, each at its block edges."""
    assert len(nc.CLASSES) == 14 and (1, 32, 0) not in nc.CLASSES
    for cls in nc.CLASSES:
        s = nc.sizes(cls)
        assert min(s) >= 2 and max(s) == nc.nmax(cls)
        if cls[0] == 2 and cls[1] > 4:  # the first size the variant takes, a panel boundary (n + 3) & ~3, exactly full
            assert s[0] == 16 * (cls[1] - 1) + 1 and any(x % 4 for x in s) and any(x % 4 == 0 for x in s)
        assert all("real" in nc.families(cls, n) for n in s if cls[0] == 1 and n == 54)
    assert sum(len(nc.families(cls, n)) for cls in nc.CLASSES for n in nc.sizes(cls)) == len(
        [1 for cls in nc.CLASSES for n in nc.sizes(cls)]) * 5 + 4


@pytest.mark.parametrize("n", HOST_N)
def test_forced_order_has_its_key_gap(n):
    """M = P D: at every step of the restatement the second-largest FP32 key is below 0.7 x the largest, so the
    pivot sequence is P^-1 whatever the rounding of the elimination before it."""
    for kind in nc.PERMS:
        J, g = nc.forced_system(kind, n)
        M = nc.matrix(J, g)
        D = M[nc.forced_pivots(kind, n)]  # rows back in natural order
        off = np.abs(D).sum(axis=1) - np.abs(np.diag(D))
        assert np.all(off <= 0.3 * (1 + 1e-6)) and np.all(np.abs(np.diag(D)) >= 1.0 - 1e-6)
        _, perm, ok, gaps = nc.gauss_jordan(M)
        assert ok and perm.tolist() == nc.forced_pivots(kind, n).tolist()
        assert gaps.max() < nc.KEY_GAP, (kind, gaps.max())
    # the orders put pivots in every 16-lane row, in the last lane / row, and across waves and panels of four
    if n >= 64:
        p = nc.forced_pivots("random", n)
        assert len({int(x) // 16 for x in p[:16]}) >= 3
        assert nc.forced_pivots("reversal", n)[0] == n - 1 and nc.forced_pivots("shift17", n)[0] == n - 17
        assert any(p[k] // 4 != p[k + 1] // 4 for k in range(0, n - 1, 4))


@pytest.mark.parametrize("n", HOST_N)
def test_tie_singular_and_tiny_inputs(n):
    J, g = nc.tie_system(n)
    M = nc.matrix(J, g)
    assert np.all(np.abs(M[:, 0]) == 1.0)  # exact after the FP32 rounding of J: every row ties
    _, perm, ok, gaps = nc.gauss_jordan(M)
    assert ok and perm[0] == 0 and gaps[0] == 1.0
    for k in nc.singular_columns(n):
        J, g = nc.singular_system(n, k)
        M = nc.matrix(J, g)
        assert np.all(M[:, k] == 0.0) and np.all(nc.matrix(J, g, np.longdouble)[:, k] == 0)
        assert not nc.gauss_jordan(M)[2]
    assert 0 in nc.singular_columns(n) and n - 1 in nc.singular_columns(n)
    assert (n - 1) & ~3 in nc.singular_columns(n)  # inside the last panel of four
    # the tiny column: nonzero in FP64, every FP32 key 0 (far below the smallest subnormal, 2^-149, so that
    # flushing or keeping subnormals makes no difference).  The rule: a column whose largest |a| rounds to an FP32
    # zero is singular, although FP64 could still divide by it.
    J, g = nc.tiny_system(n)
    M = nc.matrix(J, g)
    k = n // 2
    assert M[k, k] == 0.0 and np.all(M[np.arange(n) != k, k] != 0.0) and np.max(np.abs(M[:, k])) < 2.0 ** -190
    assert np.all(np.abs(M[:, k]).astype(np.float32) == 0.0)
    a, _, ok, _ = nc.gauss_jordan(M)
    assert not ok
    assert np.all(nc.expect_ok("tiny", n) == [True, False, True])
    for J, g in (nc.regular_system(n), nc.regular_system(n, seed=1)):
        assert np.linalg.cond(nc.matrix(J, g)) < 10.0


def test_newton_like_condition_numbers():
    """The family's own gamma leaves M near the identity; gamma = 1e-3 and 1e-2 bring the 2-norm condition numbers
    to 1e2..1e6 (1.3e6 at n = 64; the real Newton matrices of n = 54 reach 1e8..1e14)."""
    hi = []
    for n in (54, 64, 192):
        s = nc.newton_systems(n)
        conds = [np.linalg.cond(nc.matrix(J, g)) for J, g in s]
        assert s[0][1] <= 1e-5 and s[1][1] <= 1e-5 and (s[2][1], s[3][1]) == (1e-3, 1e-2)
        assert np.array_equal(s[0][0], s[2][0]) and np.array_equal(s[1][0], s[3][0])  # the same J
        hi.append(max(conds))
        assert max(conds) < 1e10  # extended_solution's refinement converges
    assert max(hi) > 1e6


def test_real_newton_matrices():
    """I - gamma J at the oracle's GRI-3.0 Jacobians: 2 states x 3 gamma, finite, n = 54, J as parked (FP32)."""
    s = nc.real_systems()
    assert len(s) == 6 and [g for _, g in s] == list(nc.REAL_GAMMAS) * 2
    for J, g in s:
        assert J.shape == (54, 54) and J.dtype == np.float32 and np.isfinite(J).all()
        assert nc.gauss_jordan(nc.matrix(J, g))[2]
    assert not np.array_equal(s[0][0], s[3][0])


@pytest.mark.parametrize("n", BOUND_N)
def test_restatement_meets_the_bounds(n):
    """The unfaulted restatement passes every bound the GPU test applies, in FP64 and with its inverse rounded to
    FP32 element by element; the latter uses most of its bound (the bound is the rounding and nothing else)."""
    use = []
    for family in nc.FAMILIES:
        if family == "real" and n != 54:
            continue
        c = nc.case(family, n)
        assert c.ok_b.tolist() == c.ok.tolist()
        for i in np.nonzero(c.ok)[0]:
            assert np.isfinite(c.Xa[i]).all() and np.isfinite(c.Xb[i]).all()
            assert c.err_b(i) <= 1e-6 * np.max(np.abs(c.Xa[i]))  # the two references agree
            assert c.ratio64(i, c.Xb[i]) <= 1.0 / nc.MARGIN
            use.append(c.ratio32(i, nc.fp32_stored_solution(c.Binv[i], c.perm[i], c.B[i])))
    assert max(use) <= 1.0
    if n >= 11:
        assert min(use) > 0.4


def _breaks(c, i, X):
    return c.ratio64(i, X) > 1.0 and c.ratio32(i, X) > 1.0


def test_fp32_bound_sees_single_elements():
    """n = 54 real Newton matrices: zeroing one element of the FP32-stored inverse, or swapping it with its right
    neighbour, breaks the componentwise bound wherever the element stands above the FP64 term of the bound (an
    absolute per-system figure: 10 x the restatement's error plus the solve's rounding); the unit vectors read
    every element out."""
    c = nc.case("real", 54)
    rng = np.random.default_rng(5)
    for i in range(len(c.ok)):
        B32 = c.Binv[i].astype(np.float32).astype(np.float64)
        assert c.ratio32(i, nc.gj_solve(B32, c.perm[i], c.B[i])) <= 1.0
        seen = np.abs(B32) * (1.0 - nc.EPS32S) > c.bound64(i)
        assert seen.mean() > 0.5, seen.mean()  # most of the inverse is within the bound's sight
        r, q = np.nonzero(seen)
        for t in rng.choice(r.size, 60, replace=False):
            Z = B32.copy()
            Z[r[t], q[t]] = 0.0
            assert c.ratio32(i, nc.gj_solve(Z, c.perm[i], c.B[i])) > 1.0, (i, r[t], q[t])
            q2 = (q[t] + 1) % 54
            if abs(abs(B32[r[t], q[t]]) - abs(B32[r[t], q2])) * (1.0 - nc.EPS32S) > 2.0 * c.bound64(i):
                S = B32.copy()
                S[r[t], [q[t], q2]] = S[r[t], [q2, q[t]]]
                assert c.ratio32(i, nc.gj_solve(S, c.perm[i], c.B[i])) > 1.0, (i, r[t], q[t])


def _faulted(c, i, fault):
    Bi, perm, ok, _ = nc.gauss_jordan(nc.matrix(c.J[i], c.gamma[i]), fault=fault)
    return nc.gj_solve(Bi, perm, c.B[i]) if ok else np.full_like(c.Xa[i], np.nan)


def test_planted_faults_fail_the_bounds():
    """Each fault this code can plausibly have, planted into the restatement, fails the FP64 and the FP32-stored
    bound on at least one case of the GPU test (a NaN counts as a failure: the GPU test asserts finiteness)."""
    def fails(c, i, X):
        return (not np.isfinite(X).all()) or _breaks(c, i, X)

    # the pivot search does not mask the used rows on one step: a used row wins wherever its entry is the larger
    hit = 0
    for family, n in (("newton", 54), ("forced", 61), ("tie", 64)):
        c = nc.case(family, n)
        for i in np.nonzero(c.ok)[0]:
            for k in range(1, n):
                _, perm, ok, _ = nc.gauss_jordan(nc.matrix(c.J[i], c.gamma[i]), fault=("unmasked", k))
                if not ok or perm.tolist() != c.perm[i].tolist():
                    assert fails(c, i, _faulted(c, i, ("unmasked", k))), (family, i, k)
                    hit += 1
                    break
    assert hit >= 1
    # perm applied once instead of twice in the solve: every permuting system
    c = nc.case("forced", 61)
    for i, kind in enumerate(nc.PERMS):
        X = nc.gj_solve(c.Binv[i], c.perm[i], c.B[i], once=True)
        assert fails(c, i, X) == (kind != "identity"), kind
    # a panel of four skipped that holds a live column: the last, partly padded one
    for n in (61, 113, 177):
        c = nc.case("tie", n)
        assert fails(c, 0, _faulted(c, 0, ("skip", (n - 1) & ~3))), n
        c = nc.case("forced", n)
        assert all(fails(c, i, _faulted(c, i, ("skip", (n - 1) & ~3))) for i in range(len(nc.PERMS))), n
    # column k of the inverse left as the multiplier
    for family, n in (("newton", 54), ("forced", 64), ("singular", 33)):
        c = nc.case(family, n)
        for i in np.nonzero(c.ok)[0]:
            for k in (0, n // 2, n - 1):
                assert fails(c, i, _faulted(c, i, ("multiplier", k))), (family, n, i, k)
