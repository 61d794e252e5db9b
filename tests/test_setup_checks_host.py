"""CPU-side preconditions of tests/test_gpu_setup_checks.py: each planted column is exactly zero (or, for the tiny
column, nonzero in FP64 with every FP32 key 0), the neighbours are regular with a pivot order no rounding changes,
and the references' `ok` vector is the one the GPU test states.
"""
import numpy as np
import pytest

import newton_cases as nc
import setup_cases as sc

HOST_N = sorted({n for _, n in sc.PARAMS})


def test_classes_and_sizes():
    """Every wave class, at n = N and one n < N."""
    assert [cls for cls, _ in sc.PARAMS[::2]] == nc.WAVE_CLASSES
    for cls, n in sc.PARAMS:
        assert n <= cls[1] and (cls[1] != 64 or n > 32)
    assert {n for cls, n in sc.PARAMS if n == cls[1]} == {32, 54, 64}
    assert {n for cls, n in sc.PARAMS if n < cls[1]} == {31, 53, 33}


@pytest.mark.parametrize("n", HOST_N)
def test_every_step_has_its_zero_column(n):
    c = sc.every_step(n)
    assert len(c.ok) == 2 * n + 1 <= 3 * 64
    assert c.ok.tolist() == [i % 2 == 0 for i in range(2 * n + 1)]
    assert c.ok_b.tolist() == c.ok.tolist()  # the reference's ok vector is as stated
    for k in range(n):
        J, g = c.J[2 * k + 1], c.gamma[2 * k + 1]
        assert g == 1.0 and J[k, k] == 1.0 and np.all(np.delete(J[:, k], k) == 0.0)
        M = nc.matrix(J, g)
        assert np.all(M[:, k] == 0.0) and np.all(nc.matrix(J, g, np.longdouble)[:, k] == 0)
        # column k alone: every other column has its nonzero diagonal, so the steps before k find a pivot
        assert np.all(np.abs(np.delete(np.diag(M), k)) > 0.5)
        # the restatement fails at step k and not before: with column k made regular again it goes through
        J2 = J.copy()
        J2[k, k] = 0.0
        assert nc.gauss_jordan(nc.matrix(J2, g))[2]


@pytest.mark.parametrize("n", HOST_N)
def test_neighbours_are_regular(n):
    for seed in range(sc.NREG):
        J, g = nc.regular_system(n, seed=seed)
        assert np.linalg.cond(nc.matrix(J, g)) < 10.0
        r = sc.regular_reference(n, seed)
        assert r["ok"] and r["perm"].tolist() == list(range(n))
        assert r["gaps"].max() < nc.KEY_GAP  # the pivot order holds whatever the rounding
        assert np.isfinite(r["Xa"]).all() and np.max(np.abs(r["Xb"] - r["Xa"])) <= 1e-12 * np.max(np.abs(r["Xa"]))
    c = sc.every_step(n)
    for i in np.nonzero(c.ok)[0]:
        assert np.array_equal(c.J[i], nc.regular_system(n, seed=(i // 2) % sc.NREG)[0])
        assert c.ratio64(i, c.Xb[i]) <= 1.0 / nc.MARGIN
        assert c.ratio32(i, nc.fp32_stored_solution(c.Binv[i], c.perm[i], c.B[i])) <= 1.0


@pytest.mark.parametrize("n", HOST_N)
def test_tiny_column_at_both_ends(n):
    c = sc.tiny_ends(n)
    assert c.ok.tolist() == [True, False, True, False, True] == c.ok_b.tolist()
    for i, k in ((1, 0), (3, n - 1)):
        M = nc.matrix(c.J[i], c.gamma[i])
        assert M[k, k] == 0.0 and np.all(np.delete(M[:, k], k) != 0.0) and np.max(np.abs(M[:, k])) < 2.0 ** -190
        assert np.all(np.abs(M[:, k]).astype(np.float32) == 0.0)
        # the key is still 0 when its step comes: the restatement with the used rows' keys left in
        a = M.copy()
        for j in range(k):  # the steps before k pivot on the diagonal (regular columns, diagonally dominant)
            g = a[:, j] / a[j, j]
            g[j] = 0.0
            a -= np.outer(g, a[j].copy())
        assert np.all(np.abs(a[k:, k]).astype(np.float32) == 0.0) and np.any(a[k:, k] != 0.0)
