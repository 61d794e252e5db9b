"""The singular test of the wave kernels' Newton set-up at every pivot step (ckmi_newton_probe on the launches of
setup_cases.py; test_setup_checks_host.py proves the inputs on the CPU).

NewtonMatrixGJ64::factor() returns `ok` = false exactly when some step's largest FP32 key is 0.  Every wave class
(N = 32 FP32-stored; 54 and 64 in both forms), at n = N and one n < N:

  every step         for each k in 0..n-1 a system whose column k of I - gamma J is exactly zero, each between two
                     regular systems of the same launch: ok = 0 for exactly those, every regular neighbour has ok = 1,
                     the reference's pivots and its solutions inside the bound of its class (test_gpu_newton.py's)
  persistent object  a set-up with a zero column k, any k, before a regular one on the same matrix object leaves no
                     trace (ok = 1, the same bits as without it); a regular one before a singular one does not
                     hide it (ok = 0)
  tiny column        nonzero in FP64, FP32 key 0, at step 0 and at step n - 1
"""
import numpy as np
import pytest

import newton_cases as nc
import setup_cases as sc

pytestmark = pytest.mark.gpu


def probe(cls, J, gamma, B, **kw):
    from pychemkin_amd import _native

    return _native.newton_probe(cls[0], cls[1], bool(cls[2]), J, gamma, B, **kw)


def _ids(v):
    return nc.class_id(v) if isinstance(v, tuple) else str(v)


def _judge(cls, c, X, perm, ok, what):
    """ok as the launch states it; the regular systems' pivots and solutions against the references."""
    n = c.n
    assert ok.tolist() == c.ok.astype(int).tolist(), (what, np.nonzero(ok != c.ok.astype(int))[0].tolist())
    worst = 0.0
    for i in np.nonzero(c.ok)[0]:
        assert perm[i].tolist() == c.perm[i].tolist(), (what, i, perm[i])
        assert np.isfinite(X[i]).all(), (what, i)
        worst = max(worst, c.ratio(i, X[i], cls[2]))
    print(f"setup-ratio {nc.class_id(cls)} n={n} {what}: {worst:.3f}")
    assert worst <= 1.0, what


@pytest.mark.parametrize("cls,n", sc.PARAMS, ids=_ids)
def test_zero_column_at_every_step(cls, n):
    c = sc.every_step(n)
    X, perm, ok = probe(cls, c.J, c.gamma, c.B)
    _judge(cls, c, X, perm, ok, "every-step")


@pytest.mark.parametrize("cls,n", sc.PARAMS, ids=_ids)
def test_persistent_object_at_every_step(cls, n):
    """Pass 0 of the probe is a set-up on the same matrix object before the judged one."""
    c = sc.every_step(n)
    reg = np.arange(0, 2 * n, 2)  # the regular system in front of the zero column of step k
    bad = reg + 1
    # singular (step k), then regular
    X0, perm0, ok0 = probe(cls, c.J[reg], c.gamma[reg], c.B[reg])
    X, perm, ok = probe(cls, c.J[reg], c.gamma[reg], c.B[reg], J_prev=c.J[bad], gamma_prev=c.gamma[bad])
    assert ok0.tolist() == [1] * n == ok.tolist(), np.nonzero(ok != 1)[0].tolist()
    assert np.array_equal(perm, perm0) and np.array_equal(X, X0)
    worst = 0.0
    for j, i in enumerate(reg):
        assert perm[j].tolist() == c.perm[i].tolist(), j
        worst = max(worst, c.ratio(i, X[j], cls[2]))
    print(f"setup-ratio {nc.class_id(cls)} n={n} singular-then-regular: {worst:.3f}")
    assert worst <= 1.0
    # regular, then singular (step k)
    _, _, ok = probe(cls, c.J[bad], c.gamma[bad], c.B[bad], J_prev=c.J[reg], gamma_prev=c.gamma[reg])
    assert ok.tolist() == [0] * n, np.nonzero(ok)[0].tolist()


@pytest.mark.parametrize("cls,n", sc.PARAMS, ids=_ids)
def test_tiny_column_first_and_last_step(cls, n):
    c = sc.tiny_ends(n)
    X, perm, ok = probe(cls, c.J, c.gamma, c.B)
    _judge(cls, c, X, perm, ok, "tiny")
    bad, reg = np.array([1, 3]), np.array([0, 2])
    X2, perm2, ok2 = probe(cls, c.J[reg], c.gamma[reg], c.B[reg], J_prev=c.J[bad], gamma_prev=c.gamma[bad])
    assert ok2.tolist() == [1, 1] and np.array_equal(perm2, perm[reg]) and np.array_equal(X2, X[reg])
    _, _, ok3 = probe(cls, c.J[bad], c.gamma[bad], c.B[bad], J_prev=c.J[reg], gamma_prev=c.gamma[reg])
    assert ok3.tolist() == [0, 0]
