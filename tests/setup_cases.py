"""Launches of the set-up checks (test_setup_checks_host.py proves the inputs on the CPU, test_gpu_setup_checks.py
runs ckmi_newton_probe on them): the singular test of NewtonMatrixGJ64::factor() at EVERY pivot step.

factor() folds each step's largest FP32 key into one running value and returns `ok` from it, so three things can go
wrong that test_gpu_newton.py's three sampled columns (0, n - 1, one interior) do not pin down: a step whose key is
left out of the running value, a running value that is not started afresh in a call on the persistent matrix object,
and a zero key that is lost between its step and the end.  Every input and expectation here comes from
newton_cases.py's numpy references, never from the kernel.
"""
import functools

import numpy as np

import newton_cases as nc

# every wave class at n = N and one n < N (N - 1; 33 in the 64 class: the first order it takes over the 54 class's)
SIZES = {32: (32, 31), 54: (54, 53), 64: (64, 33)}
PARAMS = [(cls, n) for cls in nc.WAVE_CLASSES for n in SIZES[cls[1]]]
NREG = 3  # distinct regular neighbours (seeds 0..2), cycled through a launch


def tiny_system_at(n, k):
    """newton_cases.tiny_system with the tiny column at k: 0 on the diagonal (gamma 2^-100 x J 2^100), ~1e-61
    elsewhere -- nonzero in FP64, every FP32 key 0."""
    J0, _ = nc.regular_system(n, seed=7)
    J = (J0.astype(np.float64) * 2.0 ** 100).astype(np.float32)
    J[:, k] = np.asarray(1e-30 * (1.0 + np.arange(n) % 5), np.float32)
    J[k, k] = np.float32(2.0 ** 100)
    return J, nc.TINY_GAMMA


class Launch(nc.Case):
    """One launch: `bad` [(J, gamma)], each between two regular systems -- regular, bad[0], regular, bad[1], ...,
    regular.  Fields and bounds as newton_cases.Case; the references of the NREG regular systems are computed once
    per order and shared."""

    def __init__(self, n, bad):
        self.family, self.n = "setup", n
        sy = []
        for i, s in enumerate(bad):
            sy += [nc.regular_system(n, seed=i % NREG), s]
        sy.append(nc.regular_system(n, seed=len(bad) % NREG))
        ns = len(sy)
        self.J = np.stack([s[0] for s in sy])
        self.gamma = np.array([s[1] for s in sy])
        self.ok = np.array([i % 2 == 0 for i in range(ns)])
        self.B = np.stack([nc.rhs(n, (i // 2) % NREG) for i in range(ns)])
        nr = self.B.shape[1]
        self.Xa = np.full((ns, nr, n), np.nan)
        self.Xb = np.full((ns, nr, n), np.nan)
        self.scale = np.full((ns, nr, n), np.nan)
        self.perm = np.zeros((ns, n), int)
        self.gaps = np.zeros((ns, n))
        self.ok_b = np.zeros(ns, bool)
        self.Binv = [None] * ns
        for i in range(ns):
            if self.ok[i]:
                r = regular_reference(n, (i // 2) % NREG)
                self.Binv[i], self.perm[i], self.ok_b[i], self.gaps[i] = r["Binv"], r["perm"], r["ok"], r["gaps"]
                self.Xa[i], self.Xb[i], self.scale[i] = r["Xa"], r["Xb"], r["scale"]
            else:
                _, _, self.ok_b[i], _ = nc.gauss_jordan(nc.matrix(self.J[i], self.gamma[i]))


@functools.lru_cache(maxsize=None)
def regular_reference(n, seed):
    """Both references of regular_system(n, seed) on rhs(n, seed)."""
    J, g = nc.regular_system(n, seed=seed)
    B = nc.rhs(n, seed)
    Binv, perm, ok, gaps = nc.gauss_jordan(nc.matrix(J, g))
    return dict(Binv=Binv, perm=perm, ok=ok, gaps=gaps, Xa=nc.extended_solution(J, g, B),
                Xb=nc.gj_solve(Binv, perm, B), scale=nc.solve_scale(Binv, perm, B))


@functools.lru_cache(maxsize=None)
def every_step(n):
    """For every pivot step k one system whose column k of I - gamma J is exactly zero: 2 n + 1 systems."""
    return Launch(n, [nc.singular_system(n, k) for k in range(n)])


@functools.lru_cache(maxsize=None)
def tiny_ends(n):
    """The tiny column at step 0 and at step n - 1."""
    return Launch(n, [tiny_system_at(n, 0), tiny_system_at(n, n - 1)])
