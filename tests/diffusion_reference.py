"""Independent numpy restatement of the diffusion coefficients (tests only; no fit tables of the package).

* ``binary_exact``: Chapman-Enskog D_jk at T, P straight from the TRANLIB parameters (no fit):
  D_jk = 3/16 sqrt(2 pi (kB T)^3 / m_jk) / (P pi sigma_jk^2 Omega11*(T / eps_jk, delta*_jk)), Omega11* by the
  Neufeld-Janzen-Aziz correlation + 0.19 delta*^2 / T*, TRANLIB's combination rules (polar-nonpolar pairs with
  the induction correction xi).
* ``binary_fits``: the fitted form, ln D_jk at 1 atm as a cubic in ln T by ``np.polyfit`` on the 50-point grid.
* ``binary_from_fits`` / ``mixture_averaged`` / ``multicomponent``: the three device results restated on a given
  fit table, the multicomponent matrix from the defining triple sum of L and ``np.linalg.inv``.
* ``multicomponent_longdouble``: the same matrix by a partial-pivoting Gauss-Jordan in ``np.longdouble``, the
  measure of the float64 restatement's own element-wise error.
"""
import numpy as np

KB = 1.380649e-16
NA = 6.02214076e23
P_ATM = 1.01325e6
XFLOOR = 1e-12


def omega11(ts, dstar):
    return (1.06036 * ts ** -0.15610 + 0.19300 * np.exp(-0.47635 * ts) + 1.03587 * np.exp(-1.52996 * ts)
            + 1.76474 * np.exp(-3.89411 * ts) + 0.19 * dstar ** 2 / ts)


def pair_parameters(params, induction=True):
    """eps_jk [K], sigma_jk [cm], delta*_jk as [KK][KK]; induction=False applies the plain geometric /
    arithmetic rule to every pair (what a polar-nonpolar pair must differ from)."""
    p = np.asarray(params, dtype=np.float64)
    eps, sig, mu, alpha = p[:, 1], p[:, 2] * 1e-8, p[:, 3] * 1e-18, p[:, 4] * 1e-24
    KK = len(eps)
    E = np.sqrt(np.outer(eps, eps))
    S = 0.5 * (sig[:, None] + sig[None, :])
    M2 = np.outer(mu, mu)
    if induction:
        for j in range(KK):
            for k in range(KK):
                if (mu[j] > 0) != (mu[k] > 0):
                    pp, nn = (j, k) if mu[j] > 0 else (k, j)
                    alpha_s = alpha[nn] / sig[nn] ** 3
                    mu_s2 = mu[pp] ** 2 / (eps[pp] * KB * sig[pp] ** 3)
                    xi = 1.0 + 0.25 * alpha_s * mu_s2 * np.sqrt(eps[pp] / eps[nn])
                    E[j, k] = xi ** 2 * np.sqrt(eps[nn] * eps[pp])
                    S[j, k] = 0.5 * (sig[nn] + sig[pp]) * xi ** (-1.0 / 6.0)
                    M2[j, k] = 0.0
    return E, S, 0.5 * M2 / (E * KB * S ** 3)


def binary_exact(T, P, wt, params, induction=True):
    """D_jk [KK][KK] [cm2/s] at one T [K] and P [dyn/cm2], no fit."""
    wt = np.asarray(wt, dtype=np.float64)
    E, S, dstar = pair_parameters(params, induction)
    m = np.outer(wt, wt) / (wt[:, None] + wt[None, :]) / NA
    kT = KB * T
    return 3.0 / 16.0 * np.sqrt(2.0 * np.pi * kT ** 3 / m) / (P * np.pi * S ** 2 * omega11(T / E, dstar))


def fit_grid(tlow=300.0, thigh=3500.0, npts=50):
    return tlow + (thigh - tlow) * np.arange(npts) / (npts - 1)


def binary_fits(wt, params, tlow=300.0, thigh=3500.0, induction=True):
    """[KK][KK][4]: ln D_jk(1 atm) = sum_n c_n (ln T)^n by np.polyfit on the 50-point grid."""
    Tg = fit_grid(tlow, thigh)
    lnD = np.log(np.stack([binary_exact(t, P_ATM, wt, params, induction) for t in Tg]))  # [50][KK][KK]
    KK = lnD.shape[1]
    c = np.polyfit(np.log(Tg), lnD.reshape(len(Tg), KK * KK), 3)  # highest power first
    return c[::-1].T.reshape(KK, KK, 4).copy()


def _cubic(f, x):
    return f[..., 0] + x * (f[..., 1] + x * (f[..., 2] + x * f[..., 3]))


def binary_from_fits(T, P, dfits):
    """[n][KK][KK] from a fit table, as ckmi_binary_diffusion."""
    T = np.atleast_1d(np.asarray(T, dtype=np.float64))
    P = np.atleast_1d(np.asarray(P, dtype=np.float64))
    x = np.log(T)[:, None, None]
    return np.exp(_cubic(np.asarray(dfits)[None], x)) * (P_ATM / P)[:, None, None]


def floored_mole_fractions(Y, wt):
    """X~ [KK] of one state: negative mass fractions count as 0, then (X+ + 1e-12) / sum (X+ + 1e-12)."""
    x = np.maximum(np.asarray(Y, dtype=np.float64), 0.0) / wt
    s = x.sum()
    x = x / s if s > 0 else x
    x = x + XFLOOR
    return x / x.sum()


def mixture_averaged(T, P, Y, wt, dfits):
    """D_km [KK][n] as ckmi_mixture_diffusion (Y [KK][n])."""
    T = np.atleast_1d(T)
    Dall = binary_from_fits(T, P, dfits)
    Y = np.asarray(Y, dtype=np.float64).reshape(len(wt), len(T))
    out = np.zeros_like(Y)
    for s in range(len(T)):
        X = floored_mole_fractions(Y[:, s], wt)
        wbar = X @ wt
        for k in range(len(wt)):
            o = np.arange(len(wt)) != k
            out[k, s] = (X[o] @ wt[o]) / (wbar * np.sum(X[o] / Dall[s][k, o]))
    return out


def l_matrix(T, P, X, wt, Dbin, dtype=np.float64):
    """L_ij = 16 T / (25 P) sum_k X_k / (W_i D_ik) {W_j X_j (1 - d_ik) - W_i X_i (d_ij - d_jk)}, the defining
    triple sum (TRANLIB MCMDIF's L00,00 block), vectorised over k."""
    X = np.asarray(X, dtype=dtype)
    W = np.asarray(wt, dtype=dtype)
    Dm = np.asarray(Dbin, dtype=dtype)
    KK = len(W)
    I = np.eye(KK, dtype=dtype)
    A = X[None, :] / (W[:, None] * Dm)  # A[i, k] = X_k / (W_i D_ik)
    t1 = (A * (1 - I)).sum(axis=1)[:, None] * (W * X)[None, :]              # sum_k A_ik (1 - d_ik) W_j X_j
    t2 = (W * X)[:, None] * (A.sum(axis=1)[:, None] * I - A)                 # W_i X_i (d_ij sum_k A_ik - A_ij)
    L = dtype(16.0) * dtype(T) / (dtype(25.0) * dtype(P)) * (t1 - t2)
    return L


def _d_from_p(T, P, X, wt, p, dtype=np.float64):
    wbar = np.asarray(X, dtype=dtype) @ np.asarray(wt, dtype=dtype)
    cf = dtype(16.0) * dtype(T) / (dtype(25.0) * dtype(P))
    D = np.asarray(X, dtype=dtype)[:, None] * cf * wbar / np.asarray(wt, dtype=dtype)[None, :] * (p - np.diag(p)[:, None])
    np.fill_diagonal(D, 0.0)
    return D


def multicomponent_state(T, P, X, wt, Dbin):
    """D_ij [KK][KK] of one state from floored mole fractions X and the binary matrix at (T, P): np.linalg.inv."""
    L = l_matrix(T, P, X, wt, Dbin)
    return _d_from_p(T, P, X, wt, np.linalg.inv(L))


def multicomponent(T, P, Y, wt, dfits):
    """[n][KK][KK] as ckmi_multicomponent_diffusion (Y [KK][n])."""
    T = np.atleast_1d(T)
    P = np.atleast_1d(P)
    Dall = binary_from_fits(T, P, dfits)
    Y = np.asarray(Y, dtype=np.float64).reshape(len(wt), len(T))
    return np.stack([multicomponent_state(T[s], P[s], floored_mole_fractions(Y[:, s], wt), wt, Dall[s])
                     for s in range(len(T))])


def gauss_jordan_inverse(A):
    """Inverse by Gauss-Jordan with partial (row) pivoting, in the dtype of A (np.longdouble for the error
    measurement)."""
    A = A.copy()
    n = A.shape[0]
    B = np.eye(n, dtype=A.dtype)
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if p != c:
            A[[c, p]] = A[[p, c]]
            B[[c, p]] = B[[p, c]]
        piv = A[c, c]
        A[c] = A[c] / piv
        B[c] = B[c] / piv
        f = A[:, c].copy()
        f[c] = 0
        A -= np.outer(f, A[c])
        B -= np.outer(f, B[c])
    return B


def multicomponent_longdouble(T, P, X, wt, Dbin):
    """The matrix of multicomponent_state with L assembled and inverted in np.longdouble (from the same float64
    inputs), returned as longdouble."""
    ld = np.longdouble
    L = l_matrix(T, P, X, wt, Dbin, dtype=ld)
    return _d_from_p(T, P, X, wt, gauss_jordan_inverse(L), dtype=ld)


def reference_error(T, P, X, wt, Dbin):
    """Element-wise error of the float64 restatement against the longdouble elimination, relative to max |D|."""
    D = multicomponent_state(T, P, X, wt, Dbin)
    Dl = multicomponent_longdouble(T, P, X, wt, Dbin)
    return float(np.max(np.abs(D.astype(np.longdouble) - Dl)) / np.max(np.abs(Dl)))


def mass_conservation_residual(D, wt):
    """Mass conservation: v_j = W_j sum_k W_k D_kj is the same for all j (then the diffusive mass fluxes
    sum_k W_k X_k V_k vanish for every d with sum d = 0); returns max |v - mean v| / max |v|."""
    v = np.asarray(wt) * (np.asarray(wt) @ D)
    return float(np.max(np.abs(v - v.mean())) / np.max(np.abs(v)))


def stefan_maxwell_residual(D, X, wt, Dbin, d):
    """V_i = -(1 / (X_i Wbar)) sum_j W_j D_ij d_j for a d with sum d = 0 must satisfy
    sum_{j != i} X_i X_j (V_i - V_j) / D_ij = d_i; returns max |lhs - d| / max |d|."""
    wt = np.asarray(wt)
    wbar = X @ wt
    V = -(D @ (wt * d)) / (X * wbar)
    XX = np.outer(X, X) / Dbin
    np.fill_diagonal(XX, 0.0)
    lhs = XX.sum(axis=1) * V - XX @ V
    return float(np.max(np.abs(lhs - d)) / np.max(np.abs(d)))
