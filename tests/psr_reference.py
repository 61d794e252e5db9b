"""Independent numpy reference for the steady-state perfectly stirred reactor (test infrastructure).

Built from the CPU oracle's closed constant-pressure right-hand side (``Oracle.rhs_jac(problem=1)``)
and species thermo (``Oracle.thermo``: cp/R, h/RT): the PSR residual is that right-hand side plus the
inflow terms

    F_k = (Y_k,in - Y_k) / tau + wdot_k W_k / rho
    F_T = [ (H_in - sum_k Y_k,in h_k(T)) / tau - sum_k h_k wdot_k W_k / rho - Q / (rho V) ] / cp

with rho = P Wbar / (R T), tau given (mode 1) or tau = rho V / mdot (mode 2), and
Q = qloss + htc areaq (T - tamb) in cal/s.  ``solve`` is pseudo-transient implicit Euler with a doubling
step; a PSR root cancels the residual, so no integrator is needed to judge a GPU answer: the tests
evaluate ``residual`` at the GPU's state.
"""
import numpy as np

RU = 1.3806504e-16 * 6.02214179e23  # erg/(mol K), the oracle's gas constant (k_B N_A)
ERG_PER_CAL = 4.184e7


class PSRReference:
    def __init__(self, oracle, P, Tin, Yin, mdot, tau=None, volume=None, energy=1, qloss=0.0, htc=0.0, areaq=0.0,
                 tamb=300.0):
        assert (tau is None) != (volume is None)
        self.o = oracle
        self.wt = np.asarray(oracle.wt, dtype=np.float64)
        self.P, self.Tin, self.mdot = float(P), float(Tin), float(mdot)
        self.Yin = np.asarray(Yin, dtype=np.float64)
        self.tau_given, self.volume = tau, volume
        self.energy = energy
        self.qloss, self.htc, self.areaq, self.tamb = qloss, htc, areaq, tamb
        _, hRT, _ = oracle.thermo(self.Tin)
        self.Hin = float(np.sum(self.Yin * hRT * RU * self.Tin / self.wt))

    def rho(self, y):
        return self.P / (RU * y[0] * np.sum(y[1:] / self.wt))

    def tau(self, y):
        return self.tau_given if self.tau_given is not None else self.rho(y) * self.volume / self.mdot

    def heat_loss(self, T):
        return (self.qloss + self.htc * self.areaq * (T - self.tamb)) * ERG_PER_CAL  # erg/s

    def residual(self, y, jac=False):
        """F(y) for y = [T, Y_1..Y_KK]; with jac=True also an approximate Jacobian (the oracle's closed
        Jacobian plus the inflow terms at fixed tau), good enough for the damped iteration below."""
        y = np.asarray(y, dtype=np.float64)
        T, Y = y[0], y[1:]
        f, J = self.o.rhs_jac(y, problem=1, energy=self.energy, P0=self.P)
        tau = self.tau(y)
        F = f.copy()
        F[1:] += (self.Yin - Y) / tau
        cpR, hRT, _ = self.o.thermo(T)
        cpk, hk = cpR * RU / self.wt, hRT * RU * T / self.wt
        cp = float(np.sum(Y * cpk))
        if self.energy == 1:
            rhoV = tau * self.mdot  # = rho V in both modes
            fin = (self.Hin - float(np.sum(self.Yin * hk))) / (tau * cp)
            F[0] += fin - self.heat_loss(T) / (rhoV * cp)
        else:
            F[0] = 0.0
        if not jac:
            return F
        J = J.copy()
        J[1:, 1:] -= np.eye(Y.size) / tau
        if self.energy == 1:
            J[0, 0] += -float(np.sum(self.Yin * cpk)) / (tau * cp) - self.htc * self.areaq * ERG_PER_CAL / (rhoV * cp)
            J[0, 1:] += -(F[0] - f[0]) * cpk / cp
        else:
            J[0, :] = 0.0
        return F, J

    def scaled(self, y, F=None):
        """Largest scaled residual: tau |F_k| / (|Y_k| + 1e-6) over the species and tau |F_T| / T."""
        F = self.residual(y) if F is None else F
        tau = self.tau(y)
        return max(float(np.max(tau * np.abs(F[1:]) / (np.abs(y[1:]) + 1e-6))), tau * abs(F[0]) / y[0])

    def solve(self, T0, Y0, tol=1e-10, max_iter=400):
        """Pseudo-transient implicit Euler from the estimate (T0, Y0): y <- y + (I / dt - J)^-1 F(y), dt
        doubling after every step that lowers the scaled residual and halving otherwise.  Returns
        (y, iterations)."""
        y = np.concatenate([[float(T0)], np.asarray(Y0, dtype=np.float64)])
        dt = 0.1 * self.tau(y)
        F, J = self.residual(y, jac=True)
        res = self.scaled(y, F)
        n = y.size
        for it in range(1, max_iter + 1):
            if res <= tol:
                return y, it - 1
            dy = np.linalg.solve(np.eye(n) / dt - J, F)
            yn = y + dy
            # the physical root: a step that leaves the positive orthant is retried with a smaller dt
            ok = yn[0] > 200.0 and yn[0] < 5000.0 and np.all(yn[1:] > -1e-9)
            if ok:
                Fn, Jn = self.residual(yn, jac=True)
                rn = self.scaled(yn, Fn)
                ok = np.isfinite(rn) and (rn < res or dt < 1e3 * self.tau(y))
            if ok:
                y, F, J, res = yn, Fn, Jn, rn
                dt *= 2.0
            else:
                dt *= 0.25
        raise RuntimeError(f"PSR reference did not converge: scaled residual {res:.3e}")


def rounding_allowance(oracle, tables, P, y, tau):
    """Rounding allowance of the species residuals at the state y [T, Y]:
    64 ulp x tau W_k / rho x sum_i |nu_ki| (qf_i + qr_i).  Two FP64 evaluations of a cancelling sum
    differ by ulps of its gross terms, not of the net."""
    wt = np.asarray(oracle.wt, dtype=np.float64)
    T, Y = y[0], y[1:]
    qf, qr, _ = oracle.rates(float(T), float(P), Y)
    KK, II = wt.size, qf.size
    absnu = np.zeros((KK, II))
    for side_sp, side_nu, cnt in (("rsp", "rnu", "nr"), ("psp", "pnu", "np")):
        sp, nu, nn = np.asarray(tables[side_sp]), np.asarray(tables[side_nu]), np.asarray(tables[cnt])
        for i in range(II):
            for u in range(int(nn[i])):
                absnu[int(sp[i, u]), i] += abs(float(nu[i, u]))
    rho = P / (RU * T * np.sum(Y / wt))
    return 64.0 * 2.0 ** -52 * tau * wt / rho * (absnu @ (qf + qr))
