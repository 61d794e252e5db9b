"""Independent numpy reference for networks of steady-state PSRs with recycle streams (test infrastructure).

Built on ``psr_reference.PSRReference`` (the CPU oracle's right-hand side and thermo): the linear flow balance,
the mass-and-enthalpy mixing of streams, a Gauss-Seidel solve in the order the reactors are given, and the
COUPLED residual -- every reactor's PSR residual with its inlet rebuilt from the other reactors' states.  At a
root of the network the coupled residual cancels, so a GPU answer is judged by evaluating it at the GPU's own
states: no integrator and no tear iteration on the reference side.
"""
import numpy as np

from psr_reference import RU, PSRReference


def flow_balance(split, ext_total):
    """Through-flows of (I - F^T) mdot = mdot_ext.  split [R][R + 1]: row j is where reactor j's outflow goes (the
    last column leaves the network); ext_total [R]: the external mass flow into every reactor."""
    split = np.asarray(split, dtype=np.float64)
    R = split.shape[0]
    return np.linalg.solve(np.eye(R) - split[:, :R].T, np.asarray(ext_total, dtype=np.float64))


def h_cp_mass(oracle, T, Y):
    """Mixture enthalpy [erg/g] and cp [erg/(g K)] from the oracle's NASA-7 evaluation."""
    cpR, hRT, _ = oracle.thermo(float(T))
    wt = np.asarray(oracle.wt, dtype=np.float64)
    return float(np.sum(Y * hRT * RU * T / wt)), float(np.sum(Y * cpR * RU / wt))


def mix(oracle, streams):
    """(T, Y, mdot) of the streams [(mdot, T, Y), ...] mixed by mass and enthalpy; T by Newton on
    h(T, Y_mix) = H_mix down to a step of 1e-13 T.  One stream alone is returned as it is."""
    streams = [(float(m), float(T), np.asarray(Y, dtype=np.float64)) for m, T, Y in streams if m > 0.0]
    if not streams:
        raise ValueError("no stream to mix")
    if len(streams) == 1:
        return streams[0][1], streams[0][2], streams[0][0]
    mdot = sum(m for m, _, _ in streams)
    Y = sum(m * y for m, _, y in streams) / mdot
    H = sum(m * h_cp_mass(oracle, T, y)[0] for m, T, y in streams) / mdot
    T = sum(m * t for m, t, _ in streams) / mdot
    for _ in range(100):
        h, cp = h_cp_mass(oracle, T, Y)
        dT = (H - h) / cp
        T += dT
        if abs(dT) <= 1e-13 * T:
            return T, Y, mdot
    raise RuntimeError("the mixed temperature did not converge")


class NetworkReference:
    """One network of R PSRs.  P, tau (or volume) [R]; split [R][R + 1]; ext: for every reactor a list of
    (mdot, T, Y) external inlets; heat: for every reactor a dict of PSRReference's qloss / htc / areaq / tamb."""

    def __init__(self, oracle, P, split, ext, tau=None, volume=None, heat=None):
        self.o = oracle
        self.split = np.asarray(split, dtype=np.float64)
        self.R = self.split.shape[0]
        self.P = np.broadcast_to(np.asarray(P, dtype=np.float64), (self.R,))
        self.ext = [[(float(m), float(T), np.asarray(Y, dtype=np.float64)) for m, T, Y in e if m > 0.0] for e in ext]
        self.tau = None if tau is None else np.broadcast_to(np.asarray(tau, dtype=np.float64), (self.R,))
        self.volume = None if volume is None else np.broadcast_to(np.asarray(volume, dtype=np.float64), (self.R,))
        self.heat = heat if heat is not None else [{} for _ in range(self.R)]
        self.mdot = flow_balance(self.split, [sum(m for m, _, _ in e) for e in self.ext])
        self.feed_forward = not any(self.split[j, i] != 0.0 for i in range(self.R) for j in range(i, self.R))

    def sources(self, i, T, Y, have):
        """The streams into reactor i: its external inlets and f_ji mdot_j of every reactor j in `have`."""
        s = list(self.ext[i])
        for j in range(self.R):
            if have[j] and self.split[j, i] > 0.0:
                s.append((self.split[j, i] * self.mdot[j], T[j], Y[j]))
        return s

    def reactor(self, i, T, Y, have=None):
        """(PSRReference of reactor i with its inlet mixed from the given states, (T_in, Y_in))."""
        have = [True] * self.R if have is None else have
        Tin, Yin, _ = mix(self.o, self.sources(i, T, Y, have))
        kw = dict(self.heat[i])
        if self.tau is not None:
            kw["tau"] = float(self.tau[i])
        else:
            kw["volume"] = float(self.volume[i])
        return PSRReference(self.o, self.P[i], Tin, Yin, self.mdot[i], **kw), (Tin, Yin)

    def solve(self, Tguess, Yguess, guess_mode=None, tear=None, tear_rtol=1e-6, tear_atol=1e-8, max_sweeps=200,
              tol=1e-10, warm=False):
        """Gauss-Seidel in the order given.  The first sweep leaves out sources that have no solution yet; later
        sweeps start every reactor from its previous solution.  guess_mode[i] 1: the estimate's temperature with
        the mixed inlet's composition.  warm: the estimates are a solution of every reactor already (nothing is left
        out of the first sweep).  Converged when every tear point (every reactor when none is given) changed
        by <= tear_atol + tear_rtol |Y| and tear_rtol T over a sweep.  Returns (T, Y, sweeps, scaled change)."""
        R = self.R
        T = np.array(Tguess, dtype=np.float64)
        Y = np.array(Yguess, dtype=np.float64)
        have = [bool(warm)] * R
        guess_mode = [0] * R if guess_mode is None else guess_mode
        tear = np.asarray(tear if tear is not None and np.any(tear) else np.ones(R), dtype=bool)
        worst = 0.0
        for sweep in range(max_sweeps):
            Tp, Yp = T.copy(), Y.copy()
            for i in range(R):
                ref, (Tin, Yin) = self.reactor(i, T, Y, have)
                Y0 = Yin if (sweep == 0 and guess_mode[i] == 1) else Y[i]
                y, _ = ref.solve(T[i], Y0, tol=tol)
                T[i], Y[i] = y[0], y[1:]
                have[i] = True
            if self.feed_forward:
                return T, Y, 1, 0.0
            if sweep > 0:
                eT = np.abs(T - Tp) / (tear_rtol * np.abs(T))
                eY = np.max(np.abs(Y - Yp) / (tear_atol + tear_rtol * np.abs(Y)), axis=1)
                worst = float(np.max(np.maximum(eT, eY)[tear]))
                if worst <= 1.0:
                    return T, Y, sweep + 1, worst
        raise RuntimeError(f"the network reference did not converge: scaled tear change {worst:.3e}")

    def coupled_residual(self, T, Y):
        """For every reactor: (PSRReference at the inlet rebuilt from the given states, F, tau) with F the PSR
        residual [F_T, F_1..F_KK] at the reactor's own state."""
        out = []
        for i in range(self.R):
            ref, _ = self.reactor(i, T, Y)
            y = np.concatenate([[T[i]], Y[i]])
            out.append((ref, ref.residual(y), ref.tau(y)))
        return out

    def exits(self, T, Y):
        """[(reactor, mdot, T, Y)] of the streams that leave the network."""
        return [(i, self.split[i, -1] * self.mdot[i], T[i], Y[i]) for i in range(self.R) if self.split[i, -1] > 0.0]


def mole_fractions(Y, wt):
    x = np.asarray(Y) / np.asarray(wt)
    return x / x.sum(axis=-1, keepdims=True)
