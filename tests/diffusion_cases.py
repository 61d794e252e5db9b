"""Mechanisms, transport parameters and states of the diffusion tests (test_diffusion_host.py proves the
reference's invariants on them on the CPU, test_gpu_diffusion.py runs the kernels on them), with the numpy
reference of every state computed once per session.
"""
import functools
import os

import numpy as np

import diffusion_reference as dr
import mechanism_variants as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAN = os.path.join(ROOT, "data", "grimech30_transport.dat")
P_ATM = dr.P_ATM
BATCHES = (1, 63, 64, 65, 130)  # the edges of a 64-lane block and of one state per wave
# name -> KK: wave kernels <16>, <56>, <64> (exactly full) and the workgroup path at its first size and at 161
MECHS = {"h2": 10, "gri": 53, "gri64": 64, "gri65": 65, "big161": 161}


@functools.lru_cache(maxsize=None)
def mechanism(name):
    from pychemkin_amd.mechanism import Mechanism

    if name == "h2":
        return mv.subset_mechanism(mv.H2_SPECIES, ("O", "H", "N", "AR"))
    if name == "gri":
        return Mechanism.from_files(mv.CHEM, mv.THERM)
    if name == "big161":
        return Mechanism.from_files(os.path.join(mv.DATA, "gri30_tracer161_chem.inp"),
                                    os.path.join(mv.DATA, "gri30_tracer161_thermo.dat"))
    return mv.tracer_mechanism(int(name[3:]) - mv.KK_GRI)


@functools.lru_cache(maxsize=None)
def transport_params(name):
    """[KK][6] TRANLIB parameters; every species outside GRI-3.0's transport file (the argon tracers) gets
    argon's record."""
    from pychemkin_amd import transport

    data = transport.parse_transport_text(open(TRAN).read())
    return np.array([data.get(s.upper(), data["AR"]) for s in mechanism(name).species], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def native_fits(name):
    from pychemkin_amd import transport

    return transport.diffusion_fits(mechanism(name).wt, transport_params(name))


def _Y(mech, moles):
    X = np.zeros(mech.KK)
    for k, v in moles.items():
        X[mech.species.index(k)] = v
    Y = X * mech.wt
    return Y / Y.sum()


def traces_Y(mech, seed=3):
    """8 major species, 12 traces with X between 1e-9 and 1e-3, the rest exactly 0 (fewer of each on a small
    mechanism): the composition on which elimination without row pivoting fails."""
    rng = np.random.default_rng(seed)
    KK = mech.KK
    nm = min(8, max(2, KK // 3))
    nt = min(12, KK - nm - 1)
    idx = rng.permutation(KK)
    X = np.zeros(KK)
    X[idx[:nm]] = rng.uniform(0.05, 1.0, nm)
    X[idx[nm:nm + nt]] = 10.0 ** rng.uniform(-9.0, -3.0, nt)
    assert np.count_nonzero(X) == nm + nt < KK
    Y = X * mech.wt
    return Y / Y.sum()


@functools.lru_cache(maxsize=None)
def states(name):
    """(labels, T [6], P [6], Y [KK][6]) of one mechanism."""
    mech = mechanism(name)
    ch4 = "CH4" in mech.species
    fresh = _Y(mech, {"CH4": 1.0, "O2": 2.0, "N2": 7.52} if ch4 else {"H2": 2.0, "O2": 1.0, "N2": 3.76})
    burnt = _Y(mech, {"CO2": 1.0, "H2O": 2.0, "N2": 7.52} if ch4 else {"H2O": 2.0, "N2": 3.76})
    neg = burnt.copy()  # integrator-style undershoots on species that are absent
    absent = np.nonzero(burnt == 0.0)[0]
    neg[absent[:3]] = [-1e-14, -3e-11, -2e-9][:len(absent[:3])]
    if "AX1" in mech.species:  # the species next to the padding of a size variant takes part
        fresh = 0.9 * fresh
        fresh[mech.species.index("AX1")] += 0.05
        fresh[mech.KK - 1] += 0.05
    rows = [("fresh 300 K 1 atm", 300.0, 1.0, fresh),
            ("burnt 2200 K 20 atm", 2200.0, 20.0, burnt),
            ("pure N2", 1000.0, 1.0, _Y(mech, {"N2": 1.0})),
            ("majors + traces + zeros", 1500.0, 5.0, traces_Y(mech)),
            ("negative traces", 1800.0, 10.0, neg),
            ("fresh 3500 K", 3500.0, 1.0, fresh)]
    return ([r[0] for r in rows], np.array([r[1] for r in rows]), np.array([r[2] for r in rows]) * P_ATM,
            np.stack([r[3] for r in rows], axis=1))


def batch(name, n):
    """The six states repeated cyclically to n states: (index into the six, T [n], P [n], Y [KK][n])."""
    _, T, P, Y = states(name)
    idx = np.arange(n) % len(T)
    return idx, T[idx].copy(), P[idx].copy(), np.ascontiguousarray(Y[:, idx])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The numpy restatement on the native fit table for the six states: dict(binary [6][KK][KK], mixture [KK][6],
    multi [6][KK][KK], X [6][KK], mass [6], sm [6], err [6], d [6][KK]) -- the mass-conservation and Stefan-Maxwell
    residuals of the float64 reference and its element-wise error against the longdouble elimination."""
    mech = mechanism(name)
    wt = mech.wt
    _, T, P, Y = states(name)
    f = native_fits(name)
    Db = dr.binary_from_fits(T, P, f)
    out = dict(binary=Db, mixture=dr.mixture_averaged(T, P, Y, wt, f), multi=dr.multicomponent(T, P, Y, wt, f),
               X=np.stack([dr.floored_mole_fractions(Y[:, s], wt) for s in range(len(T))]))
    rng = np.random.default_rng(17)
    d = rng.standard_normal((len(T), mech.KK))
    out["d"] = d - d.mean(axis=1, keepdims=True)
    out["mass"] = np.array([dr.mass_conservation_residual(out["multi"][s], wt) for s in range(len(T))])
    out["sm"] = np.array([dr.stefan_maxwell_residual(out["multi"][s], out["X"][s], wt, Db[s], out["d"][s])
                          for s in range(len(T))])
    out["err"] = np.array([dr.reference_error(T[s], P[s], out["X"][s], wt, Db[s]) for s in range(len(T))])
    for v in out.values():
        v.setflags(write=False)
    return out
