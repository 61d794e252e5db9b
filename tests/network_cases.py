"""The reactor networks the tests share, as plain numbers (test infrastructure): the two GRI-3.0 golden networks of
the reference's examples/reactor_network scripts, and the combustor family of the batch tests."""
import numpy as np

from conftest import P_ATM, ch4_air_Y, within

GOLDEN_SPECIES = ("CH4", "CO", "NO")


def check_golden(g, mech, T, mdot, Y, label):
    """The five golden columns (T, mass flow rate, CH4 / CO / NO mole fractions), each under the golden's own
    tolerances with the project's comparator; every figure is printed before it is asserted."""
    x = np.atleast_2d(Y) / mech.wt
    X = x / x.sum(axis=1, keepdims=True)
    cols = {"state-temperature": (np.atleast_1d(T), "tolerance-var"),
            "state-mass_flow_rate": (np.atleast_1d(mdot), "tolerance-var")}
    for s in GOLDEN_SPECIES:
        cols["species-mole_fraction_" + s] = (X[:, mech.species.index(s)], "tolerance-frac")
    for key, (v, tol) in cols.items():
        ref = np.asarray(g[key])
        print(f"{label} {key}: {v.tolist()} golden {ref.tolist()} |diff| {np.abs(v - ref).tolist()}")
        assert np.all(within(v, ref, *g[tol])), (label, key, v.tolist(), ref.tolist())


def air_Y(mech):
    """ck.Air: O2 0.21, N2 0.79 by mole."""
    X = np.zeros(mech.KK)
    X[mech.species.index("O2")], X[mech.species.index("N2")] = 0.21, 0.79
    Y = X * mech.wt
    return Y / Y.sum()


def mole_Y(mech, recipe):
    X = np.zeros(mech.KK)
    for s, v in recipe:
        X[mech.species.index(s)] = v
    Y = X * mech.wt
    return Y / Y.sum()


def combustor(mech, phi=0.6, to_third=0.2, back=1.0, tau=(0.5e-3, 1.5e-3, 1.5e-3), P=10.0 * P_ATM):
    """PSRnetwork.py:131-349: mixing zone (phi = 0.6 premix 500 g/s + air 50 g/s, 650 K) -> flame zone (+ air
    100 g/s at 670 K) -> 20 % to the recirculation zone, 80 % out; the recirculation zone returns 15 % to the
    mixing zone and 85 % to the flame zone.  The family around it: `to_third` is the flame zone's fraction to the
    third zone, which returns the share `back` of its outflow (15 : 85 as above) and lets the rest out, so that
    to_third * back of the flame zone's outflow recirculates; back = 0 is a feed-forward network with two exits."""
    premix, air = ch4_air_Y(mech, phi)[0], air_Y(mech)
    ext = [[(500.0, 650.0, premix), (50.0, 650.0, air)], [(100.0, 670.0, air)], []]
    split = np.array([[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, to_third, 1.0 - to_third],
                      [0.15 * back, 0.85 * back, 0.0, 1.0 - back]])
    return dict(P=P, ext=ext, split=split, tau=np.array(tau, dtype=np.float64), premix=premix,
                T_estimate=np.array([800.0, 1600.0, 1600.0]), tear=np.array([0, 0, 1], np.int32))


COMBUSTOR_MDOT = (574.375, 812.5, 162.5)


def chain_feeds(mech):
    """PSRChain_network.py:100-127: CH4 3.275 g/s at 300 K and air 45 g/s at 550 K (mixed adiabatically into the
    premix), air 62 g/s at 550 K into reactor 2, CH4:CO2 = 0.6:0.4 (mole) 0.12 g/s at 300 K into reactor 3."""
    return dict(P=2.1 * P_ATM, fuel=(3.275, 300.0, mole_Y(mech, [("CH4", 1.0)])), air=(45.0, 550.0, air_Y(mech)),
                air2=(62.0, 550.0, air_Y(mech)), reburn=(0.12, 300.0, mole_Y(mech, [("CH4", 0.6), ("CO2", 0.4)])),
                tau=np.array([2.0e-3, 1.5e-3, 3.5e-3]),
                split=np.array([[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]))


CHAIN_MDOT = (48.275, 110.275, 110.395)
CHAIN_PREMIX_T = 512.1186


def pack_ext(ext, KK, E=None):
    """The padded [R][E] / [R][E][KK] arrays of BatchPSRNetwork.run from per-reactor lists of (mdot, T, Y)."""
    R = len(ext)
    E = max(1, max(len(e) for e in ext)) if E is None else E
    m, T, Y = np.zeros((R, E)), np.full((R, E), 300.0), np.zeros((R, E, KK))
    for i, e in enumerate(ext):
        for s, (md, t, y) in enumerate(e):
            m[i, s], T[i, s], Y[i, s] = md, t, y
    return m, T, Y
