"""The numpy restatement of the equilibrium solver (tests/equilibrium_reference.py) against the reference's
three equilibrium goldens, and the iteration counts that the kernel's cap of 200 rests on.  CPU only."""
import numpy as np
import pytest

from conftest import P_ATM, golden, within
from equilibrium_reference import EquilibriumReference, _Y_of, edge_states, robustness_grid


@pytest.fixture(scope="module")
def eq(mech):
    return EquilibriumReference(mech)


def premixed_Y(mech):
    """equilibriumcomposition.py:50-62: fuel X CH4/H2 = 0.8/0.2, air Y O2/N2 = 0.23/0.77, 1 : 17.19 by mass."""
    Yf = _Y_of(mech, {"CH4": 0.8, "H2": 0.2})
    Ya = np.zeros(mech.KK)
    Ya[mech.species.index("O2")], Ya[mech.species.index("N2")] = 0.23, 0.77
    return (Yf + 17.19 * Ya) / 18.19


def test_hp_golden(eq, mech):
    """adiabaticflametemperature.baseline: CH4/O2 at 295.15 K, 1 atm, phi = 0.5..1.6, option 5 (P and H)."""
    g = golden("adiabaticflametemperature")
    Y = np.stack([_Y_of(mech, {"CH4": phi, "O2": 2.0}) for phi in g["state-equivalence_ratio"]])
    r = eq.solve(np.full(len(Y), 5), 295.15, P_ATM, Y)
    assert np.all(r["status"] == 0)
    err = np.max(np.abs(r["T"] / np.asarray(g["state-temperature"]) - 1))
    print("HP golden: max |T / T_gold - 1| =", err, "iterations", r["iterations"].tolist())
    assert err < 1e-7


def test_tp_golden(eq, mech):
    """equilibriumcomposition.baseline: NO [ppm] at 1 atm, 500..2480 K, every point cold-started."""
    g = golden("equilibriumcomposition")
    Ts = np.asarray(g["state-temperature"])
    r = eq.solve(np.ones(Ts.size, int), Ts, P_ATM, premixed_Y(mech))
    assert np.all(r["status"] == 0)
    no = r["X"][:, mech.species.index("NO")] * 1e6
    gold = np.asarray(g["species-NO_mole_fraction"])
    assert np.all(within(no, gold, *g["tolerance-frac"]))
    big = gold > 1.0
    err = np.max(np.abs(no[big] / gold[big] - 1))
    print("TP golden: max relative NO error above 1 ppm =", err, "max iterations", r["iterations"].max())
    assert err < 1e-7


def test_cj_golden(eq, mech):
    """multiplemechanisms.baseline (:59-65,114): X CH4/O2/N2 = 0.1/0.21/0.79, 1000 K, 1 atm, detonation()."""
    g = golden("multiplemechanisms")
    r = eq.solve([10], 1000.0, P_ATM, _Y_of(mech, {"CH4": 0.1, "O2": 0.21, "N2": 0.79}))
    assert r["status"][0] == 0
    print("CJ golden: T", r["T"][0], "D [m/s]", r["detspeed"][0] / 100, "iterations", r["iterations"][0])
    assert within(r["T"], g["state-temperature_IdealGas"], *g["tolerance-var"]).all()
    assert within(r["detspeed"] / 100.0, g["state-detonation_speed_IdealGas"], *g["tolerance-var"]).all()
    assert r["sound"][0] == pytest.approx(r["detspeed"][0] * 0.55, rel=0.1)  # D V2 / V1, V2 / V1 near 0.55


def test_every_option_converges_within_100_iterations(eq, mech):
    """256 states of the robustness grid and the eight edge states: options 1..9 all converge in at most 100
    iterations, half the kernel's default cap."""
    T, P, Y = robustness_grid(mech, 256, seed=1)
    for o in range(1, 10):
        r = eq.solve(np.full(256, o), T, P, Y)
        assert np.all(r["status"] == 0), o
        assert r["iterations"].max() <= 100, (o, r["iterations"].max())
    E = edge_states(mech)
    for Tq in (300.0, 1500.0, 3000.0):
        for o in (1, 5, 7):
            r = eq.solve(np.full(len(E), o), Tq, P_ATM, E)
            assert np.all(r["status"] == 0) and r["iterations"].max() <= 100, (Tq, o, r["iterations"].tolist())


def test_constraints_hold_at_the_solution(eq, mech):
    """The two held quantities and the elements at the reference's own answers (64 states, options 1..9)."""
    T, P, Y = robustness_grid(mech, 64, seed=3)
    opt = 1 + np.arange(64) % 9
    r = eq.solve(opt, T, P, Y)
    V0, H0, U0, S0, b0 = eq.properties(T, P, Y)
    V, H, U, S, b = eq.properties(r["T"], r["P"], r["Y"])
    held = {1: "TP", 2: "TV", 3: "TS", 4: "PV", 5: "PH", 6: "PS", 7: "VU", 8: "VH", 9: "VS"}
    val = {"T": (T, r["T"]), "P": (P, r["P"]), "V": (V0, V), "H": (H0, H), "U": (U0, U), "S": (S0, S)}
    hscale = eq.properties(T, P, Y)[0] * P  # P V = n R T: the size of an energy per gram
    for i, o in enumerate(opt):
        for c in held[o]:
            a, b_ = val[c][0][i], val[c][1][i]
            scale = hscale[i] if c in "HU" else abs(a)
            assert abs(a - b_) <= 1e-10 * max(scale, abs(a)), (i, o, c, a, b_)
    assert np.max(np.abs(b - b0)) / np.max(b0) < 1e-12


def test_matches_the_oracle_tp_solver(eq, mech, oracle):
    """Cross-check against the oracle's independent TP Gibbs minimiser on five temperatures."""
    from oracle.equilibrium import TPEquilibrium

    Y = premixed_Y(mech)
    tp = TPEquilibrium(mech, oracle.thermo)
    Ts = np.array([2400.0, 2000.0, 1600.0, 1200.0, 800.0])
    r = eq.solve(np.ones(5, int), Ts, P_ATM, Y)
    for i, Tq in enumerate(Ts):
        x = tp.solve(Tq, 1.0, Y)
        m = x > 1e-12
        assert np.max(np.abs(r["X"][i][m] / x[m] - 1)) < 1e-8
