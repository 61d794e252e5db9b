"""Batched chemical equilibrium and Chapman-Jouguet states on the GPU (ckmi_equil_run, BatchEquilibrium,
ck.equilibrium / ck.detonation / ck.calculate_equilibrium, the KINCalculateEq* shims), judged with the
reference's three equilibrium goldens and with the numpy restatement of tests/equilibrium_reference.py.

Measured on an MI355X (the 130-state batch of `batch`): the kernel and the numpy reference disagree by at most
1.77e-11 in T, P (relative) and ln x_j (x_j >= 1e-20) -- the ln x_j of a trace species; T 1.7e-13, P 6.6e-13.
The bound is ten times that (MEASURED rounds it up), for reordered sums.
"""
import ctypes as ct

import numpy as np
import pytest

from conftest import P_ATM, golden, gpu_available, within
from equilibrium_reference import RU, EquilibriumReference, _Y_of, edge_states, robustness_grid

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MEASURED = 1.8e-11          # largest kernel-vs-numpy disagreement seen
BOUND = 10 * MEASURED       # never looser than 1e-7, the bar at which the goldens are met
assert BOUND <= 1e-7


@pytest.fixture(scope="module")
def dm(tables):
    from pychemkin_amd import _native

    d = _native.DeviceMechanism(tables, device=0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def eq(mech):
    return EquilibriumReference(mech)


def gpu(dm, opt, T, P, Y, **kw):
    import torch

    r = dm.equil_run(np.asarray(opt, np.int32), np.asarray(T, np.float64), np.asarray(P, np.float64), Y, **kw)
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in r.items() if k != "_inputs"}
    o["iterations"], o["status"] = o["stats"][:, 0], o["stats"][:, 1]
    return o


def mole(mech, Y):
    x = Y / np.asarray(mech.wt)
    return x / x.sum(axis=1, keepdims=True)


def disagreement(mech, g, ref):
    """Largest |T/T' - 1|, |P/P' - 1| and |ln x - ln x'| over x' >= 1e-20."""
    X, m = mole(mech, g["Y"]), ref["X"] >= 1e-20
    with np.errstate(divide="ignore"):
        dx = np.abs(np.log(np.where(m, X, 1.0)) - np.log(np.where(m, ref["X"], 1.0)))
    return max(np.max(np.abs(g["T"] / ref["T"] - 1)), np.max(np.abs(g["P"] / ref["P"] - 1)), np.max(dx))


@pytest.fixture(scope="module")
def batch(mech, eq, dm):
    """130 states (two full waves and a 2-lane tail), options 1..9 by index: 122 of the robustness grid and
    the eight edge states; the numpy reference's answers and one launch of the kernel."""
    T, P, Y = robustness_grid(mech, 122, seed=1)
    T = np.concatenate([T, [300.0, 1500.0, 3000.0, 300.0, 1500.0, 3000.0, 300.0, 1500.0]])
    P = np.concatenate([P, np.full(8, P_ATM)])
    Y = np.concatenate([Y, edge_states(mech)])
    opt = (1 + np.arange(130) % 9).astype(np.int32)
    return dict(T=T, P=P, Y=Y, opt=opt, ref=eq.solve(opt, T, P, Y), gpu=gpu(dm, opt, T, P, Y))


def premixed_Y(mech):
    Yf = _Y_of(mech, {"CH4": 0.8, "H2": 0.2})
    Ya = np.zeros(mech.KK)
    Ya[mech.species.index("O2")], Ya[mech.species.index("N2")] = 0.23, 0.77
    return (Yf + 17.19 * Ya) / 18.19


CJ_GOLDEN_X = {"CH4": 0.1, "O2": 0.21, "N2": 0.79}


# ---------------------------------------------------------------------- goldens through the kernel
def test_hp_golden(dm, mech):
    g = golden("adiabaticflametemperature")
    Y = np.stack([_Y_of(mech, {"CH4": phi, "O2": 2.0}) for phi in g["state-equivalence_ratio"]])
    r = gpu(dm, np.full(12, 5), np.full(12, 295.15), np.full(12, P_ATM), Y)
    assert r["status"].tolist() == [0] * 12
    err = np.max(np.abs(r["T"] / np.asarray(g["state-temperature"]) - 1))
    print("HP golden on the GPU: max |T / T_gold - 1| =", err, "iterations", r["iterations"].tolist())
    assert err < 1e-7
    assert np.all(r["sound"] == 0.0) and np.all(r["detspeed"] == 0.0)


def test_tp_golden(dm, mech):
    g = golden("equilibriumcomposition")
    Ts = np.asarray(g["state-temperature"])
    r = gpu(dm, np.ones(Ts.size), Ts, np.full(Ts.size, P_ATM), np.tile(premixed_Y(mech), (Ts.size, 1)))
    assert np.all(r["status"] == 0)
    no = mole(mech, r["Y"])[:, mech.species.index("NO")] * 1e6
    gold = np.asarray(g["species-NO_mole_fraction"])
    assert np.all(within(no, gold, *g["tolerance-frac"]))
    big = gold > 1.0
    err = np.max(np.abs(no[big] / gold[big] - 1))
    print("TP golden on the GPU: max relative NO error above 1 ppm =", err, "max iterations", r["iterations"].max())
    assert err < 1e-7
    assert np.array_equal(r["T"], Ts) and np.all(r["P"] == P_ATM)   # held values come back as given


def test_cj_golden(dm, mech):
    g = golden("multiplemechanisms")
    r = gpu(dm, [10], [1000.0], [P_ATM], _Y_of(mech, CJ_GOLDEN_X)[None])
    assert r["status"][0] == 0
    print("CJ golden on the GPU: T", r["T"][0], "D [m/s]", r["detspeed"][0] / 100, "stats", r["stats"][0].tolist())
    assert within(r["T"], g["state-temperature_IdealGas"], *g["tolerance-var"]).all()
    assert within(r["detspeed"] / 100.0, g["state-detonation_speed_IdealGas"], *g["tolerance-var"]).all()


# ---------------------------------------------------------------------- against the numpy reference
def test_matches_numpy_reference(batch, mech):
    g, ref = batch["gpu"], batch["ref"]
    assert np.all(ref["status"] == 0)
    assert g["status"].tolist() == [0] * 130
    d = disagreement(mech, g, ref)
    print("kernel vs numpy reference, 130 states: largest disagreement", d, "iterations gpu / ref",
          g["iterations"].max(), ref["iterations"].max())
    assert d <= BOUND
    assert np.all(g["sound"] == 0.0) and np.all(g["detspeed"] == 0.0)


# ---------------------------------------------------------------------- shapes
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_size_does_not_change_answers(batch, dm, n):
    """The first n states alone give bitwise what they give inside the 130-state launch."""
    r = gpu(dm, batch["opt"][:n], batch["T"][:n], batch["P"][:n], batch["Y"][:n])
    for k in ("T", "P", "Y", "stats"):
        assert np.array_equal(r[k], batch["gpu"][k][:n]), (n, k)


def test_position_and_neighbours_do_not_change_answers(batch, dm):
    """A state's result is bitwise the same alone, and at another place beside other options."""
    full = batch["gpu"]
    for i in (77, 129):
        one = gpu(dm, batch["opt"][i:i + 1], batch["T"][i:i + 1], batch["P"][i:i + 1], batch["Y"][i:i + 1])
        for k in ("T", "P", "Y", "stats"):
            assert np.array_equal(one[k][0], full[k][i]), (i, k)
    perm = np.random.default_rng(5).permutation(130)
    r = gpu(dm, batch["opt"][perm], batch["T"][perm], batch["P"][perm], batch["Y"][perm])
    for k in ("T", "P", "Y", "stats"):
        assert np.array_equal(r[k], full[k][perm]), k


# ---------------------------------------------------------------------- constraints at the GPU's own state
def test_constraints_at_gpu_state(batch, eq):
    """Recomputed in numpy from the kernel's (T, P, Y): the two held quantities within 1e-10 relative, the
    elements within 1e-12 of the largest element content, sum Y = 1 within 1e-14.  H and U have an arbitrary
    zero (the elements' reference state), so their scale is max(|value|, n R T), the thermal energy."""
    g = batch["gpu"]
    T, P, Y, opt = batch["T"], batch["P"], batch["Y"], batch["opt"]
    V0, H0, U0, S0, b0 = eq.properties(T, P, Y)
    V, H, U, S, b = eq.properties(g["T"], g["P"], g["Y"])
    held = {1: "TP", 2: "TV", 3: "TS", 4: "PV", 5: "PH", 6: "PS", 7: "VU", 8: "VH", 9: "VS"}
    val = {"T": (T, g["T"]), "P": (P, g["P"]), "V": (V0, V), "H": (H0, H), "U": (U0, U), "S": (S0, S)}
    worst = 0.0
    for i, o in enumerate(opt):
        for c in held[int(o)]:
            a, c_ = val[c][0][i], val[c][1][i]
            scale = max(abs(a), P[i] * V0[i]) if c in "HU" else abs(a)
            worst = max(worst, abs(a - c_) / scale)
            assert abs(a - c_) <= 1e-10 * scale, (i, o, c, a, c_)
    el = np.max(np.abs(b - b0) / np.max(b0, axis=1, keepdims=True))
    sy = np.max(np.abs(g["Y"].sum(axis=1) - 1))
    print("constraints at the GPU states: held", worst, "elements", el, "sum Y - 1", sy)
    assert el <= 1e-12 and sy <= 1e-14


# ---------------------------------------------------------------------- CJ batch
def test_cj_batch(dm, eq, mech):
    """6 mixtures x 4 pressures in one launch: D and T against the reference inside the CJ golden's tolerance,
    sound = D V2 / V1, and the equilibrium sound speed a^2 = -V^2 (dP/dV)_S from two solves of the kernel's own
    option 9 at V (1 +- 1e-4) (the finite difference sets the 1e-5 bar)."""
    tol = golden("multiplemechanisms")["tolerance-var"]
    mixes = [({"H2": 2, "O2": 1}, 298.15), (CJ_GOLDEN_X, 1000.0), ({"CH4": 1, "O2": 2, "N2": 7.52}, 300.0),
             ({"H2": 0.02, "O2": 0.21, "N2": 0.77}, 500.0), ({"C3H8": 1, "O2": 5}, 300.0),
             ({"H2": 2, "O2": 1, "AR": 7}, 298.15)]
    press = [0.2, 1.0, 2.0, 10.0]
    Y = np.stack([_Y_of(mech, m) for m, _ in mixes for _ in press])
    T = np.array([t for _, t in mixes for _ in press])
    P = np.array([p * P_ATM for _ in mixes for p in press])
    g = gpu(dm, np.full(24, 10), T, P, Y)
    ref = eq.solve(np.full(24, 10), T, P, Y)
    assert np.all(ref["status"] == 0) and g["status"].tolist() == [0] * 24
    assert within(g["T"], ref["T"], *tol).all() and within(g["detspeed"], ref["detspeed"], *tol).all()
    print("CJ batch: max |D/D_ref - 1|", np.max(np.abs(g["detspeed"] / ref["detspeed"] - 1)), "|T/T_ref - 1|",
          np.max(np.abs(g["T"] / ref["T"] - 1)), "iterations", g["iterations"].max(), "points", g["stats"][:, 2].max())
    i2 = 4 * 0 + 1  # 2 H2 + O2 at 298.15 K, 1 atm: the textbook 2837 m/s, 18.8 atm, 3680 K
    assert abs(g["detspeed"][i2] / 100 - 2837) < 3 and abs(g["P"][i2] / P_ATM - 18.8) < 0.1 and abs(g["T"][i2] - 3680) < 3
    V1 = eq.properties(T, P, Y)[0]
    V2, _, _, S2, _ = eq.properties(g["T"], g["P"], g["Y"])
    assert np.max(np.abs(g["sound"] / (g["detspeed"] * V2 / V1) - 1)) < 1e-12
    # frozen states of the CJ composition with volume V2 (1 +- eps) and entropy S2 (secant on T), then option 9
    eps, P2 = 1e-4, {}
    nR = g["P"] * V2 / g["T"]
    for sgn in (+1, -1):
        Vt = V2 * (1 + sgn * eps)
        f = lambda Tt: eq.properties(Tt, nR * Tt / Vt, g["Y"])[3] - S2
        Ta, Tb = g["T"] * (1 - sgn * 1e-4), g["T"]
        fa, fb = f(Ta), f(Tb)
        for _ in range(8):
            Tn = Tb - fb * (Tb - Ta) / np.where(fb != fa, fb - fa, 1.0)
            Ta, fa, Tb = Tb, fb, Tn
            fb = f(Tb)
        assert np.max(np.abs(fb) / S2) < 1e-13
        r = gpu(dm, np.full(24, 9), Tb, nR * Tb / Vt, g["Y"])
        assert np.all(r["status"] == 0)
        P2[sgn] = r["P"]
    a_eq = np.sqrt(-V2 * V2 * (P2[+1] - P2[-1]) / (2 * eps * V2))
    print("CJ condition: max |sound / a_eq - 1| =", np.max(np.abs(g["sound"] / a_eq - 1)))
    assert np.max(np.abs(g["sound"] / a_eq - 1)) < 1e-5


# ---------------------------------------------------------------------- failure paths
def test_iteration_cap_reports_not_converged(batch, dm):
    from pychemkin_amd import _native

    r = gpu(dm, batch["opt"], batch["T"], batch["P"], batch["Y"], max_iter=3)
    assert r["status"].tolist() == [_native.RUN_EQ_NOT_CONVERGED] * 130 == [7] * 130
    assert r["iterations"].tolist() == [3] * 130
    assert np.all(np.isfinite(r["T"])) and np.all(np.isfinite(r["P"])) and np.all(np.isfinite(r["Y"]))
    assert np.max(np.abs(r["Y"].sum(axis=1) - 1)) < 1e-14


def test_cj_minimum_outside_the_bracket_is_not_converged(dm, eq, mech):
    """V / V1 held to [0.30, 0.50] leaves the CJ point (near 0.55) outside: the secant steps bisect towards the
    upper end and the state comes back as not converged, in the kernel as in the reference."""
    Y = _Y_of(mech, CJ_GOLDEN_X)[None]
    r = gpu(dm, [10], [1000.0], [P_ATM], Y, cj_bracket=(0.30, 0.50), cj_start=0.40)
    ref = eq.solve([10], 1000.0, P_ATM, Y, cj_vlo=0.30, cj_vhi=0.50, cj_start=0.40)
    assert r["status"].tolist() == ref["status"].tolist() == [7]
    assert r["stats"][0, 2] == ref["cj_iterations"][0] > 5
    assert np.isfinite(r["T"][0]) and np.isfinite(r["detspeed"][0])


def test_unknown_option_is_rejected(batch, dm, chem):
    import pychemkin_amd as ck
    from pychemkin_amd import _native

    for bad in (0, 11, -1):
        with pytest.raises(_native.NativeError, match="1..10"):
            dm.equil_run(np.array([1, bad], np.int32), batch["T"][:2], batch["P"][:2], batch["Y"][:2])
        with pytest.raises(ValueError, match="1..10"):
            ck.BatchEquilibrium(chem, devices=[0]).run([1, bad], 1500.0, P_ATM, Y=batch["Y"][:2])


def test_161_species_mechanism(big_mech):
    """Nothing caps the species count: 16 TP and HP states of the 161-species stand-in equal the reference."""
    from pychemkin_amd import _native

    big = _native.DeviceMechanism(big_mech.to_tables(), device=0)
    ref = EquilibriumReference(big_mech)
    T, P, _ = robustness_grid(big_mech, 16, seed=7)
    Y = np.stack([_Y_of(big_mech, {"CH4": phi, "O2": 2.0, "N2": 7.52}) for phi in np.linspace(0.5, 2.0, 16)])
    opt = np.where(np.arange(16) % 2 == 0, 1, 5)
    g, r = gpu(big, opt, T, P, Y), ref.solve(opt, T, P, Y)
    big.close()
    assert np.all(r["status"] == 0) and g["status"].tolist() == [0] * 16
    d = disagreement(big_mech, g, r)
    print("161 species: largest disagreement", d, "iterations", g["iterations"].max())
    assert d <= BOUND


# ---------------------------------------------------------------------- Python layers
def test_equilibrium_and_detonation_functions(chem, mech):
    import pychemkin_amd as ck

    g = golden("adiabaticflametemperature")
    mix = ck.Mixture(chem)
    mix.temperature, mix.pressure = 295.15, P_ATM
    mix.X = [("CH4", g["state-equivalence_ratio"][5]), ("O2", 2.0)]
    hp = ck.equilibrium(mix, 5)
    assert abs(hp.temperature / g["state-temperature"][5] - 1) < 1e-7 and hp.pressure == P_ATM
    assert abs(hp.Y.sum() - 1) < 1e-14 and mix.temperature == 295.15
    tp = mix.Find_Equilibrium()
    assert tp.temperature == 295.15 and tp.X[mech.species.index("H2O")] > 0.6
    gc = golden("multiplemechanisms")
    cj = ck.Mixture(chem)
    cj.temperature, cj.pressure = 1000.0, P_ATM
    cj.X = [(k, v) for k, v in CJ_GOLDEN_X.items()]
    speeds, burnt = ck.detonation(cj)
    assert within([burnt.temperature], gc["state-temperature_IdealGas"], *gc["tolerance-var"]).all()
    assert within([speeds[1] / 100.0], gc["state-detonation_speed_IdealGas"], *gc["tolerance-var"]).all()
    assert 0.5 < speeds[0] / speeds[1] < 0.65 and burnt.pressure > 5 * P_ATM
    # mole fractions in and out give the same state as mass fractions
    sv, x = ck.calculate_equilibrium(chem.chemID, P_ATM, 295.15, mix.X, chem.WT, "mole", "mole", EQOption=5)
    assert sv[1] == hp.temperature and sv[2] == sv[3] == 0.0
    assert np.max(np.abs(x - hp.X)) < 1e-15


def test_kin_equilibrium_entry_points(mech, eq):
    from pychemkin_amd import kin

    L = kin.bind()
    cs = ct.c_int(kin.register(mech))
    try:
        Y = _Y_of(mech, CJ_GOLDEN_X)
        X = Y / mech.wt
        X = np.ascontiguousarray(X / X.sum())
        P, T = ct.c_double(P_ATM), ct.c_double(1000.0)
        Pe, Te, snd, det = (ct.c_double(0.0) for _ in range(4))
        Xe = np.zeros(mech.KK)
        ref = eq.solve([5, 10], 1000.0, P_ATM, Y)
        for i, o in enumerate((5, 10)):
            rc = L.KINCalculateEqGasWithOption(ct.byref(cs), ct.byref(ct.c_int(o)), ct.byref(ct.c_int(0)), ct.byref(P),
                                               ct.byref(T), X, ct.byref(Pe), ct.byref(Te), ct.byref(snd), ct.byref(det), Xe)
            assert rc == 0, kin.last_error()
            assert abs(Te.value / ref["T"][i] - 1) < 1e-7 and abs(Pe.value / ref["P"][i] - 1) < 1e-7
            assert abs(Xe.sum() - 1) < 1e-14 and np.max(np.abs(Xe - ref["X"][i])) < 1e-9
            assert (det.value > 1e5 and snd.value > 5e4) if o == 10 else (det.value == snd.value == 0.0)
        assert P.value == P_ATM and T.value == 1000.0
        rc = L.KINCalculateEqGasWithOption(ct.byref(cs), ct.byref(ct.c_int(1)), ct.byref(ct.c_int(1)), ct.byref(P),
                                           ct.byref(T), X, ct.byref(Pe), ct.byref(Te), ct.byref(snd), ct.byref(det), Xe)
        assert rc == 4 and "real-gas" in kin.last_error()
        Xtp = np.zeros(mech.KK)
        assert L.KINCalculateEquil(ct.byref(cs), ct.byref(P), ct.byref(T), X, Xtp) == 0
        assert np.max(np.abs(Xtp - eq.solve([1], 1000.0, P_ATM, Y)["X"][0])) < 1e-9
        assert L.KINCalculateEquilWithOption(ct.byref(cs), ct.byref(ct.c_int(5)), ct.byref(P), ct.byref(T), X, Xtp) == 0
        assert abs(T.value / ref["T"][0] - 1) < 1e-7 and P.value == P_ATM   # T and P updated in place
        assert L.KINCalculateEquilWithOption(ct.byref(cs), ct.byref(ct.c_int(12)), ct.byref(P), ct.byref(T), X, Xtp) == 1
    finally:
        kin.release(cs.value)


@pytest.mark.skipif(not (__import__("torch").cuda.is_available() and __import__("torch").cuda.device_count() >= 2),
                    reason="needs 2 GPUs")
def test_batch_equilibrium_over_two_devices(batch, chem):
    import pychemkin_amd as ck

    one = ck.BatchEquilibrium(chem, devices=[0]).run(batch["opt"], batch["T"], batch["P"], Y=batch["Y"])
    two = ck.BatchEquilibrium(chem, devices=[0, 1]).run(batch["opt"], batch["T"], batch["P"], Y=batch["Y"])
    for k in ("T", "P", "Y", "iterations", "status"):
        assert np.array_equal(getattr(one, k), getattr(two, k)), k
    assert np.array_equal(one.T, batch["gpu"]["T"])


def test_batch_equilibrium_broadcasts(batch, chem, mech):
    import pychemkin_amd as ck

    X = mole(mech, batch["Y"][:1])[0]
    r = ck.BatchEquilibrium(chem, devices=[0]).run(5, [300.0, 400.0, 500.0], P_ATM, X=X)
    assert r.T.shape == (3,) and r.Y.shape == (3, mech.KK) and np.all(r.status == 0) and np.all(np.diff(r.T) > 0)
    assert np.all(r.iterations > 0) and np.all(r.P == P_ATM)


def test_psr_equilibrium_estimate_stays_ignited(chem, mech):
    """DESIGN.md §8's case: CH4/air phi = 1, 300 K inlet, tau = 1 ms.  The HP-equilibrium estimate lands on the
    same ignited steady state as the burnt estimate."""
    import pychemkin_amd as ck
    from conftest import ch4_air_Y

    psr = ck.BatchPSR(chem, ss_rtol=1e-8, ss_atol=1e-14, rtol=1e-8, atol=1e-14, devices=[0])
    Yin = ch4_air_Y(mech, 1.0)[0]
    a = psr.run(300.0, P_ATM, 1.0, tau=1e-3, Yin=Yin, estimate="equilibrium")
    b = psr.run(300.0, P_ATM, 1.0, tau=1e-3, Yin=Yin, estimate="burnt")
    assert a.status.tolist() == b.status.tolist() == [0]
    assert a.T[0] > 1500.0 and abs(a.T[0] / b.T[0] - 1) < 1e-6
    with pytest.raises(ValueError, match="equilibrium"):
        psr.run(300.0, P_ATM, 1.0, tau=1e-3, Yin=Yin, estimate="nonsense")
