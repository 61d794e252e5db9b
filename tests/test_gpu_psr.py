"""Batched steady-state PSRs on the GPU (ckmi_psr_run, BatchPSR, the stirreactors drop-ins), judged with
the numpy reference of tests/psr_reference.py: the PSR right-hand side cancels at a root, so the
reference residual is evaluated AT THE GPU'S STATE -- no integrator on the reference side.

Steady-state rule 1e-8 / 1e-14, integrator tolerances 1e-8 / 1e-14, GRI-3.0 CH4/air, 300 K inlet, 1 atm.

Measured on an MI355X (13-reactor S-curve batch): reference residual at the GPU states 0.26-0.86 of the
rule (rounding allowance at most 0.21 of it), T within 1e-11 and species within 7e-9 relative of the
reference roots, sum Y = 1 within 3e-16.
"""
import os

import numpy as np
import pytest

from conftest import P_ATM, ROOT, THERM, ch4_air_Y, gpu_available
from psr_reference import ERG_PER_CAL, RU, PSRReference, rounding_allowance

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

SS_RTOL, SS_ATOL = 1e-8, 1e-14
TOL = dict(ss_rtol=SS_RTOL, ss_atol=SS_ATOL, rtol=1e-8, atol=1e-14)
TIN, MDOT = 300.0, 1.0
# (tau, estimate): five residence times from the burnt estimate and the cold estimate, twice, plus the unburnt
# 1700 K estimate that blows out under time marching: 13 reactors, one more than a workgroup's 12 waves
CASES = [(1e-2, "burnt"), (1e-3, "burnt"), (3e-4, "burnt"), (1e-4, "burnt"), (1e-5, "burnt"), (1e-3, "cold")]
BATCH = CASES + CASES + [(1e-3, "unburnt1700")]


def _check_rule(ref, oracle, tables, T, Y, tau, label):
    """The reference residual at the GPU state meets the steady-state rule plus the rounding allowance."""
    y = np.concatenate([[T], Y])
    F = ref.residual(y)
    lim = SS_RTOL * np.abs(Y) + SS_ATOL + rounding_allowance(oracle, tables, ref.P, y, tau)
    worst = float(np.max(tau * np.abs(F[1:]) / lim))
    worst_T = tau * abs(F[0]) / (SS_RTOL * T)
    print(f"{label}: species residual / limit {worst:.3e}, temperature residual / limit {worst_T:.3e}")
    assert worst <= 1.0 and worst_T <= 1.0, (label, worst, worst_T)


def _check_root(yref, T, Y, label):
    big = yref[1:] > 1e-6
    dT, dY = abs(T / yref[0] - 1.0), float(np.max(np.abs(Y[big] / yref[1:][big] - 1.0)))
    print(f"{label}: |T / Tref - 1| {dT:.3e}, max |Y / Yref - 1| over Y > 1e-6 {dY:.3e}")
    assert dT <= 1e-6 and dY <= 1e-5, (label, dT, dY)


def _h_cp(oracle, T, Y):
    cpR, hRT, _ = oracle.thermo(float(T))
    return float(np.sum(Y * hRT * RU * T / oracle.wt)), float(np.sum(Y * cpR * RU / oracle.wt))


@pytest.fixture(scope="module")
def scurve(chem, mech, oracle):
    """The shared S-curve batch: inlet, burnt estimate (CPU oracle), the GPU result and the reference roots."""
    import pychemkin_amd as ck

    Yin = ch4_air_Y(mech, 1.0)[0]
    r, Yb = oracle.reactor(1600.0, P_ATM, 1.0, Yin, problem=1, energy=1, t_end=1e-2, atol=1e-12, rtol=1e-8)
    assert r.status == 0
    est = {"burnt": (r.T, Yb), "cold": (TIN, Yin), "unburnt1700": (1700.0, Yin)}
    taus = np.array([c[0] for c in BATCH])
    Tg = np.array([est[c[1]][0] for c in BATCH])
    Yg = np.stack([est[c[1]][1] for c in BATCH])
    batch = ck.BatchPSR(chem, devices=[0], **TOL)
    res = batch.run(TIN, P_ATM, MDOT, tau=taus, Yin=Yin, estimate="given", T_estimate=Tg, Y_estimate=Yg)
    roots = {}
    for tau, e in set(BATCH):
        roots[(tau, e)] = PSRReference(oracle, P_ATM, TIN, Yin, MDOT, tau=tau).solve(*est[e])[0]
    return dict(Yin=Yin, burnt=(r.T, Yb), res=res, roots=roots, batch=batch, taus=taus)


def test_s_curve(scurve, chem, mech, oracle, tables):
    res, Yin = scurve["res"], scurve["Yin"]
    print("status", res.status.tolist(), "steps", res.stats[:, 0].tolist(), "resid", res.resid.tolist())
    assert res.status.tolist() == [0] * len(BATCH)
    assert np.all(res.resid <= 1.0) and np.all(np.isfinite(res.T)) and np.all(np.isfinite(res.Y))
    for i, (tau, e) in enumerate(BATCH):
        ref = PSRReference(oracle, P_ATM, TIN, Yin, MDOT, tau=tau)
        _check_rule(ref, oracle, tables, res.T[i], res.Y[i], tau, f"reactor {i} tau {tau} {e}")
        _check_root(scurve["roots"][(tau, e)], res.T[i], res.Y[i], f"reactor {i} tau {tau} {e}")
        assert res.tau[i] == tau and abs(res.volume[i] * res.rho[i] / (tau * MDOT) - 1.0) < 1e-14
    # the branches: ignited for tau >= 1e-4 s, blown out at 1e-5 s, cold stays cold, and the unburnt 1700 K
    # estimate blows out under time marching
    assert np.all(res.T[:4] > 1700.0) and np.all(np.diff(res.T[:4]) < 0.0)
    assert abs(res.T[4] - TIN) < 1e-6 and res.T[5] == TIN and abs(res.T[12] - TIN) < 1e-6
    # the second copy of the six cases ran in other waves (and through the work queue): same answers
    assert np.array_equal(res.T[:6], res.T[6:12]) and np.array_equal(res.Y[:6], res.Y[6:12])
    # a batch of 1
    Tb, Yb = scurve["burnt"]
    one = scurve["batch"].run(TIN, P_ATM, MDOT, tau=1e-3, Yin=Yin, estimate="given", T_estimate=Tb, Y_estimate=Yb)
    assert one.status.tolist() == [0] and one.T[0] == res.T[1] and np.array_equal(one.Y[0], res.Y[1])


def test_invariants(scurve, mech, oracle):
    """Checks that need no reference solution: element content, enthalpy balance and sum Y."""
    res, Yin = scurve["res"], scurve["Yin"]
    ncf = np.asarray(mech.ncf, dtype=np.float64)
    Hin, _ = _h_cp(oracle, TIN, Yin)
    for i in range(len(BATCH)):
        Y, T = res.Y[i], res.T[i]
        # |sum_k a_mk (Y_k - Y_k,in) / W_k| <= sum_k a_mk (ss_rtol |Y_k| + ss_atol) / W_k: exact from the rule
        drift = np.abs(ncf @ ((Y - Yin) / mech.wt))
        bound = ncf @ ((SS_RTOL * np.abs(Y) + SS_ATOL) / mech.wt)
        h, cp = _h_cp(oracle, T, Y)
        print(f"reactor {i}: element drift / bound {np.max(drift / bound):.3e}, "
              f"enthalpy defect / (ss_rtol T cp) {abs(h - Hin) / (SS_RTOL * T * cp):.3e}, sum Y - 1 {Y.sum() - 1:.3e}")
        assert np.all(drift <= bound)
        assert abs(h - Hin) <= SS_RTOL * T * cp          # adiabatic: h(T, Y) = H_in
        assert abs(Y.sum() - 1.0) <= 1e-12


def test_modes(scurve, chem, mech, oracle, tables):
    import pychemkin_amd as ck

    res, Yin = scurve["res"], scurve["Yin"]
    Tb, Yb = scurve["burnt"]
    given = dict(Yin=Yin, estimate="given", T_estimate=Tb, Y_estimate=Yb)
    # volume given == residence time given at the tau it reports
    V = float(res.volume[1])
    rv = ck.BatchPSR(chem, mode="volume", devices=[0], **TOL).run(TIN, P_ATM, MDOT, volume=V, **given)
    assert rv.status.tolist() == [0] and rv.volume[0] == V
    assert abs(rv.tau[0] - rv.rho[0] * V / MDOT) <= 1e-15 * rv.tau[0]
    ra = scurve["batch"].run(TIN, P_ATM, MDOT, tau=float(rv.tau[0]), **given)
    _check_root(np.concatenate([[ra.T[0]], ra.Y[0]]), rv.T[0], rv.Y[0], "volume given vs residence time given")
    _check_rule(PSRReference(oracle, P_ATM, TIN, Yin, MDOT, volume=V), oracle, tables, rv.T[0], rv.Y[0],
                float(rv.tau[0]), "volume given")
    # fixed temperature: T stays, the species meet the rule
    rt = ck.BatchPSR(chem, energy="TGIV", devices=[0], **TOL).run(TIN, P_ATM, MDOT, tau=1e-3, Yin=Yin, estimate="given",
                                                                  T_estimate=1800.0, Y_estimate=Yb)
    assert rt.status.tolist() == [0] and rt.T[0] == 1800.0
    _check_rule(PSRReference(oracle, P_ATM, TIN, Yin, MDOT, tau=1e-3, energy=2), oracle, tables, 1800.0, rt.Y[0], 1e-3,
                "fixed temperature")
    # heat loss: the enthalpy balance h - H_in + Q / mdot = 0 holds with Q, and the reactor is colder
    Hin, _ = _h_cp(oracle, TIN, Yin)
    for kw in (dict(qloss=50.0), dict(htc=1e-3, areaq=100.0, tamb=320.0)):
        rq = ck.BatchPSR(chem, devices=[0], **TOL, **kw).run(TIN, P_ATM, MDOT, tau=1e-3, **given)
        assert rq.status.tolist() == [0]
        T = rq.T[0]
        Q = (kw.get("qloss", 0.0) + kw.get("htc", 0.0) * kw.get("areaq", 0.0) * (T - kw.get("tamb", 300.0))) * ERG_PER_CAL
        h, cp = _h_cp(oracle, T, rq.Y[0])
        print(f"{kw}: T {T:.3f} K, enthalpy defect / (ss_rtol T cp) {abs(h - Hin + Q / MDOT) / (SS_RTOL * T * cp):.3e}")
        assert Q > 0.0 and abs(h - Hin + Q / MDOT) <= SS_RTOL * T * cp
        assert T < res.T[1] - 10.0
        _check_rule(PSRReference(oracle, P_ATM, TIN, Yin, MDOT, tau=1e-3, **kw), oracle, tables, T, rq.Y[0], 1e-3, str(kw))


def test_two_inlets_equal_the_premixed_inlet(chem, mech, scurve):
    import pychemkin_amd as ck
    from pychemkin_amd.stirreactors import PSR_SetResTime_EnergyConservation as PSR

    def stream(phi, T, mdot, label):
        s = ck.Stream(chem, label=label)
        s.pressure, s.temperature, s.Y, s.mass_flowrate = P_ATM, T, ch4_air_Y(mech, phi)[0], mdot
        return s

    a, b = stream(0.8, 300.0, 0.6, "a"), stream(1.3, 600.0, 0.4, "b")
    Tb, Yb = scurve["burnt"]
    est = ck.Mixture(chem)
    est.pressure, est.temperature, est.Y = P_ATM, Tb, Yb
    two = PSR(est, label="two")
    two.set_inlet(a)
    two.set_inlet(b)
    Tm, Ym, mm = two.effective_inlet()
    assert 300.0 < Tm < 600.0 and mm == 1.0
    # the host mixing agrees with the device-thermo adiabatic mixing (which stops within 0.1 K)
    assert abs(ck.adiabatic_mixing([(a, 0.6), (b, 0.4)], "mass").temperature - Tm) <= 0.1
    pre = ck.Stream(chem, label="pre")
    pre.pressure, pre.temperature, pre.Y, pre.mass_flowrate = P_ATM, Tm, Ym, mm
    one = PSR(est, label="one")
    one.set_inlet(pre)
    sols = []
    for r in (two, one):
        r.residence_time = 1e-3
        r.steady_state_tolerances = (SS_ATOL, SS_RTOL)
        r.time_stepping_tolerances = (1e-14, 1e-8)
        assert r.run() == 0
        sols.append(r.process_solution())
    _check_root(np.concatenate([[sols[1].temperature], sols[1].Y]), sols[0].temperature, sols[0].Y, "two inlets vs premixed")
    assert sols[0].temperature > 1500.0 and sols[0].mass_flowrate == 1.0


def test_limits_and_errors(scurve, chem, big_mech):
    import pychemkin_amd as ck
    from pychemkin_amd import _native

    Yin = scurve["Yin"]
    Tb, Yb = scurve["burnt"]
    # t_max = tau from a burnt estimate: not steady yet -- status 6 and a finite state
    r = ck.BatchPSR(chem, t_max=1e-3, devices=[0], **TOL).run(TIN, P_ATM, MDOT, tau=1e-3, Yin=Yin, estimate="given",
                                                              T_estimate=Tb, Y_estimate=Yb)
    assert r.status.tolist() == [_native.RUN_NOT_STEADY] == [6]
    assert np.isfinite(r.T[0]) and np.all(np.isfinite(r.Y[0])) and r.resid[0] > 1.0
    # a cfg that asks for a closed-reactor feature is rejected (CKMI_ERR_ARG = 1)
    dm = chem.device_mechanism(0)
    args = (np.array([P_ATM]), np.array([TIN]), Yin[None], np.array([MDOT]), np.array([1e-3]), np.array([Tb]), Yb[None])
    for bad in (dict(ign_mode="TIFP"), dict(profile=([0.0, 1.0], [P_ATM, P_ATM])), dict(asteps=5),
                dict(profile2=([0.0, 1.0], [1.0, 2.0]), prof2_kind=1)):
        with pytest.raises(_native.NativeError, match=r"code 1\)"):
            dm.psr_run(_native.make_cfg(t_end=0.0, atol=1e-14, rtol=1e-8, **bad), 1, *args)
    with pytest.raises(_native.NativeError, match=r"code 1\)"):
        dm.psr_run(_native.make_cfg(t_end=0.0, atol=1e-14, rtol=1e-8), 3, *args)          # mode
    # 161 species: the workgroup kernel is out of scope (CKMI_ERR_UNSUPPORTED = 4)
    big = _native.DeviceMechanism(big_mech.to_tables(), device=0)
    Yb_big = np.zeros(big_mech.KK)
    Yb_big[big_mech.species.index("N2")] = 1.0
    with pytest.raises(_native.NativeError, match=r"code 4\).*64"):
        big.psr_run(_native.make_cfg(t_end=0.0, atol=1e-14, rtol=1e-8), 1, np.array([P_ATM]), np.array([TIN]), Yb_big[None],
                    np.array([MDOT]), np.array([1e-3]), np.array([TIN]), Yb_big[None])
    big.close()


def test_plog_mechanism(oracle, mech, scurve, tables):
    """data/gri30_plog_chem.inp runs the PLOG instantiation: one ignited reactor meets the rule."""
    from oracle.oracle import Oracle
    from pychemkin_amd import _native
    from pychemkin_amd.mechanism import Mechanism

    pmech = Mechanism.from_files(os.path.join(ROOT, "data", "gri30_plog_chem.inp"), THERM)
    porc = Oracle(pmech)
    assert pmech.species == mech.species
    Yin = scurve["Yin"]
    Tb, Yb = scurve["burnt"]
    dm = _native.DeviceMechanism(pmech.to_tables(), device=0)
    r = dm.psr_run(_native.make_cfg(t_end=0.0, atol=1e-14, rtol=1e-8), 1, np.array([P_ATM]), np.array([TIN]), Yin[None],
                   np.array([MDOT]), np.array([1e-3]), np.array([Tb]), Yb[None], ss_rtol=SS_RTOL, ss_atol=SS_ATOL)
    T, Y, st = float(r["T"].cpu()[0]), r["Y"].cpu().numpy()[0], r["stats"].cpu().numpy()[0]
    dm.close()
    assert st[6] == 0 and T > 1700.0
    _check_rule(PSRReference(porc, P_ATM, TIN, Yin, MDOT, tau=1e-3), porc, pmech.to_tables(), T, Y, 1e-3, "PLOG")


def test_dropin_phi_loop_equals_batch(chem, mech):
    """A phi loop over run() / process_solution(), shaped like the reference's PSRgas test but on GRI CH4/air
    with a burnt estimate, equals BatchPSR on the same conditions."""
    import pychemkin_amd as ck
    from pychemkin_amd.stirreactors.PSR import PSR_SetResTime_EnergyConservation as PSR

    phis = [0.8, 1.0, 1.2]
    feed = ck.Stream(chem, label="feed_1")
    feed.pressure, feed.temperature, feed.Y, feed.mass_flowrate = P_ATM, 300.0, ch4_air_Y(mech, phis[0])[0], 432.0
    sphere = PSR(feed, label="PSR_1")
    sphere.set_inlet(feed)
    sphere.residence_time = 1e-3
    sphere.steady_state_tolerances = (SS_ATOL, SS_RTOL)
    sphere.timestepping_tolerances = (1e-14, 1e-8)
    sphere.set_species_floor(-1.0e-10)
    Ts, Ys, Yins, Yests = [], [], [], []
    for phi in phis:
        feed.Y = ch4_air_Y(mech, phi)[0]
        sphere.reset_estimate_composition(feed.Y, mode="mass")
        Yins.append(feed.Y)                            # what the reactor is given (a Mixture renormalises)
        Yests.append(sphere.reactormixture.Y)
        sphere.set_estimate_conditions("HP")          # the burnt estimate
        assert sphere.run() == 0
        sol = sphere.process_solution()
        assert sol.mass_flowrate == 432.0 and sol.pressure == P_ATM
        Ts.append(sol.temperature)
        Ys.append(sol.Y)
    batch = ck.BatchPSR(chem, devices=[0], **TOL)
    Tg, Yg = batch.burnt_estimate(np.full(3, P_ATM), np.stack(Yests))
    res = batch.run(300.0, P_ATM, 432.0, tau=1e-3, Yin=np.stack(Yins), estimate="given", T_estimate=Tg, Y_estimate=Yg)
    burnt = batch.run(300.0, P_ATM, 432.0, tau=1e-3, Yin=np.stack(Yins), estimate="burnt")
    assert burnt.status.tolist() == [0, 0, 0]
    np.testing.assert_allclose(burnt.T, res.T, rtol=1e-6)     # estimate="burnt": the same branch and root
    assert res.status.tolist() == [0, 0, 0]
    assert np.all(res.T > 1700.0)
    np.testing.assert_allclose(Ts, res.T, rtol=1e-12)
    Yn = np.maximum(res.Y, 0.0)
    np.testing.assert_allclose(np.stack(Ys), Yn / Yn.sum(axis=1, keepdims=True), rtol=1e-12, atol=1e-300)
