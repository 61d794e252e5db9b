"""Batched PSR reactor networks on the GPU (ckmi_psr_network_run, BatchPSRNetwork, the ReactorNetwork drop-in).

The goldens are the reference's three GRI-3.0 network baselines.  Everything else is judged with the COUPLED
residual of tests/network_reference.py: for every reactor of a network the inlet is rebuilt with the numpy mixing
from the GPU's own reactor states and the PSR residual of tests/psr_reference.py is evaluated there -- no
integrator and no tear iteration on the reference side.  The bound on it follows from the two tolerances alone
(DESIGN.md §13):

    tau |F_k| <= ss_rtol |Y_k| + ss_atol + rounding_k + sum_{j >= i} (f_ji mdot_j / mdot_i) (tear_atol + tear_rtol |Y_j,k|)

the steady-state rule at the inlet the reactor was last solved with, plus what the tear tolerance lets the
recycled share of that inlet (the sources solved after reactor i in the sweep, all tear points here) still move;
tau |F_T| <= ss_rtol T + (|dH_in| + sum_k |dY_in,k| |h_k(T)| + 1e-11 |H_in|) / cp with dH_in, dY_in bounded the
same way (1e-11 |H_in|: the mixing's own enthalpy tolerance).

Measured on an MI355X: PSRnetwork golden met in 7 sweeps (T within 4.3e-6 relative, CH4 / CO / NO within 5.7e-8);
chain golden in one sweep (T within 2e-6, species within 3.3e-9); the batch of 70 takes 1-11 sweeps (mean 7.8),
largest coupled residual 0.997 of its bound (species) and 0.11 (temperature), |sum Y - 1| <= 4.4e-16, element
balance <= 3.1e-2 of its limit, numpy roots within 3.6e-8 in T and 6.5e-9 in mole fraction; batch independence holds
bit for bit; the nine tests take 6 s together.
"""
import numpy as np
import pytest

from conftest import P_ATM, ch4_air_Y, golden, gpu_available, within
from network_cases import (CHAIN_MDOT, COMBUSTOR_MDOT, GOLDEN_SPECIES, air_Y, chain_feeds, check_golden, combustor, pack_ext)
from network_reference import NetworkReference, h_cp_mass, mole_fractions
from psr_reference import RU, rounding_allowance

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

SS_RTOL, SS_ATOL, TEAR_RTOL, TEAR_ATOL = 1e-9, 1e-14, 1e-7, 1e-8
TOL = dict(ss_rtol=SS_RTOL, ss_atol=SS_ATOL, rtol=1e-9, atol=1e-14, tear_rtol=TEAR_RTOL, tear_atol=TEAR_ATOL)
N_BATCH = 70   # past one wave of per-network lanes, and no multiple of the PSR kernel's 12 reactors per workgroup


# ---------------------------------------------------------------------------- the residual bound
def residual_bounds(net, oracle, tables, T, Y, tols=(SS_RTOL, SS_ATOL, TEAR_RTOL, TEAR_ATOL)):
    """Per reactor: (tau |F_k| / bound_k, tau |F_T| / bound_T, bound_k [KK]) at the states (T, Y) of one network."""
    ss_rtol, ss_atol, tear_rtol, tear_atol = tols
    wt = np.asarray(oracle.wt, dtype=np.float64)
    out = []
    for i, (ref, F, tau) in enumerate(net.coupled_residual(T, Y)):
        y = np.concatenate([[T[i]], Y[i]])
        _, hRT, _ = oracle.thermo(float(T[i]))
        hk = hRT * RU * T[i] / wt
        _, cp = h_cp_mass(oracle, T[i], Y[i])
        dYin, dHin = np.zeros_like(Y[i]), 0.0
        for j in range(i, net.R):          # sources solved after reactor i: at most the tear tolerance off
            share = net.split[j, i] * net.mdot[j] / net.mdot[i]
            if share > 0.0:
                dy = tear_atol + tear_rtol * np.abs(Y[j])
                _, hRTj, _ = oracle.thermo(float(T[j]))
                _, cpj = h_cp_mass(oracle, T[j], Y[j])
                dYin += share * dy
                dHin += share * (float(np.sum(dy * np.abs(hRTj * RU * T[j] / wt))) + cpj * tear_rtol * T[j])
        bk = ss_rtol * np.abs(Y[i]) + ss_atol + rounding_allowance(oracle, tables, ref.P, y, tau) + dYin
        bT = ss_rtol * T[i] + (dHin + float(np.sum(dYin * np.abs(hk))) + 1e-11 * abs(ref.Hin)) / cp
        out.append((float(np.max(tau * np.abs(F[1:]) / bk)), tau * abs(F[0]) / bT, bk))
    return out


def _reference(oracle, c, volume=None, heat=None):
    return NetworkReference(oracle, c["P"], c["split"], c["ext"], tau=None if volume is not None else c["tau"],
                            volume=volume, heat=heat)


def _check_network(label, net, oracle, tables, mech, T, Y, tols=(SS_RTOL, SS_ATOL, TEAR_RTOL, TEAR_ATOL), late=None):
    """The coupled residual under its bound, and sum Y - 1 and the element balance under what that bound implies.
    Returns the largest fraction of the bound.  late: a list that collects the failures instead of raising at once
    (the batch test prints every network's figures before it asserts)."""
    try:
        return _check_network_now(label, net, oracle, tables, mech, T, Y, tols)
    except AssertionError as e:
        if late is None:
            raise
        late.append(str(e)[:400])
        return float("inf")


def _check_network_now(label, net, oracle, tables, mech, T, Y, tols):
    rb = residual_bounds(net, oracle, tables, T, Y, tols)
    worst = max(max(a, b) for a, b, _ in rb)
    print(f"{label}: coupled residual / bound, per reactor (species, temperature) "
          f"{[(round(a, 3), round(b, 3)) for a, b, _ in rb]}")
    assert worst <= 1.0, (label, [(a, b) for a, b, _ in rb])
    R = net.R
    b = np.array([bk.sum() for _, _, bk in rb])
    W = np.array([[net.split[j, i] * net.mdot[j] / net.mdot[i] for j in range(R)] for i in range(R)])
    dsum = np.abs(Y.sum(axis=1) - 1.0)
    lim = np.linalg.solve(np.eye(R) - W, b + 4e-16)        # d_i <= sum_k bound_ik + sum_j W_ij d_j; 4e-16: the inlets'
    print(f"{label}: |sum Y - 1| {dsum.tolist()} limit {lim.tolist()}")
    assert np.all(dsum <= lim), (label, dsum, lim)
    ncf = np.asarray(mech.ncf, dtype=np.float64)
    e_in = sum(m * (ncf @ (y / mech.wt)) for e in net.ext for m, _, y in e)
    e_out = sum(m * (ncf @ (y / mech.wt)) for _, m, _, y in net.exits(T, Y))
    e_lim = sum(net.mdot[i] * (ncf @ (rb[i][2] / mech.wt)) for i in range(R)) + 1e-15 * np.abs(e_in)
    print(f"{label}: element balance |in - out| / limit {(np.abs(e_in - e_out) / e_lim).tolist()}")
    assert np.all(np.abs(e_in - e_out) <= e_lim), (label, e_in, e_out, e_lim)
    return worst




def _stream(chem, m, T, Y, P, label=None):
    import pychemkin_amd as ck

    s = ck.Stream(chem, label=label)
    s.pressure, s.temperature, s.Y, s.mass_flowrate = P, T, Y, m
    return s


# ---------------------------------------------------------------------------- 1, 2: the goldens through the drop-in
def test_psrnetwork_golden(chem, mech):
    """PSRnetwork.py:131-349 through ReactorNetwork, tear tolerance 1e-5 as in the script."""
    from pychemkin_amd.hybridreactornetwork import ReactorNetwork
    from pychemkin_amd.stirreactors import PSR_SetResTime_EnergyConservation as PSR

    c = combustor(mech)
    P = c["P"]
    premixed = _stream(chem, *c["ext"][0][0], P)
    primary_air = _stream(chem, *c["ext"][0][1], P, label="Primary_Air")
    secondary_air = _stream(chem, *c["ext"][1][0], P, label="Secondary_Air")
    mix = PSR(premixed, label="mixing zone")
    mix.set_estimate_conditions(option="TP", guess_temp=800.0)
    mix.residence_time = 0.5e-3
    mix.set_inlet(premixed)
    mix.set_inlet(primary_air)
    flame = PSR(premixed, label="flame zone")
    flame.set_estimate_conditions(option="TP", guess_temp=1600.0)
    flame.residence_time = 1.5e-3
    flame.set_inlet(secondary_air)
    recirculation = PSR(premixed, label="recirculation zone")
    recirculation.set_estimate_conditions(option="TP", guess_temp=1600.0)
    recirculation.residence_time = 1.5e-3
    net = ReactorNetwork(chem)
    net.add_reactor(mix)
    net.add_reactor(flame)
    net.add_reactor(recirculation)
    net.add_outflow_connections(mix.label, [(flame.label, 1.0)])
    net.add_outflow_connections(flame.label, [(recirculation.label, 0.2), ("EXIT>>", 0.8)])
    net.add_outflow_connections(recirculation.label, [(mix.label, 0.15), (flame.label, 0.85)])
    net.add_tearingpoint(recirculation.label)
    net.set_tear_tolerance(1.0e-5)
    assert net.run() == 0 and net.get_network_run_status() == 0
    r = net.result
    print("PSRnetwork: sweeps", int(r.sweeps[0]), "tear residual", float(r.tear_resid[0]))
    assert r.status.tolist() == [0] and not r.feed_forward[0] and 2 <= r.sweeps[0] <= 200 and r.tear_resid[0] <= 1.0
    sol = [net.reactor_solutions[i] for i in (1, 2, 3)]
    assert np.allclose([s.mass_flowrate for s in sol], COMBUSTOR_MDOT, rtol=1e-13, atol=0)
    check_golden(golden("PSRnetwork"), mech, [s.temperature for s in sol], [s.mass_flowrate for s in sol],
                  np.stack([s.Y for s in sol]), "PSRnetwork")
    assert net.number_external_outlets == 1
    out = net.get_external_stream(1)
    assert abs(out.mass_flowrate - 650.0) <= 1e-10 and out.temperature == sol[1].temperature
    assert net.get_reactor_stream("flame zone") is net.reactor_solutions[2]


def test_chain_goldens(chem, mech):
    """PSRChain_network.py:100-200 through ReactorNetwork (one sweep), and the same chain by hand as three PSR
    objects (PSRChain_declustered.py:156-196); both against both goldens and against each other."""
    from pychemkin_amd.hybridreactornetwork import ReactorNetwork
    from pychemkin_amd.inlet import adiabatic_mixing_streams
    from pychemkin_amd.stirreactors import PSR_SetResTime_EnergyConservation as PSR

    f = chain_feeds(mech)
    P = f["P"]
    fuel, air = _stream(chem, *f["fuel"], P), _stream(chem, *f["air"], P)
    premixed = adiabatic_mixing_streams(fuel, air)
    reburn_fuel = _stream(chem, *f["reburn"], P)
    air.mass_flowrate = 62.0

    def tight(r):
        r.steady_state_tolerances = (1e-14, 1e-8)
        r.time_stepping_tolerances = (1e-14, 1e-8)
        return r

    combustor_ = tight(PSR(premixed, label="combustor"))
    combustor_.set_estimate_conditions(option="HP")
    combustor_.residence_time = 2.0e-3
    combustor_.set_inlet(premixed)
    dilution = tight(PSR(premixed, label="dilution zone"))
    dilution.residence_time = 1.5e-3
    dilution.set_inlet(air)
    reburn = tight(PSR(premixed, label="reburning zone"))
    reburn.residence_time = 3.5e-3
    reburn.set_inlet(reburn_fuel)
    net = ReactorNetwork(chem)
    net.add_reactor_list([combustor_, dilution, reburn])
    assert net.run() == 0
    r = net.result
    print("PSRChain_network: stage T", r.T[0].tolist())
    assert r.status.tolist() == [0] and r.sweeps.tolist() == [1] and r.feed_forward[0]
    assert np.allclose(r.mdot[0], CHAIN_MDOT, rtol=1e-14, atol=0) and net.number_external_outlets == 1
    out = net.get_external_stream(1)
    # by hand
    c1 = tight(PSR(premixed, label="combustor 1"))
    c1.set_estimate_conditions(option="HP")
    c1.residence_time = 2.0e-3
    c1.set_inlet(premixed)
    assert c1.run() == 0
    s1 = c1.process_solution()
    c2 = tight(PSR(s1, label="cooling zone"))
    c2.residence_time = 1.5e-3
    c2.set_inlet(air)
    c2.set_inlet(s1)
    assert c2.run() == 0
    s2 = c2.process_solution()
    c3 = tight(PSR(s2, label="reburn zone"))
    c3.residence_time = 3.5e-3
    c3.set_inlet(reburn_fuel)
    c3.set_inlet(s2)
    assert c3.run() == 0
    hand = c3.process_solution()
    for name in ("PSRChain_network", "PSRChain_declustered"):
        check_golden(golden(name), mech, out.temperature, out.mass_flowrate, out.Y, name + " (network)")
        check_golden(golden(name), mech, hand.temperature, hand.mass_flowrate, hand.Y, name + " (by hand)")
    g = golden("PSRChain_network")
    assert within(out.temperature, hand.temperature, *g["tolerance-var"])
    for s in GOLDEN_SPECIES:
        k = mech.species.index(s)
        assert within(out.X[k], hand.X[k], *g["tolerance-frac"])


# ---------------------------------------------------------------------------- 3, 4: the batch of 70
def _batch_cases(mech):
    rng = np.random.default_rng(7)
    phi = rng.uniform(0.5, 0.8, N_BATCH)
    back = rng.uniform(0.0, 1.0, N_BATCH)            # x 0.3 to the third zone: recirculation fraction 0 - 0.3
    back[11] = 0.0                                   # feed-forward: one sweep
    scale = rng.uniform(0.8, 1.5, N_BATCH)
    return [combustor(mech, phi=phi[n], to_third=0.3, back=back[n], tau=np.array([0.5e-3, 1.5e-3, 1.5e-3]) * scale[n])
            for n in range(N_BATCH)]


def _run_batch(chem, mech, cases, **kw):
    import pychemkin_amd as ck

    packed = [pack_ext(c["ext"], mech.KK) for c in cases]
    opts = dict(TOL)
    opts.update(kw)
    net = ck.BatchPSRNetwork(chem, 3, devices=[0], **opts)
    return net.run(np.array([c["P"] for c in cases])[:, None], np.stack([c["split"] for c in cases]),
                   np.stack([p[0] for p in packed]), np.stack([p[1] for p in packed]),
                   ext_Y=np.stack([p[2] for p in packed]), tau=np.stack([c["tau"] for c in cases]),
                   estimate="burnt", tear=np.stack([c["tear"] for c in cases]))


@pytest.fixture(scope="module")
def batch(chem, mech):
    cases = _batch_cases(mech)
    return cases, _run_batch(chem, mech, cases)


def test_batch_of_70(batch, oracle, tables, mech):
    cases, res = batch
    print("status", res.status.tolist(), "sweeps", res.sweeps.tolist())
    print("tear residual", res.tear_resid.tolist())
    assert res.status.tolist() == [0] * N_BATCH and np.all(res.reactor_status == 0)
    assert res.feed_forward.tolist() == [n == 11 for n in range(N_BATCH)]
    assert res.sweeps[11] == 1 and np.all(np.delete(res.sweeps, 11) >= 2) and np.all(res.tear_resid <= 1.0)
    worst, far_T, far_X, late = 0.0, 0.0, 0.0, []
    g = golden("PSRnetwork")
    for n, c in enumerate(cases):
        net = _reference(oracle, c)
        assert np.allclose(res.mdot[n], net.mdot, rtol=1e-13, atol=0)
        worst = max(worst, _check_network(f"network {n}", net, oracle, tables, mech, res.T[n], res.Y[n], late=late))
        # the numpy reference's root next to the GPU's (started at the GPU's states; gated at the golden tolerances
        # only).  1e-8: the reference's residual has a rounding floor above 1e-10 in the
        # hot reactors, so its roots are resolved to 1e-8, two decades inside the gate
        Tr, Yr, _, _ = net.solve(res.T[n], res.Y[n], tear=c["tear"], tear_rtol=1e-8, tear_atol=1e-12, tol=1e-8, warm=True)
        Xr, Xg = mole_fractions(Yr, mech.wt), mole_fractions(res.Y[n], mech.wt)
        far_T, far_X = max(far_T, float(np.max(np.abs(res.T[n] / Tr - 1.0)))), max(far_X, float(np.max(np.abs(Xg - Xr))))
        if not (np.all(within(res.T[n], Tr, *g["tolerance-var"])) and np.all(within(Xg, Xr, *g["tolerance-frac"]))):
            late.append(f"network {n}: outside the golden tolerances of the numpy root")
    print(f"largest coupled residual / bound {worst:.3e}; largest distance to the numpy roots: "
          f"|T / Tref - 1| {far_T:.3e}, |X - Xref| {far_X:.3e}; mean sweeps {res.sweeps.mean():.2f}, max {res.sweeps.max()}")
    assert not late, late


def test_batch_independence(batch, chem, mech):
    """Network 37 alone, and the first 64 and 65 networks: the same status and sweeps, bit-identical T and Y."""
    cases, res = batch
    for idx in ([37], list(range(64)), list(range(65))):
        one = _run_batch(chem, mech, [cases[i] for i in idx])
        assert one.status.tolist() == res.status[idx].tolist() and one.sweeps.tolist() == res.sweeps[idx].tolist()
        assert np.array_equal(one.T, res.T[idx]) and np.array_equal(one.Y, res.Y[idx]), len(idx)
        assert np.array_equal(one.tear_resid, res.tear_resid[idx]) and np.array_equal(one.stats, res.stats[idx])


# ---------------------------------------------------------------------------- 5: failures stay local
def test_failures_stay_local(chem, mech):
    cases = [combustor(mech, phi=0.6, to_third=0.3, back=b) for b in (0.0, 1.0, 0.0, 1.0, 0.0)]
    cases[1]["split"] = np.array([[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.15, 0.85, 0.0, 0.0]])  # no exit
    cases[2]["ext"][0][0] = (500.0, 650.0, ch4_air_Y(mech, 0.7)[0])
    res = _run_batch(chem, mech, cases, max_sweeps=2)
    print("status", res.status.tolist(), "sweeps", res.sweeps.tolist(), "tear residual", res.tear_resid.tolist())
    assert res.status.tolist() == [0, 12, 0, 10, 0]
    # the closed loop was never integrated, the recycle network stopped at the limit, the others took their one sweep
    assert res.sweeps.tolist() == [1, 0, 1, 2, 1]
    assert np.all(np.isnan(res.T[1])) and np.all(np.isnan(res.Y[1])) and np.all(res.stats[1] == 0)
    ok = [0, 2, 3, 4]
    assert np.all(np.isfinite(res.T[ok])) and np.all(np.isfinite(res.Y[ok])) and np.all(res.reactor_status[ok] == 0)
    assert res.tear_resid[3] > 1.0 and np.all(res.tear_resid[[0, 2, 4]] == 0.0)
    assert np.array_equal(res.T[0], res.T[4]) and np.array_equal(res.Y[0], res.Y[4])   # equal networks, equal bits
    assert not np.array_equal(res.T[0], res.T[2])


def test_failed_member_stops_its_network(chem, mech):
    """Status 11: the member's stats say which reactor and why; later positions of that network are not solved, and
    the other networks of the batch are not touched."""
    import pychemkin_amd as ck

    good, lost, good2 = combustor(mech, to_third=0.3, back=0.0), combustor(mech), combustor(mech)
    # the second reactor of `lost` is fed by the third alone, which comes after it: no stream reaches it in the first sweep
    lost["ext"] = [lost["ext"][0], [], [(100.0, 670.0, air_Y(mech))]]
    lost["split"] = np.array([[0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.5, 0.0, 0.5]])
    res = _run_batch(chem, mech, [good, lost, good2])
    alone = _run_batch(chem, mech, [good, good2])
    print("status", res.status.tolist(), "sweeps", res.sweeps.tolist(), "reactor status", res.reactor_status.tolist())
    assert res.status.tolist() == [0, 11, 0] and res.reactor_status[1].tolist() == [0, -1, 0] and res.sweeps[1] == 1
    assert np.isfinite(res.T[1, 0]) and np.all(np.isnan(res.T[1, 1:])) and np.all(np.isnan(res.Y[1, 1:]))
    assert np.all(np.isfinite(res.mdot[1]))
    assert np.array_equal(res.T[[0, 2]], alone.T) and np.array_equal(res.Y[[0, 2]], alone.Y)
    assert res.sweeps[[0, 2]].tolist() == alone.sweeps.tolist()
    # a member that cannot become steady (t_max of a microsecond at position 2): status 6 there, nothing after it
    m, T, Y = pack_ext(good["ext"], mech.KK)
    r = ck.BatchPSRNetwork(chem, 3, t_max=[0.0, 1e-6, 0.0], devices=[0], **TOL).run(
        good["P"], good["split"], m, T, ext_Y=Y, tau=good["tau"], estimate="burnt")
    assert r.status.tolist() == [11] and r.reactor_status[0].tolist() == [0, 6, 0] and r.sweeps.tolist() == [1]
    assert r.T[0, 0] == res.T[0, 0] and np.isfinite(r.T[0, 1]) and r.resid[0, 1] > 1.0 and np.isnan(r.T[0, 2])


# ---------------------------------------------------------------------------- 6: edges
def test_single_reactor_equals_batchpsr(chem, mech):
    import pychemkin_amd as ck

    Yin = ch4_air_Y(mech, 0.7)[0]
    P = 10.0 * P_ATM
    tol = dict(ss_rtol=SS_RTOL, ss_atol=SS_ATOL, rtol=1e-9, atol=1e-14)
    psr = ck.BatchPSR(chem, devices=[0], **tol)
    Tb, Yb = psr.burnt_estimate(np.array([P]), Yin[None])
    given = dict(estimate="given", T_estimate=Tb, Y_estimate=Yb)
    a = psr.run(650.0, P, 500.0, tau=1.5e-3, Yin=Yin, **given)
    net = ck.BatchPSRNetwork(chem, 1, devices=[0], **tol)
    b = net.run(P, [[0.0, 1.0]], [[500.0]], [[650.0]], ext_Y=Yin[None, None], tau=[1.5e-3], **given)
    assert a.status.tolist() == [0] and b.status.tolist() == [0] and b.sweeps.tolist() == [1] and b.feed_forward[0]
    assert b.T[0, 0] == a.T[0] and np.array_equal(b.Y[0, 0], a.Y[0]) and b.mdot[0, 0] == 500.0
    assert (b.rho[0, 0], b.tau[0, 0], b.volume[0, 0], b.resid[0, 0]) == (a.rho[0], a.tau[0], a.volume[0], a.resid[0])
    assert np.array_equal(b.stats[0, 0], a.stats[0]) and a.T[0] > 1500.0
    assert b.exit_streams(0)[0][:3] == (0, 500.0, a.T[0])


def test_chain_of_16(chem, mech, oracle, tables):
    import pychemkin_amd as ck

    R = 16
    Yin, air = ch4_air_Y(mech, 0.7)[0], air_Y(mech)
    P = 10.0 * P_ATM
    ext = [[(500.0, 650.0, Yin)]] + [[] for _ in range(R - 1)]
    ext[8] = [(20.0, 600.0, air)]
    split = np.zeros((R, R + 1))
    split[np.arange(R), np.arange(R) + 1] = 1.0
    m, T, Y = pack_ext(ext, mech.KK)
    net = ck.BatchPSRNetwork(chem, R, devices=[0], **TOL)
    res = net.run(P, split, m, T, ext_Y=Y, tau=np.full(R, 0.2e-3), estimate="burnt")
    print("chain of 16: T", res.T[0].tolist())
    assert res.status.tolist() == [0] and res.sweeps.tolist() == [1] and np.all(res.reactor_status == 0)
    assert np.allclose(res.mdot[0], [500.0] * 8 + [520.0] * 8, rtol=1e-14, atol=0)
    ref = NetworkReference(oracle, P, split, ext, tau=np.full(R, 0.2e-3))
    _check_network("chain of 16", ref, oracle, tables, mech, res.T[0], res.Y[0])
    with pytest.raises(ValueError):
        ck.BatchPSRNetwork(chem, 17)


def test_inlet_slots_modes_and_heat_loss(chem, mech, oracle, tables):
    import pychemkin_amd as ck

    c = combustor(mech)
    g = golden("PSRnetwork")
    base = _run_batch(chem, mech, [c])
    assert base.status.tolist() == [0]
    net = _reference(oracle, c)
    _check_network("combustor, E = 2 (the third zone has no external inlet)", net, oracle, tables, mech, base.T[0], base.Y[0])
    # three external inlets into the mixing zone (E = 3): the primary air in two halves
    c3 = combustor(mech)
    air = c3["ext"][0][1][2]
    c3["ext"][0] = [c3["ext"][0][0], (25.0, 650.0, air), (25.0, 650.0, air)]
    r3 = _run_batch(chem, mech, [c3])
    assert r3.status.tolist() == [0] and r3.sweeps.tolist() == base.sweeps.tolist()
    _check_network("combustor, E = 3", _reference(oracle, c3), oracle, tables, mech, r3.T[0], r3.Y[0])
    assert np.all(within(r3.T[0], base.T[0], *g["tolerance-var"]))
    assert np.all(within(mole_fractions(r3.Y[0], mech.wt), mole_fractions(base.Y[0], mech.wt), *g["tolerance-frac"]))
    # position 2 (the flame zone) with its volume given == residence time given at the tau it reports
    V = float(base.volume[0, 1])
    m, T, Y = pack_ext(c["ext"], mech.KK)
    rv = ck.BatchPSRNetwork(chem, 3, mode=["residence_time", "volume", "residence_time"], devices=[0], **TOL).run(
        c["P"], c["split"], m, T, ext_Y=Y, tau=c["tau"], volume=[1.0, V, 1.0], estimate="burnt", tear=c["tear"])
    assert rv.status.tolist() == [0] and rv.volume[0, 1] == V
    assert abs(rv.tau[0, 1] - rv.rho[0, 1] * V / rv.mdot[0, 1]) <= 1e-15 * rv.tau[0, 1]
    c_tau = combustor(mech, tau=(c["tau"][0], float(rv.tau[0, 1]), c["tau"][2]))
    rt = _run_batch(chem, mech, [c_tau])
    for i in range(3):          # the tolerance of test_gpu_psr.py's "volume given vs residence time given"
        big = rt.Y[0, i] > 1e-6
        dT, dY = abs(rv.T[0, i] / rt.T[0, i] - 1.0), float(np.max(np.abs(rv.Y[0, i][big] / rt.Y[0, i][big] - 1.0)))
        print(f"volume mode vs residence-time mode, reactor {i}: |T / Tref - 1| {dT:.3e}, max |Y / Yref - 1| {dY:.3e}")
        assert dT <= 1e-6 and dY <= 1e-5
    # heat loss at the second position of a feed-forward network cools that reactor and the one after it only
    ff = combustor(mech, to_third=0.3, back=0.0)
    m, T, Y = pack_ext(ff["ext"], mech.KK)
    args = (ff["P"], ff["split"], m, T)
    kw = dict(ext_Y=Y, tau=ff["tau"], estimate="burnt")
    cold = ck.BatchPSRNetwork(chem, 3, qloss=[0.0, 2.5e4, 0.0], devices=[0], **TOL).run(*args, **kw)
    warm = ck.BatchPSRNetwork(chem, 3, devices=[0], **TOL).run(*args, **kw)
    print("heat loss at position 2: T", cold.T[0].tolist(), "without", warm.T[0].tolist())
    assert cold.status.tolist() == [0] and warm.status.tolist() == [0] and cold.sweeps.tolist() == [1]
    assert cold.T[0, 0] == warm.T[0, 0] and np.array_equal(cold.Y[0, 0], warm.Y[0, 0])
    assert cold.T[0, 1] < warm.T[0, 1] - 10.0 and cold.T[0, 2] < warm.T[0, 2] - 10.0
    heat = [{}, dict(qloss=2.5e4), {}]
    _check_network("heat loss at position 2", _reference(oracle, ff, heat=heat), oracle, tables, mech, cold.T[0], cold.Y[0])
