"""Host side of the PSR reactor networks (no GPU needed): the numpy network reference against the reference's three
GRI-3.0 network goldens, the flow balance, the ReactorNetwork drop-in's surface and its errors, and the stream
utilities (adiabatic_mixing_streams, clone_stream, compare_streams, compare_mixtures)."""
import inspect

import numpy as np
import pytest

from conftest import P_ATM, _h_mass, ch4_air_Y, golden, within
from network_cases import CHAIN_MDOT, CHAIN_PREMIX_T, COMBUSTOR_MDOT, chain_feeds, check_golden, combustor, pack_ext
from network_reference import NetworkReference, flow_balance, mix
from psr_reference import PSRReference


def _burnt(oracle, P, Y):
    """The burnt estimate: adiabatic CONP closed reactor from Y at 1600 K, 10 ms (BatchPSR.burnt_estimate)."""
    r, Yb = oracle.reactor(1600.0, P, 1.0, Y, problem=1, energy=1, t_end=1e-2, atol=1e-12, rtol=1e-8)
    assert r.status == 0
    return r.T, Yb


# ---------------------------------------------------------------------------- the reference against the goldens
@pytest.fixture(scope="module")
def network_root(oracle, mech):
    c = combustor(mech)
    net = NetworkReference(oracle, c["P"], c["split"], c["ext"], tau=c["tau"])
    _, Yb = _burnt(oracle, c["P"], c["premix"])
    T, Y, sweeps, worst = net.solve(c["T_estimate"], np.tile(Yb, (3, 1)), tear=c["tear"], tear_rtol=1e-10, tear_atol=1e-14)
    return net, T, Y, sweeps


@pytest.fixture(scope="module")
def chain_root(oracle, mech):
    f = chain_feeds(mech)
    Tp, Yp, mp = mix(oracle, [f["fuel"], f["air"]])
    net = NetworkReference(oracle, f["P"], f["split"], [[(mp, Tp, Yp)], [f["air2"]], [f["reburn"]]], tau=f["tau"])
    Tb, Yb = _burnt(oracle, f["P"], Yp)
    # the combustor from the "HP" (burnt) estimate; the other two from the reference's cold estimate: the premix
    # temperature with the composition of their own inlet (run_without_tearstream)
    T, Y, sweeps, _ = net.solve([Tb, Tp, Tp], np.stack([Yb, Yp, Yp]), guess_mode=[0, 1, 1])
    return net, T, Y, sweeps, (Tp, Yp, mp)


def test_reference_meets_the_network_golden(network_root, mech):
    net, T, Y, sweeps = network_root
    print("sweeps", sweeps, "T", T.tolist())
    assert not net.feed_forward and 3 <= sweeps <= 40
    check_golden(golden("PSRnetwork"), mech, T, net.mdot, Y, "PSRnetwork")
    # a root of the coupled equations: every reactor's residual cancels with its inlet rebuilt from the others.
    # The last sweep moved Y_in by <= 1e-10 Y_in, i.e. tau F_k by as much; on the scale |Y_k| + 1e-6 of `scaled`
    # that is up to 1e-10 Y_in,k / Y_k, a few hundred times 1e-10 for the fuel in the flame zone
    for i, (ref, F, tau) in enumerate(net.coupled_residual(T, Y)):
        y = np.concatenate([[T[i]], Y[i]])
        assert ref.scaled(y, F) <= 1e-7, (i, ref.scaled(y, F))


def test_reference_meets_the_chain_goldens(chain_root, oracle, mech):
    net, T, Y, sweeps, (Tp, Yp, mp) = chain_root
    print("stage T", T.tolist())
    assert net.feed_forward and sweeps == 1
    assert abs(Tp - CHAIN_PREMIX_T) < 1e-4 and mp == 48.275
    (i, md, Te, Ye), = net.exits(T, Y)
    assert i == 2
    check_golden(golden("PSRChain_network"), mech, Te, md, Ye, "PSRChain_network")
    # the same chain by hand, one reactor after another (PSRChain_declustered.py:156-196); reactors 2 and 3 start
    # from the solution stream they are created with
    f = chain_feeds(mech)
    Tb, Yb = _burnt(oracle, f["P"], Yp)
    y1, _ = PSRReference(oracle, f["P"], Tp, Yp, mp, tau=f["tau"][0]).solve(Tb, Yb)
    T2, Y2, m2 = mix(oracle, [f["air2"], (mp, y1[0], y1[1:])])
    y2, _ = PSRReference(oracle, f["P"], T2, Y2, m2, tau=f["tau"][1]).solve(y1[0], y1[1:])
    T3, Y3, m3 = mix(oracle, [f["reburn"], (m2, y2[0], y2[1:])])
    y3, _ = PSRReference(oracle, f["P"], T3, Y3, m3, tau=f["tau"][2]).solve(y2[0], y2[1:])
    check_golden(golden("PSRChain_declustered"), mech, y3[0], m3, y3[1:], "PSRChain_declustered")
    # both routes reach the same roots (the cold and the hot estimate of reactors 2 and 3 agree)
    assert np.all(within([y1[0], y2[0], y3[0]], T, 1e-6, 1e-8))


def test_flow_balance(mech):
    c = combustor(mech)
    md = flow_balance(c["split"], [550.0, 100.0, 0.0])
    assert np.max(np.abs(md - np.array(COMBUSTOR_MDOT))) <= 1e-12 * 812.5
    f = chain_feeds(mech)
    md = flow_balance(f["split"], [48.275, 62.0, 0.12])
    assert np.max(np.abs(md - np.array(CHAIN_MDOT))) <= 1e-12 * 110.395
    # the exits carry what came in
    assert abs(c["split"][1, -1] * COMBUSTOR_MDOT[1] - 650.0) <= 1e-10


# ---------------------------------------------------------------------------- the drop-in
def _stream(chem, Y, T, mdot, P=P_ATM, label=None):
    import pychemkin_amd as ck

    s = ck.Stream(chem, label=label)
    s.pressure, s.temperature, s.Y, s.mass_flowrate = P, T, Y, mdot
    return s


def _psr(chem, est, label, tau=1e-3, inlets=()):
    from pychemkin_amd.stirreactors import PSR_SetResTime_EnergyConservation

    r = PSR_SetResTime_EnergyConservation(est, label=label)
    r.residence_time = tau
    for s in inlets:
        r.set_inlet(s)
    return r


def test_dropin_signatures():
    from pychemkin_amd import inlet, mixture
    from pychemkin_amd.hybridreactornetwork import ReactorNetwork

    want = {"__init__": ["self", "chem"], "add_reactor": ["self", "reactor"], "add_reactor_list": ["self", "reactor_list"],
            "show_reactors": ["self"], "get_reactor_label": ["self", "reactor_index"],
            "add_outflow_connections": ["self", "source_label", "outflow_split"], "clear_connections": ["self"],
            "remove_reactor": ["self", "name"], "show_internal_outflow_connections": ["self"],
            "show_internal_inflow_connections": ["self"], "add_tearingpoint": ["self", "reactor_name"],
            "remove_tearpoint": ["self", "reactor_name"], "set_tear_tolerance": ["self", "tol"],
            "set_tear_iteration_limit": ["self", "max_count"], "set_relaxation_factor": ["self", "relax"],
            "run": ["self"], "get_network_run_status": ["self"], "get_reactor_stream": ["self", "reactor_name"],
            "get_external_stream": ["self", "stream_index"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(ReactorNetwork, name)).parameters) == params, name
    assert inspect.signature(ReactorNetwork.set_tear_tolerance).parameters["tol"].default == 1.0e-6
    for prop in ("number_reactors", "number_external_outlets"):
        assert isinstance(getattr(ReactorNetwork, prop), property)
    assert list(inspect.signature(inlet.clone_stream).parameters) == ["source", "target"]
    assert list(inspect.signature(inlet.adiabatic_mixing_streams).parameters) == ["streamA", "streamB"]
    for fn in (inlet.compare_streams, mixture.compare_mixtures):
        p = inspect.signature(fn).parameters
        assert [(k, v.default) for k, v in list(p.items())[2:]] == [("atol", 1.0e-10), ("rtol", 1.0e-3), ("mode", "mass")]
    assert list(inspect.signature(inlet.compare_streams).parameters)[:2] == ["streamA", "streamB"]
    assert list(inspect.signature(mixture.compare_mixtures).parameters)[:2] == ["mixtureA", "mixtureB"]


def test_dropin_connections_and_errors(chem, mech):
    from pychemkin_amd.flowreactors.PFR import PlugFlowReactor_FixedTemperature
    from pychemkin_amd.hybridreactornetwork import ReactorNetwork
    from pychemkin_amd.reactormodel import ReactorError

    feed = _stream(chem, ch4_air_Y(mech, 0.7)[0], 600.0, 10.0, label="feed")
    a, b, c = (_psr(chem, feed, n, inlets=[feed] if n == "A" else []) for n in "ABC")
    with pytest.raises(ReactorError):
        ReactorNetwork("GRI")                                  # not a Chemistry set
    net = ReactorNetwork(chem)
    with pytest.raises(ReactorError, match="external inlet"):
        net.add_reactor(b)                                      # the first reactor needs an external inlet
    pfr_feed = _stream(chem, ch4_air_Y(mech, 0.7)[0], 600.0, 10.0)
    with pytest.raises(ReactorError, match="plug-flow members are not on this path"):
        net.add_reactor(PlugFlowReactor_FixedTemperature(pfr_feed))
    net.add_reactor_list([a, b, c])
    net.add_reactor(b)                                          # already there: ignored
    assert net.number_reactors == 3 and [net.get_reactor_label(i) for i in (1, 2, 3)] == ["A", "B", "C"]
    assert net.get_reactor_label(7) == "" and net.get_network_run_status() == -100
    # a chain without connections: through-flow i -> i + 1, the last reactor exits
    S = net.split_matrix()
    assert np.array_equal(S, [[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    assert net.number_external_outlets == 1 and net.external_outlets == {1: 3}
    assert net.inflow_sources == {2: [(1, 1.0)], 3: [(2, 1.0)]}
    # declared connections: EXIT>>, the implied through-flow, recycle
    net.add_outflow_connections("B", [("C", 0.2), ("EXIT>>", 0.8)])
    net.add_outflow_connections("C", [("A", 0.15), ("B", 0.85)])
    S = net.split_matrix()
    assert np.allclose(S, [[0, 1, 0, 0], [0, 0, 0.2, 0.8], [0.15, 0.85, 0, 0]], rtol=0, atol=1e-15)
    assert net.number_external_outlets == 1 and net.external_outlets == {1: 2}
    net.add_outflow_connections("A", [("C", 0.25)])             # the rest is the through-flow to B
    assert np.allclose(net.split_matrix()[0], [0, 0.75, 0.25, 0])
    net.show_internal_outflow_connections()
    net.show_internal_inflow_connections()
    for bad in ([("nobody", 0.5)], [("A", 0.5)], [("B", 1.5)], [("B", 0.7), ("C", 0.7)]):
        with pytest.raises(ReactorError):
            net.add_outflow_connections("A", bad)
    with pytest.raises(ReactorError):
        net.add_outflow_connections("nobody", [("A", 1.0)])
    # tear points
    net.add_tearingpoint("C")
    with pytest.raises(ReactorError, match="already"):
        net.add_tearingpoint("C")
    with pytest.raises(ReactorError, match="NOT in the network"):
        net.add_tearingpoint("nobody")
    with pytest.raises(ReactorError):
        net.remove_tearpoint("A")
    net.remove_tearpoint("C")
    assert net.numb_tearpoints == 0
    for bad in (lambda: net.set_tear_tolerance(0.0), lambda: net.set_tear_iteration_limit(0),
                lambda: net.set_relaxation_factor(-1.0)):
        with pytest.raises(ReactorError):
            bad()
    net.set_tear_tolerance(1e-5), net.set_tear_iteration_limit(50), net.set_relaxation_factor(0.8)
    assert (net.tolerance, net.max_tearloop_count, net.relaxation_factor) == (1e-5, 50, 0.8)
    # removing C takes its connections along: B's row no longer sums to 1 and run() says so before any GPU work
    net.remove_reactor("C")
    assert net.number_reactors == 2 and net.reactor_map == {"A": 1, "B": 2}
    with pytest.raises(ReactorError, match="sum to 1"):
        net.run()
    net.clear_connections()
    assert net.number_external_outlets == 0 and np.array_equal(net.split_matrix(), [[0, 1, 0], [0, 0, 1]])
    assert net.number_external_outlets == 1
    net.remove_reactor("nobody")                                # a warning, nothing else
    with pytest.raises(ReactorError, match="NOT been solved"):
        net.get_reactor_stream("A")
    with pytest.raises(ReactorError):
        net.get_external_stream(1)


def test_batch_network_validation(chem, mech):
    from pychemkin_amd import BatchPSRNetwork, NetworkResult  # noqa: F401

    c = combustor(mech)
    m, T, Y = pack_ext(c["ext"], mech.KK)
    est = dict(estimate="given", T_estimate=c["T_estimate"], Y_estimate=c["premix"])
    with pytest.raises(ValueError):
        BatchPSRNetwork(chem, 17)
    with pytest.raises(ValueError, match="tear_rtol"):
        BatchPSRNetwork(chem, 3, tear_rtol=1e-9, ss_rtol=[1e-9, 1e-8, 1e-9])
    net = BatchPSRNetwork(chem, 3)
    bad = c["split"].copy()
    bad[1, 3] = 0.8 - 1e-9
    with pytest.raises(ValueError, match="sum to 1"):
        net.run(c["P"], bad, m, T, ext_Y=Y, tau=c["tau"], **est)
    bad = c["split"].copy()
    bad[1, 2], bad[1, 3] = -0.2, 1.2
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        net.run(c["P"], bad, m, T, ext_Y=Y, tau=c["tau"], **est)
    m0 = m.copy()
    m0[0] = 0.0
    with pytest.raises(ValueError, match="first reactor"):
        net.run(c["P"], c["split"], m0, T, ext_Y=Y, tau=c["tau"], **est)
    with pytest.raises(ValueError, match="tau is required"):
        net.run(c["P"], c["split"], m, T, ext_Y=Y, **est)
    with pytest.raises(ValueError, match="T_estimate"):
        net.run(c["P"], c["split"], m, T, ext_Y=Y, tau=c["tau"], estimate="inlet")


# ---------------------------------------------------------------------------- stream utilities
def test_adiabatic_mixing_streams(chem, mech, tables):
    from pychemkin_amd.inlet import adiabatic_mixing_streams

    f = chain_feeds(mech)
    fuel = _stream(chem, f["fuel"][2], f["fuel"][1], f["fuel"][0], P=f["P"], label="fuel")
    air = _stream(chem, f["air"][2], f["air"][1], f["air"][0], P=f["P"], label="air")
    pre = adiabatic_mixing_streams(fuel, air)
    assert pre is not fuel and pre.mass_flowrate == 48.275 and pre.pressure == f["P"]
    assert abs(pre.temperature - CHAIN_PREMIX_T) < 1e-4
    np.testing.assert_allclose(pre.Y, (3.275 * fuel.Y + 45.0 * air.Y) / 48.275, rtol=1e-14, atol=1e-300)
    H = (3.275 * _h_mass(tables, fuel.Y, 300.0) + 45.0 * _h_mass(tables, air.Y, 550.0)) / 48.275
    assert abs(_h_mass(tables, pre.Y, pre.temperature) - H) <= 1e-11 * abs(H)
    assert fuel.temperature == 300.0 and fuel.mass_flowrate == 3.275          # the arguments are left alone
    import pychemkin_amd as ck

    with pytest.raises(ck.mixture.MixtureError):
        adiabatic_mixing_streams(fuel, ck.Mixture(chem))


def test_compare_and_clone_streams(chem, mech):
    import pychemkin_amd as ck
    from pychemkin_amd.inlet import clone_stream, compare_streams
    from pychemkin_amd.mixture import compare_mixtures

    a = _stream(chem, ch4_air_Y(mech, 0.8)[0], 900.0, 5.0, label="a")
    b = ck.Stream(chem, label="b")
    clone_stream(a, b)
    assert (b.temperature, b.pressure, b.mass_flowrate) == (900.0, P_ATM, 5.0) and b.label == "b"
    np.testing.assert_allclose(b.Y, a.Y, rtol=1e-14, atol=1e-300)
    same, dmax, vmax = compare_streams(a, b, atol=1e-12, rtol=1e-9)
    assert same is True and dmax <= 1e-15 and vmax <= 1e-14
    # a species off by more than both tolerances: not the same, and the maxima report it
    Y = a.Y.copy()
    k, n2 = mech.species.index("CH4"), mech.species.index("N2")
    Y[k] += 1e-4
    Y[n2] -= 1e-4
    b.Y = Y
    same, dmax, vmax = compare_mixtures(a, b, atol=1e-8, rtol=1e-6)
    assert same is False and abs(dmax - 1e-4) < 1e-12 and abs(vmax - 1e-4 / a.Y[k]) < 1e-9
    assert compare_mixtures(a, b, atol=1e-8, rtol=1e-2)[0] is True             # inside the relative tolerance
    assert compare_mixtures(a, b, atol=1e-8, rtol=1e-6, mode="mole")[0] is False
    # compare_streams joins the flow rate's verdict to the mixtures' by `or`, as the reference does: equal flow
    # rates pass, and the maxima still report the species (this is why the network's own tear test does not use it)
    same, dmax, vmax = compare_streams(a, b, atol=1e-8, rtol=1e-6)
    assert same is True and abs(dmax - 1e-4) < 1e-12 and abs(vmax - 1e-4 / a.Y[k]) < 1e-9
    b.mass_flowrate = 6.0
    assert compare_streams(a, b, atol=1e-8, rtol=1e-6) == (False, pytest.approx(1.0), pytest.approx(0.2))
    # the flow rate enters the maxima; the verdicts are joined by `or`, as in the reference
    clone_stream(a, b)
    b.mass_flowrate = 5.5
    same, dmax, vmax = compare_streams(a, b, atol=1e-8, rtol=1e-6)
    assert same is True and dmax == pytest.approx(0.5) and vmax == pytest.approx(0.1)
    # a temperature difference alone passes when the pressures agree (the reference's `or` chain), but is reported
    clone_stream(a, b)
    b.temperature = 950.0
    same, dmax, vmax = compare_mixtures(a, b, atol=1e-8, rtol=1e-6)
    assert same is True and dmax == 50.0 and vmax == pytest.approx(50.0 / 900.0)
    with pytest.raises(ck.mixture.MixtureError):
        compare_mixtures(a, ck.Mixture(chem))                                   # not fully defined
