"""The wave kernel's hot-loop paths after the instruction-level rework ("hot-loop issue"):
the lane index recomputed in the strips / solve / set-up, the A-factor slot test hoisted out of the strips,
the unpredicated wdot scatter, fexp's three-instruction clamp and the 27-store pivot row.

1. every instantiation that inherits them integrates a few reactors against the oracle at the bars of
   test_gpu_reactor.py (tau, T and major species at 1e-4), factorising at least once;
2. the A-factor perturbation with the perturbed reaction's device slot in the first strip, a middle strip
   and the falloff strip, and an unperturbed reactor of the same launch bitwise equal to a launch without
   any perturbation;
3. fexp at its edges through the generic ROP kernel.
"""
import os

import numpy as np
import pytest

from conftest import P_ATM, ROOT, THERM, ch4_air_Y, h2_air_Y
from mechanism_variants import gri_subset_text

pytestmark = pytest.mark.gpu

MAJOR = ("CH4", "O2", "N2", "H2O", "CO2", "CO", "H2")
RUN = dict(energy=1, t_end=1.0, atol=1e-10, rtol=1e-8, ign_mode="TIFP")
NST, NFE, NJE, NLU, NCF, NEF, STATUS, NNI = range(8)


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items() if hasattr(v, "cpu")}


def _check(res, ref, Yref, mech, major=MAJOR):
    st = res["stats"]
    assert np.all(st[:, NLU] >= 1), st[:, NLU]
    for i, r in enumerate(ref):
        assert st[i, STATUS] == r.status == 0, (i, st[i].tolist(), r.status)
        assert r.tau > 0 and abs(res["tau"][i] / r.tau - 1) < 1e-4, (i, res["tau"][i], r.tau)
        assert abs(res["T"][i] / r.T - 1) < 1e-4, (i, res["T"][i], r.T)
        for sp in major:
            k = mech.species.index(sp)
            assert abs(res["Y"][i, k] - Yref[i][k]) <= 1e-4 * max(abs(Yref[i][k]), 1e-3), (i, sp)


@pytest.fixture(scope="module")
def dm(tables):
    from pychemkin_amd import _native

    return _native.DeviceMechanism(tables)


@pytest.fixture(scope="module")
def mix(mech, oracle):
    """16 reactors of test_gpu_jac_single_eval.py's mix (bench.sweep_c4's grid, CONP / CONV alternating)."""
    import bench

    T0, P0, Y0, prob = bench.sweep_c4(mech, 1, 0)
    idx = 16411 * np.arange(16)
    T0, P0, Y0, prob = T0[idx], P0[idx], Y0[idx], prob[idx]
    nfail, ref, Yref = oracle.reactor_batch(T0, P0, Y0, problem=prob, V0=np.ones(16), **RUN)
    assert nfail == 0
    return dict(T0=T0, P0=P0, Y0=Y0, prob=prob, ref=list(ref), Yref=Yref)


def _run_mix(dm, mix, path, n):
    from pychemkin_amd import _native

    _native.set_reactor_path(path)
    try:
        return _np(dm.reactor_run(_native.make_cfg(**RUN), mix["prob"][:n], mix["T0"][:n], mix["P0"][:n], np.ones(n),
                                  mix["Y0"][:n]))
    finally:
        _native.set_reactor_path(0)


# ------------------------------------------------------------------ 1. every instantiation
def test_fp32_inverse_more_reactors_than_waves(dm, mix, mech):
    """reactor_kernel<54, false, false>, 16 reactors on a workgroup of 12 waves: four waves take a second
    reactor, so the recomputed lane index is used across the persistent loop."""
    _check(_run_mix(dm, mix, 3, 16), mix["ref"], mix["Yref"], mech)


def test_fp64_inverse(dm, mix, mech):
    """reactor_kernel<54, false, true>: NewtonMatrixGJ64's own solve and set-up."""
    _check(_run_mix(dm, mix, 2, 8), mix["ref"][:8], mix["Yref"][:8], mech)


H2_SPECIES = ("H2", "H", "O", "O2", "OH", "H2O", "HO2", "H2O2", "N2", "AR")


def h2_subset_text():
    """The H2 / O2 subsystem of GRI-Mech 3.0 (10 species, N = 32 variant) cut from the repository's own file:
    reactions whose species all belong to H2_SPECIES, with their LOW / TROE lines, and third-body
    efficiencies of other species dropped (the cutter is tests/mechanism_variants.py gri_subset_text)."""
    text = gri_subset_text(H2_SPECIES, ("O", "H", "N", "AR"))
    nrx = sum("=" in l.split("!")[0] for l in text.split("\n"))
    assert nrx >= 20, nrx
    return text


def test_small_mechanism_n32(tmp_path):
    """reactor_kernel<32>: the H2 / O2 subsystem (11 variables), 4 H2 / air reactors."""
    from oracle.oracle import Oracle
    from pychemkin_amd import _native
    from pychemkin_amd.mechanism import Mechanism

    path = tmp_path / "h2_subset_chem.inp"
    path.write_text(h2_subset_text())
    m = Mechanism.from_files(str(path), THERM)
    assert m.KK + 1 <= 32
    orc = Oracle(m)
    d = _native.DeviceMechanism(m.to_tables())
    cases = [(1000.0, 1.0, 1), (1100.0, 5.0, 2), (1200.0, 20.0, 1), (950.0, 2.0, 2)]
    T0 = np.array([c[0] for c in cases])
    P0 = np.array([c[1] for c in cases]) * P_ATM
    Y0 = np.tile(h2_air_Y(m), (4, 1))
    prob = np.array([c[2] for c in cases], np.int32)
    _native.set_reactor_path(3)
    try:
        res = _np(d.reactor_run(_native.make_cfg(**RUN), prob, T0, P0, np.ones(4), Y0))
    finally:
        _native.set_reactor_path(0)
    out = [orc.reactor(T0[i], P0[i], 1.0, Y0[i], problem=int(prob[i]), **RUN) for i in range(4)]
    _check(res, [o[0] for o in out], [o[1] for o in out], m, major=("H2", "O2", "N2", "H2O"))
    d.close()


def test_plog_mechanism_n64():
    """reactor_kernel<64, true, *>: the PLOG mechanism and the conditions of test_gpu_jac_single_eval.py."""
    from oracle.oracle import Oracle
    from pychemkin_amd import _native
    from pychemkin_amd.mechanism import Mechanism

    m = Mechanism.from_files(os.path.join(ROOT, "data", "gri30_plog_chem.inp"), THERM)
    orc = Oracle(m)
    d = _native.DeviceMechanism(m.to_tables())
    cases = [(1200, 1, 1.0, 1), (1400, 10, 1.0, 2), (1600, 50, 1.5, 1), (1300, 30, 0.5, 2)]
    T0 = np.array([c[0] for c in cases], float)
    P0 = np.array([c[1] for c in cases], float) * P_ATM
    Y0 = np.stack([ch4_air_Y(m, c[2])[0] for c in cases])
    prob = np.array([c[3] for c in cases], np.int32)
    res = _np(d.reactor_run(_native.make_cfg(**RUN), prob, T0, P0, np.ones(4), Y0))
    out = [orc.reactor(T0[i], P0[i], 1.0, Y0[i], problem=int(prob[i]), **RUN) for i in range(4)]
    _check(res, [o[0] for o in out], [o[1] for o in out], m)
    d.close()


def test_plug_flow_tubes(dm, oracle, mech):
    """Problem 3 (the FP64-inverse variant with plug flow compiled in), test_gpu_jac_single_eval.py's tubes."""
    from pychemkin_amd import _native

    cases = [(1300.0, 1.0, 1.0, 50.0), (1500.0, 5.0, 0.7, 200.0), (1250.0, 20.0, 1.2, 10.0), (1700.0, 0.5, 1.0, 900.0)]
    T0 = np.array([c[0] for c in cases])
    P0 = np.array([c[1] for c in cases]) * P_ATM
    Y0 = np.stack([ch4_air_Y(mech, c[2])[0] for c in cases])
    u0 = np.array([c[3] for c in cases])
    run = dict(energy=1, t_end=30.0, atol=1e-12, rtol=1e-8, ign_mode="TIFP")
    res = _np(dm.reactor_run(_native.make_cfg(**run), np.full(4, 3, np.int32), T0, P0, u0, Y0))
    out = [oracle.reactor(T0[i], P0[i], u0[i], Y0[i], problem=3, **run) for i in range(4)]
    _check(res, [o[0] for o in out], [o[1] for o in out], mech)


# ------------------------------------------------------------------ 2. A-factor perturbation by strip
def _reaction_in_strip(dm, tables, which):
    """An original reaction index whose device slot lies in the first strip, a middle strip or the falloff
    strip (slot // 64 from the mechanism's slot_of map)."""
    slot = dm.slot_of()
    strip = slot // 64
    rtype = np.asarray(tables["rtype"])
    if which == "first":
        cand = np.nonzero(strip == 0)[0]
    elif which == "middle":
        nel = int(strip[rtype == 0].max())  # the elementary strips are 0 .. nel
        assert nel >= 2
        cand = np.nonzero(strip == nel // 2 + (nel // 2 == 0))[0]
    else:
        cand = np.nonzero(rtype == 2)[0]
        assert np.all(strip[cand] == strip.max())  # the falloff reactions close the slot order
    assert cand.size
    return int(cand[cand.size // 2])


@pytest.fixture(scope="module")
def pert_base(dm, mech):
    """The four reactors of the perturbation cases, and their launch without any perturbation."""
    from pychemkin_amd import _native

    T0, P0 = np.array([1300.0, 1400.0, 1250.0, 1500.0]), np.array([5.0, 1.0, 20.0, 10.0]) * P_ATM
    Y0 = np.stack([ch4_air_Y(mech, phi)[0] for phi in (1.0, 0.7, 1.3, 1.0)])
    prob = np.array([1, 2, 1, 2], np.int32)
    res = _np(dm.reactor_run(_native.make_cfg(**RUN), prob, T0, P0, np.ones(4), Y0))
    return dict(T0=T0, P0=P0, Y0=Y0, prob=prob, res=res)


@pytest.mark.parametrize("which", ["first", "middle", "falloff"])
def test_afactor_slot_by_strip(dm, oracle, mech, tables, pert_base, which):
    from pychemkin_amd import _native

    b = pert_base
    irx = _reaction_in_strip(dm, tables, which)
    rxn = np.array([irx, irx, irx, -1], np.int32)  # reactor 3 is left unperturbed
    fac = np.array([2.0, 0.5, 3.0, 1.0])
    res = _np(dm.reactor_run(_native.make_cfg(**RUN), b["prob"], b["T0"], b["P0"], np.ones(4), b["Y0"], afac_rxn=rxn,
                             afac=fac))
    orx = np.where(rxn < 0, 0, rxn).astype(np.int32)  # the oracle takes a factor of 1 on any reaction
    nfail, ref, Yref = oracle.reactor_batch_pert(b["T0"], b["P0"], b["Y0"], orx, fac, problem=b["prob"], V0=np.ones(4),
                                                 **RUN)
    assert nfail == 0
    _check(res, list(ref), Yref, mech)
    for k in ("tau", "T", "P", "V", "Y", "stats"):  # the unperturbed reactor: bitwise the plain launch's
        assert np.array_equal(res[k][3], b["res"][k][3]), (which, k)
    for i in range(3):  # and the perturbation took effect
        assert res["tau"][i] != b["res"]["tau"][i], (which, i)


# ------------------------------------------------------------------ 3. fexp at its edges
def test_fexp_edges_through_generic_rop_kernel(dm, oracle, mech, tables):
    """The generic ROP kernel (eval_rxn_img -> fexp) at temperatures where GRI-3.0's largest E/(R T) is past
    fexp's +/-1000 saturation (T = 55 K: 63,707 K / 55 K = 1,158), where it is close to it (64 - 120 K) and
    where no exponent comes near it (300 - 3,500 K).

    Checked on the CPU first: the oracle alone is finite at every state from 90 K up; at 55 K and 64 K its own
    rates of three or four reactions are 0 x inf (k_f = exp(-1158) = 0 times exp(-dG) = inf), which leaves 9
    of the 53 species non-finite there.  Those entries carry no demand; every entry where the oracle is finite
    must be finite on the GPU and within the 1e-11 bar of test_gpu_rop_jit.py (of the state's largest finite
    |wdot|).  A NaN temperature must give NaN rates."""
    from pychemkin_amd import _native

    rng = np.random.default_rng(8)
    Ts = np.array([55.0, 64.0, 90.0, 120.0, 300.0, 1000.0, 2000.0, 3500.0])
    E = np.asarray(tables["arr"]).reshape(-1, 3)[:, 2]
    assert E.max() / Ts[0] > 1000.0 and E.max() / Ts[4] < 1000.0
    T = np.repeat(Ts, 5)
    n = T.size
    P = P_ATM * 10.0 ** rng.uniform(-1.0, 2.0, n)
    Y = rng.dirichlet(0.5 * np.ones(mech.KK), n).T.copy()
    wo = oracle.rop_batch(T, P, Y)[0]
    fin = np.isfinite(wo)
    assert fin[:, T >= 90.0].all()
    assert fin.sum(axis=0).min() >= mech.KK - 12  # the low states still compare most species
    _native.set_rop_path(1)
    try:
        w = dm.rop_thermo(T, P, Y)[0].cpu().numpy()
        Tn = T.copy()
        Tn[::7] = np.nan
        wn = dm.rop_thermo(Tn, P, Y)[0].cpu().numpy()
    finally:
        _native.set_rop_path(0)
    assert np.isfinite(w[fin]).all()
    scale = np.max(np.where(fin, np.abs(wo), 0.0), axis=0, keepdims=True)
    err = np.where(fin, np.abs(w - np.where(fin, wo, 0.0)), 0.0) / np.where(scale > 0, scale, 1.0)
    print("fexp edges: max scaled error per temperature", {float(t): float(err[:, T == t].max()) for t in Ts})
    assert err.max() < 1e-11
    assert np.isnan(wn[:, ::7]).all()
    keep = np.ones(n, bool)
    keep[::7] = False
    assert np.array_equal(wn[:, keep], w[:, keep], equal_nan=True)  # (the coldest states hold NaN entries themselves)
