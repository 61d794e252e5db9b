"""CPU-side preconditions of tests/test_gpu_jacobian.py: for every input the GPU test uses, the mechanism maps to
the intended kernel variant, the reference is finite, the reference pieces added for this test (the open reactor's
volume-given terms) agree with central differences of the reference's own F, and the A-factor perturbations of the
sharpness test move the oracle's own Jacobian far enough to be seen.
"""
import numpy as np
import pytest

import jacobian_cases as jc
from mechanism_variants import WAVE_CASES, big_variant, wave_variant


# ---------------------------------------------------------------------- variants
@pytest.mark.parametrize("case", jc.CASES, ids=repr)
def test_case_maps_to_intended_variant(case):
    nv, pl = case.nvar, jc.is_plog(case.key)
    v = case.variant()
    if case.kind == "big":
        if nv > 64:
            want_nv = int(case.key.split("_")[1]) if "_" in case.key else 162
            assert nv == want_nv and v == big_variant(nv, pl)
        else:  # a wave-sized mechanism forced onto the workgroup kernel: the smallest matrix of its family
            assert case.path == 1 and v == ((8, True) if pl else (4, False))
    elif case.kind == "psr":
        assert nv <= 64 and v == ((64, pl) if pl or nv > 54 else (54, False))
    else:
        assert nv <= 64 and len(v) >= 1
        for N, PL, PF in v:
            assert PL == pl and N >= nv
            if case.key in WAVE_CASES:
                assert nv == WAVE_CASES[case.key][0]
                assert (N, PL) == (WAVE_CASES[case.key][1] if not PF else wave_variant(max(nv, 33), pl))
        assert all(p in (1, 2, 3, 4) for p in case.problems)
        if any(p == 3 for p in case.problems):
            assert any(PF for _, _, PF in v)


def test_cases_cover_every_variant():
    wave = {x for c in jc.CASES if c.kind == "wave" for x in c.variant()}
    assert {(32, False, False), (54, False, False), (64, False, False), (64, True, False), (54, False, True),
            (64, True, True)} <= wave
    big = {c.variant() for c in jc.CASES if c.kind == "big"}
    assert {(4, False), (5, False), (6, False), (11, False), (12, False), (8, True), (11, True), (12, True)} <= big
    psr = {(c.variant(), c.psr["mode"], c.energy) for c in jc.CASES if c.kind == "psr"}
    for v in ((54, False), (64, False), (64, True)):
        assert {(v, m, e) for m in (1, 2) for e in (1, 2)} <= psr
    assert jc.key_general("ford") and jc.key_general("wide") and jc.key_general("ext161") and not jc.key_general("cheb")
    assert jc.is_plog("cheb") and not jc.is_plog("gri")
    assert len({c.id for c in jc.CASES}) == len(jc.CASES)


# ---------------------------------------------------------------------- states and references
@pytest.mark.parametrize("key", sorted({c.key for c in jc.CASES}))
def test_states(key):
    st, mech = jc.states(key), jc.mechanism(key)
    y = st["y"]
    assert st["T_end"] > jc.T_CTX + 1000.0  # the run the states are cut from ignites
    i2, i3, i4 = st["i"]
    assert 0 < i2 < i3 < i4 < jc.NSAVE - 1
    # the burnt state has three quarters of the temperature rise behind it and is not yet equilibrated: its net
    # rates are within 1e2 of those at the largest dT/dt (the last saved point where they are a tenth, or the very
    # next one); at the equilibrated end of the run they are 1e6 smaller still
    assert y[3, 0] >= jc.T_CTX + 0.75 * (st["T_end"] - jc.T_CTX)
    fmax = lambda yy: np.max(np.abs(jc.oracle(key).rhs_jac(yy, problem=1, energy=1, P0=jc.P_CTX)[0][1:]))  # noqa: E731
    assert fmax(y[3]) >= 0.01 * fmax(y[2])
    assert fmax(y[3]) > 1e6 * fmax(st["y_equil"])
    # metric (a) can resolve 1e-9 at every state: the cancellation inside the net rates stays below 1e-9 / 2^-52.
    # The tracer mechanisms come closest, 1.5e6 in the induction (their exchange reactions AXk + H <=> AXk+1 + H
    # run 1e6 times faster forth and back than net); without tracers it is below 500 everywhere.
    gn = [jc.gross_over_net(key, y[i], st["P0"][i]) for i in range(8)]
    assert max(gn) < 4e6 and jc.gross_over_net(key, st["y_equil"], jc.P_CTX) > 1e12, gn
    if not (mech.KK > 53 and mech.species[-1].startswith("AX")):
        assert max(gn) < 500.0, gn
    assert np.count_nonzero(y[0, 1:]) <= 5 and y[0, 0] == jc.T_CTX          # exact zeros in most species
    assert jc.T_CTX < y[1, 0] < y[2, 0] < y[3, 0]
    assert y[4, 0] == 1000.0 and y[7, 0] == 300.0
    assert [y[5, 1 + mech.species.index(s)] for s in jc.RADICALS] == [-1e-12] * 4
    assert np.count_nonzero(y[6, 1:] == 1e-30) >= 1
    assert np.all(y[2, 1 + np.array([mech.species.index(s) for s in jc.RADICALS])] > 1e-8)  # state 3 is live
    if mech.KK > 53 and mech.species[-1].startswith("AX"):
        assert y[0, -1] > 0 and y[2, -1] > 0  # the species next to the padding takes part


@pytest.mark.parametrize("case", jc.CASES, ids=repr)
def test_reference_is_finite(case):
    f, J = jc.reference(case)
    assert np.isfinite(f).all() and np.isfinite(J).all()
    assert np.all(np.max(np.abs(f[:, 1:]), axis=1) > 0)
    if case.t and not case.engine:  # the profile cases evaluate strictly inside a piece
        assert any(a < case.t < b for a, b in zip(jc.PROF_X[:-1], jc.PROF_X[1:]))


# ---------------------------------------------------------------------- the open reactor's volume-given terms
def _fd(F, y):
    n = y.size
    D = np.zeros((n, n))
    for j in range(n):
        h = 1e-6 * max(abs(y[j]), 1e-4)
        yp, ym = y.copy(), y.copy()
        yp[j] += h
        ym[j] -= h
        D[:, j] = (F(yp) - F(ym)) / (2 * h)
    return D


@pytest.mark.parametrize("energy", [1, 2])
@pytest.mark.parametrize("state", [1, 2, 3])
def test_psr_volume_terms_against_central_differences(state, energy):
    """psr_reference_jac's volume-given terms against central differences of the reference's own F.

    The terms are isolated exactly: with tau frozen at its value at y, F is the residence-time-given residual, so
    FD(volume given) - FD(tau frozen) is the derivative of F through tau alone, which is what the new terms are
    (the closed part, with its third-body and falloff-F derivatives left out by design, cancels).  That covers the
    T column and the diagonal of the new terms.  Measured on the CPU: 3e-10 of the row maximum at worst (the state
    of largest dT/dt); the bar is 1e-8, fifty times the rounding eps / h = 2e-10 of one central difference with
    h = 1e-6 y (two are subtracted here; the truncation, h^2, is below that), against the 2e-2 of the existing
    finite-difference tests.  The whole Jacobian's distance from its own central differences is printed only: it is
    the oracle's closed Jacobian's, which those tests pin."""
    from psr_reference import PSRReference

    orc, st = jc.oracle("gri"), jc.states("gri")
    y = st["y"][state].copy()
    kw = dict(energy=energy, **jc.HTC)
    vol = jc.PSR_TAU * jc.PSR_MDOT / (jc.P_CTX / (jc.RU * y[0] * np.sum(y[1:] / orc.wt)))
    r2 = PSRReference(orc, jc.P_CTX, jc.PSR_TIN, st["Y0"], jc.PSR_MDOT, volume=vol, **kw)
    r1 = PSRReference(orc, jc.P_CTX, jc.PSR_TIN, st["Y0"], jc.PSR_MDOT, tau=r2.tau(y), **kw)
    _, J2 = jc.psr_reference_jac(r2, y)
    _, J1 = jc.psr_reference_jac(r1, y)
    D2, D1 = _fd(r2.residual, y), _fd(r1.residual, y)
    new, new_fd = J2 - J1, D2 - D1
    rowmax = np.maximum(np.max(np.abs(D2), axis=1), 1e-300)
    e_new = np.max(np.abs(new - new_fd) / rowmax[:, None])
    e_all = np.max(np.abs(J2 - D2) / rowmax[:, None])
    print(f"PSR volume terms state {state} energy {energy}: new terms {e_new:.2e}, whole J {e_all:.2e}")
    assert np.max(np.abs(new[:, 0])) > 0 and np.max(np.abs(np.diag(new)[1:])) > 0
    assert e_new < 1e-8


# ---------------------------------------------------------------------- the engine's oracle entry
@pytest.mark.parametrize("cid", [c.id for c in jc.CASES if c.engine and c.key == "gri"])
def test_engine_entry_against_central_differences(cid):
    """Oracle.rhs_jac_engine (the context from the cylinder's initial state) against central differences of its own
    f, at the bar of the existing finite-difference tests: 2e-2 of the row maximum (the third-body and falloff-F
    derivatives, and those of the wall coefficient h A, are left out by design); and the context is the initial
    state's: f moves when T0 moves (mass, Woschni reference) and, with ICHX, differs from the adiabatic f."""
    case = next(c for c in jc.CASES if c.id == cid)
    orc, st = jc.oracle(case.key), jc.states(case.key)
    ecfg = jc.engine_cfg(case)
    for i in (1, 2, 3):
        y = st["y"][i]
        F = lambda yy: orc.rhs_jac_engine(yy, jc.T_CTX, jc.P_CTX, st["Y0"], t=case.t, **ecfg)[0]  # noqa: E731
        f, J = orc.rhs_jac_engine(y, jc.T_CTX, jc.P_CTX, st["Y0"], t=case.t, **ecfg)
        D = _fd(F, y)
        rowmax = np.maximum(np.max(np.abs(D), axis=1), 1e-300)
        e = np.max(np.abs(J - D) / rowmax[:, None])
        print(f"engine entry {cid} state {i}: J against central differences {e:.2e} of the row maximum")
        assert e < 2e-2, (cid, i, e)
        f2 = orc.rhs_jac_engine(y, jc.T_CTX + 50.0, jc.P_CTX, st["Y0"], t=case.t, **ecfg)[0]
        assert abs(f2[0] / f[0] - 1) > 1e-3
        if case.engine == "ichx":
            fa = orc.rhs_jac_engine(y, jc.T_CTX, jc.P_CTX, st["Y0"], t=case.t, engine=ecfg["engine"] * (np.arange(20) != 7))[0]
            assert f[0] < fa[0]  # the wall takes heat out of the hot gas


# ---------------------------------------------------------------------- sharpness choice
def test_sharp_reactions_move_the_oracle_enough():
    from test_gpu_jacobian import BOUND_J

    picks = jc.sharp_reactions()
    assert [p[0] for p in picks] == [0, 1, 2]
    for rtype, rxn, moved in picks:
        print(f"sharp: type {rtype} reaction {rxn} moves metric (b) by {moved:.3e} at 1 + 1e-6, "
              f"{jc.sharp_moved(rxn, jc.SHARP_SCALE_PARKED):.3e} at 1 + 1e-4")
        assert moved >= 100.0 * BOUND_J, (rxn, moved)
        assert jc.sharp_moved(rxn, jc.SHARP_SCALE) < 100.0 * jc.FP32_EPS  # why path 1 needs the larger scale
        assert jc.sharp_moved(rxn, jc.SHARP_SCALE_PARKED) >= 100.0 * jc.FP32_EPS, rxn
