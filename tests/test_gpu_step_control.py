"""Every control path of the wave reactor kernel's step control, at the smallest batch, against the oracle.

GRI-3.0 CH4/air, phi = 1, 1 atm, bench.RUN, 12 CONP reactors with T0 spread over 1150-1300 K: one FP32-inverse
workgroup exactly (12 waves), and on the FP64-inverse path (ckmi_set_reactor_path(2)) 8 in one workgroup and 4
in a second.  The cases walk the integrator's states off the common path:

  a  plain TIFP
  b  h0 = 1e-2: convergence failures and a run of error-test failures on the first step (bdf_restore, the
     ETACF rescale, the order-1 recovery)
  c  hmax = 1e-3: hmax_inv clipping, about twice the steps
  d  nneg: the negative-part terms of the Newton iteration's norms and the clipping
  e  11 save points in [0, 1 s]: dky0_lane at every point; and the same with IGN_STOP (every reactor ignites
     before 0.1 s, so the stop leaves the t = 0 row and the NaN fill of the ten after it)
  f  threshold ignition (T_rise) with IGN_STOP: the 60-step bisection
  g  a pressure profile with two breakpoints inside the run: critical-time restarts, the hprime clip at nst == 0
  h  ADAP with asteps

Expected values are the oracle's on the same inputs, at the bars tests/test_gpu_reactor.py uses for the same
quantities (tau 1e-4, final T 1e-4, major species 1e-4 of max(|Y|, 1e-3), saved rows 1e-6) and
tests/test_gpu_features.py for the ADAP points (1e-5); the workgroup kernel, which shares the BDF helpers, runs
4 reactors of the 161-species stand-in at the bars of tests/test_gpu_bigreactor.py.

The not-gpu half asserts the preconditions on the CPU: the oracle returns status 0 on every input, and on (b)
it takes the failure paths itself.
"""
import numpy as np
import pytest

import bench
from conftest import P_ATM, ch4_air_Y

MAJOR = ("CH4", "O2", "N2", "H2O", "CO2", "CO", "H2")
NREACT = 12
T0S = np.linspace(1150.0, 1300.0, NREACT)
MXNEF1 = 3  # oracle/ckoracle.c, csrc/ckmi_reactor.hpp
T_SAVE = np.linspace(0.0, 1.0, 11)
PPRO = ([0.0, 1e-3, 2e-3, 2.0], [P_ATM, 2 * P_ATM, 3 * P_ATM, 3 * P_ATM])
ASTEPS = 20
MAX_ADAP = 256

# name -> (run configuration, stopped by IGN_STOP, save points)
CASES = {
    "a_tifp": (dict(bench.RUN), False, None),
    "b_h0": (dict(bench.RUN, h0=1e-2), False, None),
    "c_hmax": (dict(bench.RUN, hmax=1e-3), False, None),
    "d_nneg": (dict(bench.RUN, nneg=True), False, None),
    "e_save": (dict(bench.RUN), False, T_SAVE),
    "e_save_stop": (dict(bench.RUN, ign_stop=True), True, T_SAVE),
    "f_trise_stop": (dict(bench.RUN, ign_mode="T_rise", ign_val=400.0, ign_stop=True), True, None),
    "g_ppro": (dict(bench.RUN, profile=PPRO), False, None),
    "h_adap": (dict(bench.RUN, asteps=ASTEPS), False, None),
}

_REF = {}  # case name -> the oracle's results, computed once and shared by every test of the session


def oracle_ref(oracle, mech, name):
    if name not in _REF:
        cfg, _, ts = CASES[name]
        Y0 = ch4_air_Y(mech, 1.0)[0]
        out = []
        for T0 in T0S:
            if ts is None:
                r, Ye = oracle.reactor(float(T0), P_ATM, 1.0, Y0, problem=1, **cfg)
                out.append((r, Ye, None))
            else:
                r, Ye, (_, ys, _, _) = oracle.reactor(float(T0), P_ATM, 1.0, Y0, t_save=ts, problem=1, **cfg)
                out.append((r, Ye, ys))
        _REF[name] = out
    return _REF[name]


# ---------------------------------------------------------------- preconditions (CPU)
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_status_zero_on_every_input(oracle, mech, name):
    ref = oracle_ref(oracle, mech, name)
    assert len(ref) == NREACT
    for r, _, _ in ref:
        assert r.status == 0
        assert r.tau > 0


def test_oracle_takes_the_failure_paths_with_h0(oracle, mech):
    """(b) on the 1200 K reactor: at least one convergence failure, and at least MXNEF1 + 1 more error-test
    failures than the same reactor without h0 (here ncf 3, nef 71 against ncf 0, nef 53).

    These are totals of the whole run, and the step sequences of the two runs differ from the first step on,
    so across the T0 spread the difference of the totals scatters between -29 and +15.  Counted over the first
    accepted step alone (max_steps = 1), h0 = 1e-2 costs the oracle 2 or 3 convergence failures and 1 or 2
    error-test failures at every T0 of the spread, against none without it: bdf_restore and the ETACF rescale
    run on every reactor, the order-1 recovery (more than MXNEF1 error-test failures on one step) on none.
    Every reactor of the spread must show the first-step failures."""
    Y0 = ch4_air_Y(mech, 1.0)[0]
    rp, _ = oracle.reactor(1200.0, P_ATM, 1.0, Y0, problem=1, **CASES["a_tifp"][0])
    rf, _ = oracle.reactor(1200.0, P_ATM, 1.0, Y0, problem=1, **CASES["b_h0"][0])
    assert rp.status == 0 and rf.status == 0
    assert rf.ncf >= 1, (rf.ncf, rp.ncf)
    assert rf.nef >= rp.nef + MXNEF1 + 1, (rf.nef, rp.nef)
    for T0 in T0S:
        r1, _ = oracle.reactor(float(T0), P_ATM, 1.0, Y0, problem=1, **dict(CASES["b_h0"][0], max_steps=1))
        r0, _ = oracle.reactor(float(T0), P_ATM, 1.0, Y0, problem=1, **dict(CASES["a_tifp"][0], max_steps=1))
        assert r1.ncf >= 1 and r1.nef >= 1 and r0.ncf == 0 and r0.nef == 0, (T0, r1.ncf, r1.nef, r0.ncf, r0.nef)
    for r, _, _ in oracle_ref(oracle, mech, "b_h0"):
        assert r.ncf >= 1


def test_oracle_cases_leave_the_common_path(oracle, mech):
    """(c) takes more steps than (a); the IGN_STOP cases stop early, with save points left for the NaN fill."""
    a = oracle_ref(oracle, mech, "a_tifp")
    for name, (_, stopped, ts) in CASES.items():
        ref = oracle_ref(oracle, mech, name)
        for (r, _, _), (ra, _, _) in zip(ref, a):
            if name == "c_hmax":
                assert r.nst > 1.5 * ra.nst
            if stopped:
                assert r.t_end < 1.0
            if ts is not None and stopped:
                assert np.any(ts > r.t_end)


# ---------------------------------------------------------------- the kernels (GPU)
@pytest.fixture(scope="module")
def dm(tables):
    from pychemkin_amd import _native

    return _native.DeviceMechanism(tables)


def _run(dm, mech, name, path):
    from pychemkin_amd import _native

    cfg, _, ts = CASES[name]
    Y0 = np.tile(ch4_air_Y(mech, 1.0), (NREACT, 1))
    kw = dict(t_save=ts) if ts is not None else {}
    if name == "h_adap":
        kw["max_adap"] = MAX_ADAP
    _native.set_reactor_path(path)
    try:
        res = dm.reactor_run(_native.make_cfg(**cfg), np.ones(NREACT, np.int32), T0S, np.full(NREACT, P_ATM),
                             np.ones(NREACT), Y0, **kw)
        return {k: v.cpu().numpy() for k, v in res.items() if not k.startswith("_")}
    finally:
        _native.set_reactor_path(0)


@pytest.mark.gpu
@pytest.mark.parametrize("path", [0, 2])  # 0: the FP32-stored inverse (12 waves, one workgroup); 2: FP64 (8 + 4)
@pytest.mark.parametrize("name", list(CASES))
def test_control_paths_match_oracle(dm, oracle, mech, name, path):
    cfg, stopped, ts = CASES[name]
    ref = oracle_ref(oracle, mech, name)
    res = _run(dm, mech, name, path)
    tau_rtol = 1e-4  # test_gpu_reactor._check: the "same algorithm" bar on tau
    for i, (r, Ye, ys) in enumerate(ref):
        st = res["stats"][i]
        print(name, path, i, "tau", res["tau"][i], r.tau, "T", res["T"][i], r.T, "stats", st.tolist(),
              "oracle nst/ncf/nef", r.nst, r.ncf, r.nef)
        assert st[6] == r.status == 0, (i, st.tolist())
        assert abs(res["tau"][i] / r.tau - 1) < tau_rtol, (i, res["tau"][i], r.tau)
        if name == "b_h0":  # the device took the convergence-failure path too (a step of 1e-2 s cannot converge)
            assert st[4] >= 1, st.tolist()
        if not stopped:
            # (IGN_STOP ends a run at the end of the first step past the ignition point: that time is a
            # property of the step sequence, so the end states are compared on the other cases only)
            assert abs(res["T"][i] / r.T - 1) < 1e-4, (i, res["T"][i], r.T)
            for sp in MAJOR:
                k = mech.species.index(sp)
                assert abs(res["Y"][i, k] - Ye[k]) <= 1e-4 * max(abs(Ye[k]), 1e-3), (i, sp)
        else:
            assert res["t_stop"][i] < 1.0 and res["T"][i] > T0S[i] + 200.0
        if ts is not None:
            got = res["y_save"][i]
            both = ts <= min(res["t_stop"][i], r.t_end)
            assert both.sum() == (1 if stopped else len(ts))
            assert np.max(np.abs(got[both, 0] / ys[both, 0] - 1)) < 1e-6
            assert np.max(np.abs(got[both, 1:] - ys[both, 1:])) < 1e-6
            after = ts > res["t_stop"][i]
            assert after.any() == stopped and np.all(np.isnan(got[after])) and not np.any(np.isnan(got[~after]))
        if name == "h_adap":
            na = int(res["n_adap"][i])
            assert na == min(int(st[0]) // ASTEPS, MAX_ADAP) and na > 0
            ta = res["t_adap"][i, :na]
            assert np.all(np.diff(ta) > 0)
            _, _, (_, yo, _, _) = oracle.reactor(float(T0S[i]), P_ATM, 1.0, ch4_air_Y(mech, 1.0)[0], t_save=ta,
                                                 problem=1, **cfg)
            assert np.max(np.abs(res["y_adap"][i, :na, 0] / yo[:, 0] - 1)) < 1e-5


@pytest.mark.gpu
def test_workgroup_kernel_shares_the_helpers(big_mech):
    """4 reactors of the 161-species stand-in on the workgroup-per-reactor kernel, which instantiates the same
    bdf_* helpers with BdfT<256>: inputs and bars of tests/test_gpu_bigreactor.py."""
    from oracle.oracle import Oracle
    from pychemkin_amd import _native
    from test_gpu_bigreactor import MAJOR as BIG_MAJOR, RUN as BIG_RUN, _cases, tracer_Y

    n = 4
    T0, P0, phi, prob = _cases(n, 11)
    Y0 = tracer_Y(big_mech, phi)
    dmb = _native.DeviceMechanism(big_mech.to_tables())
    res = dmb.reactor_run(_native.make_cfg(**BIG_RUN), prob, T0, P0, np.ones(n), Y0)
    res = {k: v.cpu().numpy() for k, v in res.items() if not k.startswith("_")}
    nfail, ref, Yref = Oracle(big_mech).reactor_batch(T0, P0, Y0, problem=prob, V0=np.ones(n), **BIG_RUN)
    assert nfail == 0
    for i in range(n):
        r = ref[i]
        assert res["stats"][i, 6] == 0, (i, res["stats"][i].tolist())
        assert r.tau > 0 and res["tau"][i] > 0
        assert abs(res["tau"][i] / r.tau - 1) < 1e-4, (i, res["tau"][i], r.tau)
        assert abs(res["T"][i] / r.T - 1) < 1e-4, (i, res["T"][i], r.T)
        for sp in BIG_MAJOR:
            k = big_mech.species.index(sp)
            assert abs(res["Y"][i, k] - Yref[i, k]) <= 1e-4 * max(abs(Yref[i, k]), 1e-3), (i, sp)
        assert abs(res["Y"][i].sum() - 1.0) < 1e-8
    dmb.close()
