"""The reactor kernels' own right-hand side and analytic Jacobian, entry by entry, against the CPU oracle
(ckmi_reactor_rhs_jac).

The probe kernels call reactor_rhs (wave kernel) and rhs_big (workgroup kernel) once per state with the context
the integrators build, so a dropped dq/dC slot, a wrong sign, a mis-indexed entry next to a size variant's padding,
a wrong energy-row term or a wrong chunk of the FP32 parking layout shows here, where the trajectory tests only see
a slower Newton iteration.  Cases, states, references and metrics: tests/jacobian_cases.py; every input's
precondition is proved on the CPU by tests/test_jacobian_reference_host.py.

Bars.  (a) f and (b) the wave kernel's FP64 J: 10 x the largest disagreement with the reference measured on an
MI355X (MEASURED_F, MEASURED_J; the sums are reordered, not reformulated), which must stay below 1e-9 and 1e-8
(test_bounds_within_caps).  The tracer mechanisms' f gets a derived allowance on top, see MEASURED_F.  (c) the workgroup kernel's FP32-parked J is derived: 2^-23 |J_ref| (two FP32 roundings) plus the
bound of (b) on the same scale.
"""
import numpy as np
import pytest

import jacobian_cases as jc

pytestmark = pytest.mark.gpu

# measured on an MI355X (profiles/jac_probe_pytest_gpu.log).  MEASURED_F: the largest f figure of the cases WITHOUT
# tracers, 1.74e-12 on psr-plog-m2-e1 (1.65e-12 on wave-plog-pfr, 8e-13 on the engine).  The tracer mechanisms, whose
# exchange reactions cancel 1e6 : 1, reach 2.56e-10 (big-plain81) and are held to this bound plus a derived allowance
# (jacobian_cases.f_allowance): 0.013 of their bound there, 0.12 at most on any state.  MEASURED_J: the largest metric (b) of the wave and PSR
# cases, 2.46e-13 on wave-plog_t10-e1 (state T1000, problem 2); the parked entries use 0.50 of allowance (c).  The two
# passes agree to 8e-17 at worst.
MEASURED_F = 1.74e-12
MEASURED_J = 2.46e-13
BOUND_F = 10.0 * MEASURED_F
BOUND_J = 10.0 * MEASURED_J


# ---------------------------------------------------------------------- device side
@pytest.fixture(scope="module")
def devs():
    """Device mechanisms, one per mechanism key, for the life of the module."""
    from pychemkin_amd import _native

    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = _native.DeviceMechanism(jc.mechanism(key).to_tables(), device=0)
        return cache[key]

    yield get
    _native.set_reactor_path(0)
    for dm in cache.values():
        dm.close()


def probe(dm, case, a, jac, afac_rxn=None, out=None):
    """One ckmi_reactor_rhs_jac launch of case's configuration on the arrays a (launch_arrays layout)."""
    from pychemkin_amd import _native

    ecfg = {}
    if case.engine:
        import torch

        ecfg = jc.engine_cfg(case)
        if ecfg["tran"] is not None:
            ecfg["tran"] = torch.tensor(ecfg["tran"], dtype=torch.float64, device=dm.device)
    cfg = _native.make_cfg(energy=case.energy, **case.cfg, **ecfg)
    n = a["t"].size
    kw = {}
    V0 = a["V0"]
    if case.psr:
        mode, Tin, Yin, mdot, tv = jc.psr_inlet(case)
        sel = a["state"]
        kw["psr"] = (mode, Tin[sel], Yin[sel], mdot[sel])
        V0 = tv[sel]
    if case.afac:
        kw.update(afac_rxn=np.full(n, afac_rxn, np.int32), afac=np.full(n, case.afac[1]))
    _native.set_reactor_path(case.path)
    try:
        f, J = dm.rhs_jac(cfg, a["problem"], a["T0"], a["P0"], V0, a["Y0"], a["t"], a["y"], jac=jac, out=out, **kw)
    finally:
        _native.set_reactor_path(0)
    return f.cpu().numpy(), (J.cpu().numpy() if J is not None else None)


_RESULTS = {}


def result(case, devs):
    """Both passes of a case on the device and the reference, computed once per module."""
    if case.id not in _RESULTS:
        dm = devs(case.key)
        a = jc.launch_arrays(case)
        irx = jc.afac_reaction(case.key, case.afac[0], dm.slot_of()) if case.afac else None
        f_plain, _ = probe(dm, case, a, False, irx)
        f_j, J = probe(dm, case, a, True, irx)
        f_ref, J_ref = jc.reference(case, irx)
        _RESULTS[case.id] = dict(a=a, f_plain=f_plain, f_j=f_j, J=J, f_ref=f_ref, J_ref=J_ref)
    return _RESULTS[case.id]


# ---------------------------------------------------------------------- bars
def test_bounds_within_caps():
    assert BOUND_F <= 1e-9 and BOUND_J <= 1e-8


# ---------------------------------------------------------------------- (a) f, both passes
@pytest.mark.parametrize("case", jc.CASES, ids=repr)
def test_f_both_passes(case, devs):
    r = result(case, devs)
    assert np.isfinite(r["f_plain"]).all() and np.isfinite(r["f_j"]).all()
    ep = jc.f_errors(case, r["a"], r["f_plain"], r["f_ref"])
    ej = jc.f_errors(case, r["a"], r["f_j"], r["f_ref"])
    pp = jc.f_errors(case, r["a"], r["f_plain"], r["f_j"])  # the two passes against each other (measured only)
    # 10 x MEASURED_F; on the tracer mechanisms plus the derived rounding of their cancelling exchange (f_allowance)
    bound = BOUND_F + jc.f_allowance(case, r["a"])
    print(f"F {case.id}: plain {ep[0].max():.2e} {ep[1].max():.2e}  with_j {ej[0].max():.2e} {ej[1].max():.2e}  "
          f"pass-to-pass {pp[0].max():.2e} {pp[1].max():.2e}  of the bound {max(np.max(e / bound) for e in ep + ej):.3f}"
          f"  allowance {bound.max() - BOUND_F:.1e}")
    for name, e in (("plain pass", ep), ("with_j pass", ej)):
        for rows in e:
            bad = np.nonzero(rows > bound)[0]
            assert bad.size == 0, (case.id, name, jc.STATE_NAMES[r["a"]["state"][bad[0]]], rows[bad[0]], bound[bad[0]])


# ---------------------------------------------------------------------- (b), (c) J
@pytest.mark.parametrize("case", jc.CASES, ids=repr)
def test_jacobian(case, devs):
    r = result(case, devs)
    wt = jc.mechanism(case.key).wt
    n = r["J"].shape[0]
    parked = case.kind == "big"
    eb = [jc.j_error(wt, r["J"][i], r["J_ref"][i]) for i in range(n)]
    worst = int(np.argmax(eb))
    print(f"J {case.id}: metric (b) {max(eb):.2e} at state {jc.STATE_NAMES[r['a']['state'][worst]]} "
          f"problem {r['a']['problem'][worst]}" + (" (FP32-parked)" if parked else ""))
    if parked:
        ec = [jc.j_error_parked(wt, r["J"][i], r["J_ref"][i], BOUND_J) for i in range(n)]
        print(f"J {case.id}: metric (c) {max(ec):.3f} of the allowance")
        assert max(ec) <= 1.0, (case.id, jc.STATE_NAMES[r["a"]["state"][int(np.argmax(ec))]], max(ec))
    else:
        assert max(eb) <= BOUND_J, (case.id, jc.STATE_NAMES[r["a"]["state"][worst]], max(eb))


# ---------------------------------------------------------------------- (d) the test is sharp
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["elementary", "third-body", "falloff"])
def test_sharp(path, which, devs):
    """One reaction's A factor scaled by 1 + 1e-6 (path 1: 1 + 1e-4, see jacobian_cases.SHARP_SCALE_PARKED) must
    push the device Jacobian past the bound against the UNPERTURBED reference; restored, it is back inside."""
    dm = devs("gri")
    rtype, rxn, _ = jc.sharp_reactions()[which]
    case = jc.Case(f"sharp-{path}", "gri", path=path, problems=(1,))
    a = {k: v[2:3] for k, v in jc.launch_arrays(case).items()}  # state 3
    _, J_ref = jc.oracle("gri").rhs_jac(a["y"][0], problem=1, energy=1, P0=jc.P_CTX)
    wt = jc.mechanism("gri").wt
    metric = (lambda J: jc.j_error_parked(wt, J, J_ref, BOUND_J)) if path == 1 else \
        (lambda J: jc.j_error(wt, J, J_ref) / BOUND_J)
    A = dm.arrhenius()[0][rxn]
    dm.set_afactor(rxn, A * (jc.SHARP_SCALE_PARKED if path == 1 else jc.SHARP_SCALE))
    try:
        _, Jp = probe(dm, case, a, True)
    finally:
        dm.set_afactor(rxn, A)
    _, J0 = probe(dm, case, a, True)
    print(f"SHARP path {path} reaction {rxn} (type {rtype}): perturbed {metric(Jp[0]):.3g} x bound, restored {metric(J0[0]):.3g}")
    assert metric(Jp[0]) > 1.0, (path, rxn, metric(Jp[0]))
    assert metric(J0[0]) <= 1.0, (path, rxn, metric(J0[0]))


# ---------------------------------------------------------------------- (e) independence, launch shapes
@pytest.mark.parametrize("cid", ["wave-gri-e1", "big-gri-path1", "big-plog65", "psr-gri-m2-e1"])
def test_independence_and_launch_shapes(cid, devs):
    """A state's f and J are bitwise the same alone (n = 1), inside the n = 8 x problems launch and in a launch of
    4 x the probe's grid cap (the grid-stride loop runs four times); nothing is written past the outputs."""
    import torch

    case = next(c for c in jc.CASES if c.id == cid)
    dm = devs(case.key)
    r = result(case, devs)
    a = r["a"]
    n, nv = a["t"].size, case.nvar
    for i in range(0, n, max(1, n // 8)):  # n = 1: one launch per state (its first problem)
        one = {k: v[i:i + 1] for k, v in a.items()}
        f1, J1 = probe(dm, case, one, True)
        assert np.array_equal(f1[0], r["f_j"][i]) and np.array_equal(J1[0], r["J"][i]), (cid, i)
    cap = 64  # PROBE_GRID_MAX (ckmi_run.hpp)
    reps = -(-4 * cap // n)
    big = {k: np.concatenate([v] * reps, axis=0) for k, v in a.items()}
    nb = reps * n
    sentinel = -7.25e300
    fbuf = torch.full((nb * nv + 8,), sentinel, dtype=torch.float64, device=dm.device)
    Jbuf = torch.full((nb * nv * nv + 8,), sentinel, dtype=torch.float64, device=dm.device)
    out = (fbuf[:nb * nv].view(nb, nv), Jbuf[:nb * nv * nv].view(nb, nv, nv))
    fb, Jb = probe(dm, case, big, True, out=out)
    assert np.array_equal(fb.reshape(reps, n, nv), np.broadcast_to(r["f_j"], (reps, n, nv))), cid
    assert np.array_equal(Jb.reshape(reps, n, nv, nv), np.broadcast_to(r["J"], (reps, n, nv, nv))), cid
    assert bool((fbuf[nb * nv:] == sentinel).all()) and bool((Jbuf[nb * nv * nv:] == sentinel).all()), cid


# ---------------------------------------------------------------------- (f) refusals
def test_refusals(devs):
    import torch

    from pychemkin_amd import _native

    L = _native.lib()
    sentinel = -7.25e300

    def call(dm, problem, n=None, null_y=False, psr=False):
        import ctypes as ct

        KK = dm.KK
        m = len(problem)
        dev = dm.device
        f64 = dict(dtype=torch.float64, device=dev)
        prob = torch.tensor(problem, dtype=torch.int32, device=dev)
        T0 = torch.full((m,), 1400.0, **f64)
        P0 = torch.full((m,), jc.P_CTX, **f64)
        V0 = torch.ones(m, **f64)
        Y0 = torch.full((m, KK), 1.0 / KK, **f64)
        t = torch.zeros(m, **f64)
        y = torch.cat([T0[:, None], Y0], dim=1).contiguous()
        f = torch.full((m, KK + 1), sentinel, **f64)
        J = torch.full((m, KK + 1, KK + 1), sentinel, **f64)
        cfg = _native.make_cfg(energy=1)
        pc = _native.RhsPsr(1, T0.data_ptr(), Y0.data_ptr(), V0.data_ptr())
        rc = L.ckmi_reactor_rhs_jac(dm.handle, ct.byref(cfg), m if n is None else n, prob.data_ptr(), T0.data_ptr(),
                                    P0.data_ptr(), V0.data_ptr(), Y0.data_ptr(), t.data_ptr(),
                                    None if null_y else y.data_ptr(), None, ct.byref(pc) if psr else None,
                                    f.data_ptr(), J.data_ptr(), _native._stream_ptr(dev))
        torch.cuda.synchronize(dev)
        assert bool((f == sentinel).all()) and bool((J == sentinel).all()), "a refused call wrote its outputs"
        return rc

    ERR_ARG, ERR_UNSUPPORTED = 1, 4
    gri, big = devs("gri"), devs("big_65")
    assert call(big, [4]) == ERR_UNSUPPORTED          # an engine above 63 species
    assert call(big, [5], psr=True) == ERR_UNSUPPORTED  # an open reactor above 63 species
    assert call(gri, [0]) == ERR_ARG and call(gri, [1, 6]) == ERR_ARG  # problem outside 1..5
    assert call(gri, [1], n=-1) == ERR_ARG
    assert call(gri, [1], null_y=True) == ERR_ARG
    assert call(gri, [5]) == ERR_ARG                  # problem 5 without its inlet block
    assert call(gri, [1, 5], psr=True) == ERR_ARG     # open and closed reactors in one call
