"""Every compiled size variant of the device kernels at its block edges (DESIGN.md "Compiled size variants").

The host-side dispatch picks a kernel instantiation from the species, variable or element count; GRI-3.0, the
161-species stand-in and the 10-species H2 subset reach a minority of them.  These cases walk the sizes: each
variant exactly full (no padding) and with the most padding it can carry, with the highest-index species -- the
one beside the padding and the dummy slot -- live.  The inputs come from tests/mechanism_variants.py;
tests/test_size_variants_host.py proves on the CPU that each of them has its size, maps to its variant and is
solved by the reference, so nothing is filtered here.  Tolerances are the existing ones of the kernel's own test
file, named per group.

Measured on an MI355X -- kernel against tests/equilibrium_reference.py, largest disagreement over options 1-9
(T, P relative, ln x_j over x_j >= 1e-20) per element count:
    MM = 1: 2.98e-12    MM = 2: 1.19e-11    MM = 3: 2.68e-11    MM = 4: 1.14e-11
    MM = 6: 1.83e-11    MM = 7: 1.78e-11    MM = 8: 1.50e-11        (BOUND of test_gpu_equilibrium.py: 1.8e-10)
D and T of the option-10 states within 2e-14 of the reference's.  Rates: wdot within 4.7e-14 and q within 6.0e-14 of
the state's largest at every size (bar 1e-11).  PSR at nvar = 64: reference residual 0.69 of the rule.
"""
import numpy as np
import pytest
import scipy.linalg as sla

import mechanism_variants as mv
from conftest import P_ATM, golden, gpu_available, within

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

NST, NFE, NJE, NLU, NCF, NEF, STATUS, NNI = range(8)


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items() if not k.startswith("_")}


# ---------------------------------------------------------------------- 3.1 workgroup reactor kernel
@pytest.mark.parametrize("nvar,plog", mv.BIG_CASES)
def test_big_reactor_variant(nvar, plog):
    """big_reactor_kernel<NB, PL> for NB = 5..12 plain and 8, 11, 12 extended, each most padded and exactly
    full; nvar 177 and 192 are the only sizes on BigMatrix<12>, the per-column Gauss-Jordan.  4 reactors against
    the oracle at the bars of test_gpu_bigreactor.py::test_big_reactors_match_oracle (tau, T 1e-4; species
    1e-4 max(|Yref|, 1e-3) on MAJOR and the last two tracers; |sum Y - 1| < 1e-8; NST within 25 %), and at least
    one factorisation.  The tracer family's image fits the kernel's LDS at every size, KK = 191 included, so the
    thinning option of mechanism_variants stays unused (BIG_THIN is empty)."""
    from pychemkin_amd import _native

    r = mv.big_reference(nvar, plog)
    mech, ref, Yref = r["mech"], r["ref"], r["Yref"]
    assert r["nfail"] == 0
    dm = _native.DeviceMechanism(mech.to_tables())
    try:
        res = _np(dm.reactor_run(_native.make_cfg(**mv.BIG_RUN), r["prob"], r["T0"], r["P0"], np.ones(4), r["Y0"]))
    finally:
        dm.close()
    st = res["stats"]
    species = mv.BIG_MAJOR + mv.last_tracers(mech)
    for i in range(4):
        x = ref[i]
        assert st[i, STATUS] == 0, (i, st[i].tolist())
        assert x.tau > 0 and res["tau"][i] > 0
        print(f"nvar {nvar} plog {plog} reactor {i}: tau/ref - 1 {res['tau'][i] / x.tau - 1:.2e}, T/ref - 1 "
              f"{res['T'][i] / x.T - 1:.2e}, nst {st[i, NST]} (oracle {x.nst}), nlu {st[i, NLU]}")
        assert abs(res["tau"][i] / x.tau - 1) < 1e-4, (i, res["tau"][i], x.tau)
        assert abs(res["T"][i] / x.T - 1) < 1e-4, (i, res["T"][i], x.T)
        for sp in species:
            k = mech.species.index(sp)
            assert abs(res["Y"][i, k] - Yref[i, k]) <= 1e-4 * max(abs(Yref[i, k]), 1e-3), (i, sp, res["Y"][i, k], Yref[i, k])
        assert abs(res["Y"][i].sum() - 1.0) < 1e-8
    nst_o = np.array([x.nst for x in ref])
    assert np.all(np.abs(st[:, NST] - nst_o) <= 0.25 * nst_o), (st[:, NST], nst_o)
    assert np.all(st[:, NLU] >= 1), st[:, NLU]


# ---------------------------------------------------------------------- 3.2 wave kernel edges
@pytest.mark.parametrize("name,path", [(n, p) for n, c in mv.WAVE_CASES.items() for p in c[2]])
def test_wave_reactor_variant(name, path):
    """reactor_kernel<32> exactly full (31 species), <54> with 21 padded variables (32 species), <64, false, *>
    and <64, true, *> with 9 padded variables and exactly full; path 3 forces the FP32-stored inverse, 2 the
    FP64 one (0: the automatic choice).  Bars of test_gpu_hotloop_paths._check, plus the last tracer.

    Finding of this test: on the automatic path the rich 1600 K / 50 atm reactor of PLOG GRI + 10 tracers ended
    with CKMI_RUN_ERRTEST (status 2) -- 859 steps of the oracle's 902 done, 7 error-test failures in a row in the
    equilibrium tail -- in reactor_kernel<64, true, false>; a probe gave the same on 8 tracers of both bases with
    the FP32-stored inverse and status 0 at every size with the FP64 one.  Since then the FP64-inverse launch that
    follows the FP32 one in the 64-wide variants also takes again the reactors that ended with an error-test or
    convergence failure (SEL_PFR_RETRY, ckmi_reactor_kernel.hpp); a forced path 3 keeps the FP32 inverse's own
    status."""
    from pychemkin_amd import _native
    from test_gpu_hotloop_paths import _check

    r = mv.wave_reference(name)
    mech = r["mech"]
    assert r["nfail"] == 0
    dm = _native.DeviceMechanism(mech.to_tables())
    _native.set_reactor_path(path)
    try:
        res = _np(dm.reactor_run(_native.make_cfg(**mv.WAVE_RUN), r["prob"], r["T0"], r["P0"], np.ones(4), r["Y0"]))
    finally:
        _native.set_reactor_path(0)
        dm.close()
    major = mv.WAVE_MAJOR + ((mech.species[-1], "AX1") if mech.KK > mv.KK_GRI else ())
    _check(res, r["ref"], r["Yref"], mech, major=major)


def test_psr_variant_64_plain():
    """reactor_kernel<64, false, true, true>: one ignited PSR on GRI-3.0 + 10 tracers (nvar = 64, exactly full),
    checked as test_gpu_psr.py::test_plog_mechanism checks its reactor: the steady-state rule recomputed by
    PSRReference at the kernel's state."""
    from psr_reference import PSRReference
    from pychemkin_amd import _native
    from test_gpu_psr import SS_ATOL, SS_RTOL, _check_rule

    p = mv.psr_reference()
    mech, orc, Yin = p["mech"], p["oracle"], p["Yin"]
    assert p["status"] == 0 and mech.KK + 1 == 64
    dm = _native.DeviceMechanism(mech.to_tables(), device=0)
    try:
        r = dm.psr_run(_native.make_cfg(t_end=0.0, atol=1e-14, rtol=1e-8), 1, np.array([P_ATM]), np.array([mv.PSR_TIN]),
                       Yin[None], np.array([mv.PSR_MDOT]), np.array([mv.PSR_TAU]), np.array([p["Tb"]]), p["Yb"][None],
                       ss_rtol=SS_RTOL, ss_atol=SS_ATOL)
        T, Y, st = float(r["T"].cpu()[0]), r["Y"].cpu().numpy()[0], r["stats"].cpu().numpy()[0]
    finally:
        dm.close()
    assert st[STATUS] == 0 and T > 1700.0
    _check_rule(PSRReference(orc, P_ATM, mv.PSR_TIN, Yin, mv.PSR_MDOT, tau=mv.PSR_TAU), orc, mech.to_tables(), T, Y,
                mv.PSR_TAU, "PSR nvar 64")
    assert Y[-1] > 1e-3 and Y[mech.species.index("AX1")] > 1e-3


# ---------------------------------------------------------------------- 3.3 rates and thermo at the image edges
@pytest.mark.parametrize("KK,plog", mv.ROP_CASES)
def test_rates_at_image_edges(KK, plog):
    """rop_kernel<MODE, NCH, PL> (the generic kernel, set_rop_path(1)) for NCH = 1..4: KK = 63 fills every lane
    of one wave beside the dummy slot, 64 is the first with two chunks, 192 the first with four.  KK = 255, the
    last the image holds, is refused for LDS (test_rates_above_the_lds_capacity_are_refused), so the top size
    is the largest tracer count the kernels accept: 224 species on the plain base, 220 on the PLOG base.
    1 and 65 states; bars of test_gpu_bigmech.py: wdot 1e-11 of the state's largest, q 1e-11 of the state's
    largest, cp and h 1e-12, species thermo 1e-13 / 1e-12."""
    from pychemkin_amd import _native

    mech = mv.tracer_mechanism(KK - mv.KK_GRI, plog)
    dm = _native.DeviceMechanism(mech.to_tables())
    _native.set_rop_path(1)
    try:
        out = {}
        for n in mv.ROP_N:
            o = mv.rop_reference(KK, plog, n)
            w, cp, h = (x.cpu().numpy() for x in dm.rop_thermo(o["T"], o["P"], o["Y"]))
            qf, qr = (x.cpu().numpy() for x in dm.reaction_rates(o["T"], o["P"], o["Y"]))
            cpk, hk, _ = (x.cpu().numpy() for x in dm.species_thermo(o["T"]))
            out[n] = (o, w, cp, h, qf, qr, cpk, hk)
    finally:
        _native.set_rop_path(0)
        dm.close()
    for n, (o, w, cp, h, qf, qr, cpk, hk) in out.items():
        scale = np.max(np.abs(o["w"]), axis=0, keepdims=True)
        sq = np.maximum(np.max(np.abs(o["qf"]), axis=0), np.max(np.abs(o["qr"]), axis=0))[None]
        ew, eq_ = np.max(np.abs(w - o["w"]) / scale), max(np.max(np.abs(qf - o["qf"]) / sq), np.max(np.abs(qr - o["qr"]) / sq))
        print(f"KK {KK} plog {plog} n {n}: wdot {ew:.2e}, q {eq_:.2e}, cp {np.max(np.abs(cp / o['cp'] - 1)):.2e}")
        assert ew < 1e-11
        assert eq_ < 1e-11
        assert np.max(np.abs(cp / o["cp"] - 1)) < 1e-12
        assert np.max(np.abs(h - o["h"]) / np.max(np.abs(o["h"]))) < 1e-12
        assert np.allclose(cpk, o["cpk"], rtol=1e-13, atol=0)
        assert np.allclose(hk, o["hk"], rtol=1e-12, atol=1e-12)
    assert np.max(np.abs(out[65][1][-1])) > 0   # the last species (beside the dummy slot) reacts


@pytest.mark.parametrize("plog", [False, True])
def test_rates_above_the_lds_capacity_are_refused(plog):
    """One tracer above the top size (225 / 221 species), and at KK = 255, ckmi_rop_thermo and ckmi_reaction_rates
    refuse with CKMI_ERR_SIZE (image + ROP work space exceed the LDS of a CU) and leave their outputs alone;
    species thermo needs no image in LDS and still equals the oracle at KK = 255."""
    import torch
    from pychemkin_amd import _native

    for KK in (mv.ROP_TOP[plog] + 1, 255):
        mech = mv.tracer_mechanism(KK - mv.KK_GRI, plog)
        o = mv.rop_reference(KK, plog, 1)
        dm = _native.DeviceMechanism(mech.to_tables())
        _native.set_rop_path(1)
        try:
            w = torch.full((KK, 1), -7.0, dtype=torch.float64, device="cuda:0")
            with pytest.raises(_native.NativeError, match=r"code 3\).*exceed the LDS of a CU"):
                dm.rop_thermo(o["T"], o["P"], o["Y"], wdot=w)
            assert bool((w == -7.0).all())
            with pytest.raises(_native.NativeError, match=r"code 3\).*exceed the LDS of a CU"):
                dm.reaction_rates(o["T"], o["P"], o["Y"])
            cpk, hk, _ = (x.cpu().numpy() for x in dm.species_thermo(o["T"]))
        finally:
            _native.set_rop_path(0)
            dm.close()
        assert np.allclose(cpk, o["cpk"], rtol=1e-13, atol=0)
        assert np.allclose(hk, o["hk"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("plog", [False, True])
def test_256_species_are_refused(plog):
    """KK = 256 is one past the image (the dummy slot KKp - 1 has to fit in 8 bits): refused loudly by
    ckmi_mech_create or by the launch, never answered with numbers."""
    from pychemkin_amd import _native

    mech = mv.tracer_mechanism(256 - mv.KK_GRI, plog)
    assert mech.KK == 256
    T, P, Y = mv.rop_states(256, 1, seed=1)
    with pytest.raises(_native.NativeError, match="255 species"):
        dm = _native.DeviceMechanism(mech.to_tables())
        try:
            dm.rop_thermo(T, P, Y)
        finally:
            dm.close()


# ---------------------------------------------------------------------- 3.4 batched LU
def _factor(A_np):
    import torch
    from pychemkin_amd import _native

    A = torch.as_tensor(A_np.copy(), device="cuda:0")
    _, ipiv, info = _native.lu_factor_batched(A)
    torch.cuda.synchronize()
    return A.cpu().numpy(), ipiv.cpu().numpy(), info.cpu().numpy()


def _check_factors(A, LU, piv, info):
    """The assertions of test_gpu_lu.py::test_lu_matches_lapack on every system, and max |L| <= 1."""
    n = A.shape[1]
    assert np.all(info == 0)
    for s in range(A.shape[0]):
        lu_ref, piv_ref = sla.lu_factor(A[s])
        np.testing.assert_array_equal(piv[s], piv_ref)
        scale = np.abs(lu_ref).max()
        np.testing.assert_allclose(LU[s], lu_ref, rtol=0, atol=1e-12 * scale)
        L = np.tril(LU[s], -1) + np.eye(n)
        U = np.triu(LU[s])
        PA = A[s].copy()
        for i, p in enumerate(piv[s]):
            PA[[i, p]] = PA[[p, i]]
        np.testing.assert_allclose(L @ U, PA, rtol=0, atol=1e-13 * np.abs(A[s]).max() * n)
        assert np.max(np.abs(np.tril(LU[s], -1)), initial=0.0) <= 1.0


@pytest.mark.parametrize("n", mv.LU_N)
def test_lu_factor_variant(n):
    """lu_factor_kernel<NB>, NB = 1..12 at both edges (with the sizes of test_gpu_lu.py): 5 systems, half
    Newton-like and half random, and a matrix whose first column is all +-1 (ties: dgetrf takes the first
    maximum, row 0, as ckmi.h promises)."""
    A = np.concatenate([mv.lu_matrices(n), mv.tie_matrix(n)[None]])
    LU, piv, info = _factor(A)
    _check_factors(A, LU, piv, info)
    assert piv[-1][0] == 0


@pytest.mark.parametrize("n", mv.LU_N)
def test_lu_solve_variant(n):
    """ckmi_lu_solve_batched at every size with 1, 5 and 67 systems against numpy.linalg.solve at the bars of
    test_gpu_lu.py::test_lu_solve."""
    import torch
    from pychemkin_amd import _native

    for nsys in (1, 5, 67):
        A, b = mv.lu_solve_systems(n, nsys)
        At = torch.as_tensor(A.copy(), device="cuda:0")
        _, ipiv, info = _native.lu_factor_batched(At)
        bt = torch.as_tensor(b.copy(), device="cuda:0")
        _native.lu_solve_batched(At, ipiv, bt)
        x = bt.cpu().numpy()
        assert np.all(info.cpu().numpy() == 0)
        assert np.max(np.abs(np.tril(At.cpu().numpy(), -1)), initial=0.0) <= 1.0
        for s in range(nsys):
            xr = np.linalg.solve(A[s], b[s])
            np.testing.assert_allclose(x[s], xr, rtol=1e-10, atol=1e-12 * np.abs(xr).max())


@pytest.mark.parametrize("n", [5, 17])
def test_lu_grid_stride_loop(n):
    """8200 systems, more than the 8192 workgroups of a launch: the grid-stride loop takes a second matrix in
    eight workgroups.  Every system is compared with LAPACK."""
    rng = np.random.default_rng(n)
    A = rng.standard_normal((8200, n, n))
    A[::2] = mv.newton_like(rng, 4100, n)
    LU, piv, info = _factor(A)
    _check_factors(A, LU, piv, info)


def test_lu_batch_position_invariance_177():
    """BigMatrix's LU sibling at NB = 12, most padded: bitwise the same factors at another batch position."""
    rng = np.random.default_rng(177)
    A = mv.newton_like(rng, 12, 177)
    LU1, p1, _ = _factor(A)
    perm = rng.permutation(12)
    LU2, p2, _ = _factor(A[perm])
    np.testing.assert_array_equal(LU2, LU1[perm])
    np.testing.assert_array_equal(p2, p1[perm])
    one, p3, _ = _factor(A[7:8])
    np.testing.assert_array_equal(one[0], LU1[7])
    np.testing.assert_array_equal(p3[0], p1[7])


# ---------------------------------------------------------------------- 3.5 equilibrium, every element count
@pytest.mark.parametrize("MM", mv.EQ_MM)
def test_equilibrium_variant(MM):
    """equil_kernel<MM> for MM = 1, 2, 3, 4, 6, 7, 8 (GRI-3.0 is 5): options 1-9 on three (T, P) x 2-3 mixtures
    -- one with every element, one from which an element is absent -- and option 10 on the detonable mixtures,
    all in one launch, against EquilibriumReference.solve at test_gpu_equilibrium.py's BOUND; D and T of option 10
    within the CJ golden's tolerance; the first state alone bitwise what it gives in the full launch."""
    from pychemkin_amd import _native
    from test_gpu_equilibrium import BOUND, disagreement, gpu

    r = mv.equil_reference(MM)
    mech, ref, opt = r["mech"], r["ref"], r["opt"]
    assert np.all(ref["status"] == 0)
    dm = _native.DeviceMechanism(mech.to_tables(), device=0)
    try:
        g = gpu(dm, opt, r["T"], r["P"], r["Y"])
        one = gpu(dm, opt[:1], r["T"][:1], r["P"][:1], r["Y"][:1])
    finally:
        dm.close()
    assert g["status"].tolist() == [0] * opt.size
    m9, m10 = opt < 10, opt == 10
    d = disagreement(mech, {k: g[k][m9] for k in ("T", "P", "Y")}, {k: ref[k][m9] for k in ("T", "P", "X")})
    print(f"equil_kernel<{MM}>: {int(m9.sum())} states of options 1-9, largest disagreement {d:.3e}, iterations gpu / ref",
          g["iterations"].max(), ref["iterations"].max())
    assert d <= BOUND
    if m10.any():
        tol = golden("multiplemechanisms")["tolerance-var"]
        print(f"equil_kernel<{MM}>: {int(m10.sum())} CJ states, max |D/D_ref - 1|",
              np.max(np.abs(g["detspeed"][m10] / ref["detspeed"][m10] - 1)), "|T/T_ref - 1|",
              np.max(np.abs(g["T"][m10] / ref["T"][m10] - 1)))
        assert within(g["T"][m10], ref["T"][m10], *tol).all()
        assert within(g["detspeed"][m10], ref["detspeed"][m10], *tol).all()
    for k in ("T", "P", "Y", "stats"):
        assert np.array_equal(one[k][0], g[k][0]), k
