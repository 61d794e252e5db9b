"""Diffusion kernels (ckmi_binary_diffusion / ckmi_mixture_diffusion / ckmi_multicomponent_diffusion) against the
numpy restatement of tests/diffusion_reference.py, through the batched ABI, the drop-in Chemistry / Mixture methods
and the KIN calls.  Mechanisms, states and the reference of every state: tests/diffusion_cases.py (its invariants
are proven on the CPU by tests/test_diffusion_host.py).

Bars: binary and mixture-averaged 1e-12 relative against the restatement on the same fit table (a cubic, an exp
and a KK-term positive sum in FP64); multicomponent: info = 0, D_ii = 0 exactly, mass-conservation and
Stefan-Maxwell residuals at most 100 x the float64 reference's on the same state, and element-wise agreement,
relative to max |D|, at 100 x the reference's own error against the longdouble elimination (that bar stays below
1e-8 on every state, so the assembly needs no row equilibration).
"""
import ctypes as ct
import functools

import numpy as np
import pytest

import diffusion_cases as dc
import diffusion_reference as dr
import mechanism_variants as mv
from conftest import CHEM, P_ATM, THERM, TRAN, golden

pytestmark = pytest.mark.gpu

CASES = [(name, n) for name in dc.MECHS for n in dc.BATCHES]


@functools.lru_cache(maxsize=None)
def device(name):
    """(DeviceMechanism, DeviceTransport with the diffusion table) of one mechanism, kept for the session."""
    from pychemkin_amd import _native, transport

    mech = dc.mechanism(name)
    dm = _native.DeviceMechanism(mech.to_tables(), device=0)
    vf = transport.viscosity_fits(mech.wt, dc.transport_params(name))
    return dm, _native.DeviceTransport(dm, vf, None, dc.native_fits(name))


@pytest.mark.parametrize("name,n", CASES)
def test_binary_and_mixture_averaged(name, n):
    _, dt = device(name)
    ref = dc.reference(name)
    idx, T, P, Y = dc.batch(name, n)
    KK = dc.MECHS[name]
    Db = dt.binary_diffusion(T, P).cpu().numpy()
    assert Db.shape == (n, KK, KK)
    eb = np.max(np.abs(Db / ref["binary"][idx] - 1))
    Dm = dt.mixture_diffusion(T, P, Y).cpu().numpy()
    assert Dm.shape == (KK, n)
    em = np.max(np.abs(Dm / ref["mixture"][:, idx] - 1))
    print(f"{name} n={n}: binary {eb:.2e} mixture-averaged {em:.2e}")
    assert np.all(np.isfinite(Db)) and np.all(Db > 0) and eb < 1e-12
    assert np.all(np.isfinite(Dm)) and np.all(Dm > 0) and em < 1e-12


@pytest.mark.parametrize("name,n", CASES)
def test_multicomponent(name, n):
    mech = dc.mechanism(name)
    _, dt = device(name)
    ref = dc.reference(name)
    idx, T, P, Y = dc.batch(name, n)
    KK = mech.KK
    D = dt.multicomponent_diffusion(T, P, Y).cpu().numpy()  # raises when any info is non-zero
    assert D.shape == (n, KK, KK) and np.all(np.isfinite(D))
    assert np.all(D[:, np.arange(KK), np.arange(KK)] == 0.0)
    worst = dict(mass=0.0, sm=0.0, elem=0.0)
    for s in range(n):
        r = idx[s]
        mass = dr.mass_conservation_residual(D[s], mech.wt)
        sm = dr.stefan_maxwell_residual(D[s], ref["X"][r], mech.wt, ref["binary"][r], ref["d"][r])
        elem = np.max(np.abs(D[s] - ref["multi"][r])) / np.max(np.abs(ref["multi"][r]))
        worst = dict(mass=max(worst["mass"], mass / ref["mass"][r]), sm=max(worst["sm"], sm / ref["sm"][r]),
                     elem=max(worst["elem"], elem / ref["err"][r]))
        if s < 6:
            print(f"{name} n={n} state {r}: mass {mass:.2e} (ref {ref['mass'][r]:.2e})  Stefan-Maxwell {sm:.2e} "
                  f"(ref {ref['sm'][r]:.2e})  element-wise {elem:.2e} (ref vs longdouble {ref['err'][r]:.2e})")
        assert 100 * ref["err"][r] < 1e-8
        assert mass <= 100 * ref["mass"][r]
        assert sm <= 100 * ref["sm"][r]
        assert elem <= 100 * ref["err"][r]
    print(f"{name} n={n}: worst ratios to the reference's own figures {worst}")
    # the same state gives the same bits wherever it stands in the batch
    for s in range(6, n):
        assert np.array_equal(D[s], D[s - 6])


def test_fitted_against_direct_form():
    """The device's fitted binary coefficients against kinetic theory itself: the fit error of the host test
    (7.9e-3 at most, at the ends of [300, 3500] K)."""
    mech = dc.mechanism("gri")
    _, dt = device("gri")
    T = np.array([300.0, 500.0, 1000.0, 2000.0, 3500.0])
    P = np.array([1.0, 2.0, 0.1, 40.0, 1.0]) * P_ATM
    Db = dt.binary_diffusion(T, P).cpu().numpy()
    ex = np.stack([dr.binary_exact(t, p, mech.wt, dc.transport_params("gri")) for t, p in zip(T, P)])
    e = np.max(np.abs(Db / ex - 1))
    print(f"fitted vs direct: {e:.2e}")
    assert e < 1e-2


def test_argument_checks():
    from pychemkin_amd import _native, transport

    mech = dc.mechanism("gri")
    dm, dt = device("gri")
    # n = 0 is a no-op
    e = np.zeros(0)
    assert tuple(dt.binary_diffusion(e, e).shape) == (0, mech.KK, mech.KK)
    assert tuple(dt.mixture_diffusion(e, e, np.zeros((mech.KK, 0))).shape) == (mech.KK, 0)
    assert tuple(dt.multicomponent_diffusion(e, e, np.zeros((mech.KK, 0))).shape) == (0, mech.KK, mech.KK)
    # without a diffusion table: CKMI_ERR_ARG
    bare = _native.DeviceTransport(dm, transport.viscosity_fits(mech.wt, dc.transport_params("gri")))
    _, T, P, Y = dc.batch("gri", 2)
    for call in (lambda: bare.binary_diffusion(T, P), lambda: bare.mixture_diffusion(T, P, Y),
                 lambda: bare.multicomponent_diffusion(T, P, Y)):
        with pytest.raises(_native.NativeError, match=r"code 1\).*no diffusion fits"):
            call()
    bare.close()
    with pytest.raises(_native.NativeError, match="diffusion fits must be"):
        _native.DeviceTransport(dm, transport.viscosity_fits(mech.wt, dc.transport_params("gri")), None,
                                dc.native_fits("gri")[:-1])


def test_more_species_than_the_lu_holds():
    """KK = 193 > CKMI_LU_NMAX: the multicomponent call is refused with CKMI_ERR_UNSUPPORTED, the other two run."""
    from pychemkin_amd import _native, transport

    mech = mv.tracer_mechanism(193 - mv.KK_GRI)
    assert mech.KK == 193
    data = transport.parse_transport_text(open(dc.TRAN).read())
    params = np.array([data.get(s.upper(), data["AR"]) for s in mech.species])
    dm = _native.DeviceMechanism(mech.to_tables(), device=0)
    f = transport.diffusion_fits(mech.wt, params)
    dt = _native.DeviceTransport(dm, transport.viscosity_fits(mech.wt, params), None, f)
    T, P = np.array([900.0, 1500.0]), np.array([1.0, 3.0]) * P_ATM
    Y = np.zeros((193, 2))
    Y[mech.species.index("N2")] = 0.7
    Y[192] = 0.3
    with pytest.raises(_native.NativeError, match=r"code 4\).*more than 192 species"):
        dt.multicomponent_diffusion(T, P, Y)
    Dm = dt.mixture_diffusion(T, P, Y).cpu().numpy()
    assert np.max(np.abs(Dm / dr.mixture_averaged(T, P, Y, mech.wt, f) - 1)) < 1e-12
    Db = dt.binary_diffusion(T, P).cpu().numpy()
    assert np.max(np.abs(Db / dr.binary_from_fits(T, P, f) - 1)) < 1e-12
    dt.close()
    dm.close()


def _mixture(chem, T=None, P=None, comp=True):
    import pychemkin_amd as ck

    m = ck.Mixture(chem)
    if T is not None:
        m.temperature = T
    if P is not None:
        m.pressure = P
    if comp:
        m.X = [("CH4", 1.0), ("O2", 2.0), ("N2", 7.52)]
    return m


def test_public_api(chem_tran):
    import pychemkin_amd as ck

    g = golden("speciesproperties_diffusivity")
    KK = chem_tran.KK
    j, k = (chem_tran.get_specindex(s) for s in g["species"])
    D = chem_tran.SpeciesDiffusionCoeffs(g["pressure_atm"] * P_ATM, g["temperature_K"])
    assert D.shape == (KK, KK) and np.array_equal(D, D.T)
    print(f"D(CH4, O2) {D[j, k]:.10f} golden {g['state-binary_diffusivity'][0]:.10f}")
    assert abs(D[j, k] / g["state-binary_diffusivity"][0] - 1) < 1e-2
    with pytest.raises(ck.chemistry.ChemistryError, match="temperature"):
        chem_tran.SpeciesDiffusionCoeffs(P_ATM, 0.0)
    with pytest.raises(ck.chemistry.ChemistryError, match="pressure"):
        chem_tran.SpeciesDiffusionCoeffs(0.0, 500.0)
    m = _mixture(chem_tran, 500.0, 2.0 * P_ATM)
    assert np.array_equal(m.species_Diffusion_Coeffs(), D)
    Dm = m.mixture_diffusion_coeffs()
    Dmc = m.mixture_binary_diffusion_coeffs()
    assert Dm.shape == (KK,) and Dmc.shape == (KK, KK)
    # cm2/s: O2 in CH4 / air at 500 K and 2 atm, about 0.25 (D(O2, N2) is 0.2 at 300 K and 1 atm, ~ T^1.7 / P);
    # H, the lightest species, is several times faster
    o2, h = chem_tran.get_specindex("O2"), chem_tran.get_specindex("H")
    assert 0.15 < Dm[o2] < 0.4 and 3.0 * Dm[o2] < Dm[h] < 10.0 * Dm[o2]
    assert np.all(np.diag(Dmc) == 0.0) and np.all(np.isfinite(Dmc))
    f = chem_tran.diffusion_fits
    T, P, Y = np.array([500.0]), np.array([2.0 * P_ATM]), m.Y.reshape(KK, 1)
    wt = np.asarray(chem_tran.WT)
    assert np.max(np.abs(Dm / dr.mixture_averaged(T, P, Y, wt, f)[:, 0] - 1)) < 1e-12
    refmc = dr.multicomponent(T, P, Y, wt, f)[0]
    assert np.max(np.abs(Dmc - refmc)) / np.max(np.abs(refmc)) < 1e-12
    # the neighbouring methods' errors
    MixtureError = ck.mixture.MixtureError
    for call in ("species_Diffusion_Coeffs", "mixture_diffusion_coeffs", "mixture_binary_diffusion_coeffs"):
        with pytest.raises(MixtureError, match="temperature"):
            getattr(_mixture(chem_tran, None, P_ATM), call)()
        with pytest.raises(MixtureError, match="pressure"):
            getattr(_mixture(chem_tran, 500.0, None), call)()
    for call in ("mixture_diffusion_coeffs", "mixture_binary_diffusion_coeffs"):
        with pytest.raises(MixtureError, match="composition"):
            getattr(_mixture(chem_tran, 500.0, P_ATM, comp=False), call)()
    bare = ck.Chemistry(chem=CHEM, therm=THERM, label="GRI 3.0 without transport")
    bare.preprocess()
    with pytest.raises(Exception, match="no transport data"):
        bare.SpeciesDiffusionCoeffs(P_ATM, 500.0)
    with pytest.raises(MixtureError, match="no transport data"):
        _mixture(bare, 500.0, P_ATM).mixture_diffusion_coeffs()


def test_kin_entry_points(chem_tran):
    """KINGetDiffusionCoeffs / KINGetMixtureDiffusionCoeffs / KINGetOrdinaryDiffusionCoeffs through ctypes with
    F-order arrays: bit for bit the Mixture results."""
    from pychemkin_amd import kin

    KK = chem_tran.KK
    m = _mixture(chem_tran, 1200.0, 3.0 * P_ATM)
    L = kin.bind()
    cs, one, zero = ct.c_int(0), ct.c_int(1), ct.c_int(0)
    names = [CHEM, "", THERM, TRAN, "chem.asc", "surf.asc", "tran.asc", ""]
    rc = L.KINPreProcess(ct.byref(zero), ct.byref(one), *[ct.c_char_p(x.encode()) for x in names], ct.byref(cs))
    assert rc == 0, kin.last_error()
    PP, TT = ct.c_double(3.0 * P_ATM), ct.c_double(1200.0)
    Y = np.ascontiguousarray(m.Y)
    try:
        Db = np.zeros((KK, KK), order="F")
        assert L.KINGetDiffusionCoeffs(ct.byref(cs), ct.byref(PP), ct.byref(TT), Db) == 0, kin.last_error()
        Dm = np.zeros(KK)
        assert L.KINGetMixtureDiffusionCoeffs(ct.byref(cs), ct.byref(PP), ct.byref(TT), Y, Dm) == 0, kin.last_error()
        Dmc = np.zeros((KK, KK), order="F")
        assert L.KINGetOrdinaryDiffusionCoeffs(ct.byref(cs), ct.byref(PP), ct.byref(TT), Y, Dmc) == 0, kin.last_error()
        for a, b, what in ((Db, m.species_Diffusion_Coeffs(), "binary"), (Dm, m.mixture_diffusion_coeffs(), "mixture"),
                           (Dmc, m.mixture_binary_diffusion_coeffs(), "multicomponent")):
            print(f"KIN vs Mixture {what}: max |a - b| / max |b| = {np.max(np.abs(a - b)) / np.max(np.abs(b)):.2e}")
            assert np.array_equal(a, b), what
        assert not np.array_equal(Dmc, Dmc.T)  # the orientation is tested: D_jk != D_kj
        # thermal diffusion stays out of scope
        assert L.KINGetThermalDiffusionCoeffs(ct.byref(cs), ct.byref(PP), ct.byref(TT), Y, np.zeros(KK),
                                              ct.byref(ct.c_double(0.0))) == 4
    finally:
        kin.release(cs.value)
    rc = L.KINPreProcess(ct.byref(zero), ct.byref(zero), *[ct.c_char_p(x.encode()) for x in names], ct.byref(cs))
    assert rc == 0
    try:
        for call, args in ((L.KINGetDiffusionCoeffs, (np.zeros((KK, KK), order="F"),)),
                           (L.KINGetMixtureDiffusionCoeffs, (Y, np.zeros(KK))),
                           (L.KINGetOrdinaryDiffusionCoeffs, (Y, np.zeros((KK, KK), order="F")))):
            assert call(ct.byref(cs), ct.byref(PP), ct.byref(TT), *args) != 0
            assert b"transport" in L.ckmi_kin_last_error()
    finally:
        kin.release(cs.value)
