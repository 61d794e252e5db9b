"""Binary diffusion fits on the host (ckmi_diffusion_fit needs no GPU) and the invariants of the numpy
multicomponent reference that tests/test_gpu_diffusion.py holds the kernels to.

Measured here (GRI-Mech 3.0 unless said otherwise):
* golden D(CH4, O2) at 2 atm, 500 K = 0.2795563576 cm2/s (Chemkin): direct Chapman-Enskog with Neufeld's Omega11*
  0.2777265 (-6.5e-3), ln-T cubic 0.2775353 (-7.2e-3) -- the gap between Neufeld's correlation and TRANLIB's
  tabulated collision integral, as 1.1e-3 on the viscosity goldens;
* ckmi_diffusion_fit against np.polyfit on the same grid: 6.4e-14 on D over [300, 3500] K; fit against the direct
  form: 7.9e-3 at most over all pairs;
* the float64 reference on the 30 test states of the five mechanisms: mass conservation <= 2.5e-15,
  Stefan-Maxwell <= 1.8e-13, element-wise error against the longdouble elimination <= 6.4e-15 of max |D| (the figures move
  in the last digit with the LAPACK build).
"""
import numpy as np
import pytest

import diffusion_cases as dc
import diffusion_reference as dr
from conftest import P_ATM, golden


@pytest.fixture(scope="module")
def gri():
    mech = dc.mechanism("gri")
    return mech, dc.transport_params("gri"), dc.native_fits("gri")


def test_golden_binary_diffusivity(gri):
    """Chemkin's D(CH4, O2) at 2 atm and 500 K within 1e-2: the restatement, direct and fitted, and the native fit."""
    mech, params, nf = gri
    g = golden("speciesproperties_diffusivity")
    j, k = (mech.species.index(s) for s in g["species"])
    T, P, val = g["temperature_K"], g["pressure_atm"] * P_ATM, g["state-binary_diffusivity"][0]
    direct = dr.binary_exact(T, P, mech.wt, params)[j, k]
    fitted = dr.binary_from_fits([T], [P], dr.binary_fits(mech.wt, params))[0][j, k]
    native = dr.binary_from_fits([T], [P], nf)[0][j, k]
    print(f"golden {val:.10f} direct {direct:.10f} ({direct / val - 1:+.2e}) polyfit {fitted:.10f} "
          f"({fitted / val - 1:+.2e}) native {native:.10f} ({native / val - 1:+.2e})")
    for v in (direct, fitted, native):
        assert abs(v / val - 1) < 1e-2
    assert abs(direct / val - 1) > 1e-3  # the Neufeld-vs-table gap is real: a closer match would be an accident


def test_native_fit_matches_polyfit(gri):
    """ckmi_diffusion_fit (Householder QR) against np.polyfit on the same 50 points.  The ln T Vandermonde matrix
    on [ln 300, ln 3500] has a condition number of ~1e7 in this basis, so two backward-stable solvers may differ by
    ~1e7 eps ~ 1e-9 in a coefficient; the fitted D, which is what the solvers minimise, agrees far better: the
    bar is the viscosity fit's 1e-11 inside the interval (measured 6.4e-14) and 1e-10 extrapolated to 5000 K."""
    mech, params, nf = gri
    pf = dr.binary_fits(mech.wt, params)
    T = np.unique(np.r_[np.linspace(250.0, 5000.0, 120), 300.0, 3500.0])  # the fit error peaks at the ends
    one = np.full_like(T, P_ATM)
    a, b = dr.binary_from_fits(T, one, nf), dr.binary_from_fits(T, one, pf)
    inside = (T >= 300.0) & (T <= 3500.0)
    e_in, e_all = np.max(np.abs(a[inside] / b[inside] - 1)), np.max(np.abs(a / b - 1))
    ex = np.stack([dr.binary_exact(t, P_ATM, mech.wt, params) for t in T[inside]])
    e_fit = np.max(np.abs(a[inside] / ex - 1))
    print(f"native vs polyfit: {e_in:.2e} inside, {e_all:.2e} to 5000 K; fit vs direct {e_fit:.2e}")
    assert e_in < 1e-11 and e_all < 1e-10
    assert e_fit < 1e-2  # the cubic in ln T against kinetic theory itself (measured 7.9e-3)


def test_fit_properties(gri):
    mech, params, nf = gri
    assert nf.shape == (mech.KK, mech.KK, 4)
    assert np.array_equal(nf, nf.transpose(1, 0, 2))  # symmetric, exactly
    # D scales as 1 / P
    T = np.array([400.0, 1700.0])
    d1, d7 = dr.binary_from_fits(T, [P_ATM] * 2, nf), dr.binary_from_fits(T, [7 * P_ATM] * 2, nf)
    assert np.max(np.abs(d1 / (7 * d7) - 1)) < 1e-15
    # polar - nonpolar pairs carry the induction correction, polar - polar and nonpolar - nonpolar do not
    # (like for like: the native fit against np.polyfit of the plain geometric / arithmetic rule, at 300 K.  For
    # H2O - N2 xi - 1 = alpha* mu*^2 sqrt(eps_p / eps_n) / 4 = 5.5e-2: eps_jk +11 %, sigma_jk -0.9 %, at
    # T* = 1.3 about -3 % in D (measured -3.1e-2); pairs of equal polarity agree to the fit agreement, 6e-14)
    sp = mech.species.index
    plain = dr.binary_from_fits([300.0], [P_ATM], dr.binary_fits(mech.wt, params, induction=False))[0]
    nat = dr.binary_from_fits([300.0], [P_ATM], nf)[0]
    assert params[sp("H2O"), 3] > 0 and params[sp("NH3"), 3] > 0 and params[sp("N2"), 3] == 0
    assert abs(nat[sp("H2O"), sp("N2")] / plain[sp("H2O"), sp("N2")] - 1) > 1e-2
    assert abs(nat[sp("H2O"), sp("NH3")] / plain[sp("H2O"), sp("NH3")] - 1) < 1e-11
    assert abs(nat[sp("O2"), sp("N2")] / plain[sp("O2"), sp("N2")] - 1) < 1e-11
    full = dr.binary_exact(1000.0, P_ATM, mech.wt, params)
    assert np.max(np.abs(dr.binary_from_fits([1000.0], [P_ATM], nf)[0] / full - 1)) < 1e-2


def test_fit_rejects_bad_parameters(gri):
    from pychemkin_amd import _native, transport

    mech, params, _ = gri
    for col, val in ((2, 0.0), (2, -3.4), (1, 0.0), (2, np.nan)):  # sigma <= 0, eps <= 0, a record that is missing
        bad = params.copy()
        bad[7, col] = val
        if np.isnan(val):
            bad[7, :] = np.nan
        with pytest.raises(_native.NativeError, match=r"code 1\).*species 7 needs.*sigma"):
            _native.diffusion_fit(mech.wt, bad, 300.0, 3500.0)
    with pytest.raises(_native.NativeError, match="tlow"):
        _native.diffusion_fit(mech.wt, params, 3500.0, 300.0)
    with pytest.raises(_native.NativeError):
        _native.diffusion_fit(mech.wt, params[:-1], 300.0, 3500.0)
    data = transport.parse_transport_text(open(dc.TRAN).read())
    del data["AR"]
    with pytest.raises(transport.TransportError, match="AR"):
        transport.species_params(data, mech.species)
    # the C entry point itself: CKMI_ERR_ARG = 1
    bad = params.copy()
    bad[0, 2] = 0.0
    out = np.zeros((mech.KK, mech.KK, 4))
    wt = np.ascontiguousarray(mech.wt, dtype=np.float64)
    assert _native.lib().ckmi_diffusion_fit(mech.KK, wt.ctypes.data, bad.ctypes.data, 300.0, 3500.0,
                                            out.ctypes.data) == 1
    assert _native.lib().ckmi_diffusion_fit(mech.KK, wt.ctypes.data, params.ctypes.data, 300.0, 3500.0,
                                            out.ctypes.data) == 0
    assert np.array_equal(out, _native.diffusion_fit(mech.wt, params, 300.0, 3500.0))


def test_python_layers_exist_without_gpu():
    """The public entry points are there (they are what a ported speciesproperties.py / createmixture.py calls)."""
    import pychemkin_amd as ck
    from pychemkin_amd import _native, transport

    for name in ("SpeciesDiffusionCoeffs", "diffusion_fits"):
        assert hasattr(ck.Chemistry, name)
    for name in ("species_Diffusion_Coeffs", "mixture_diffusion_coeffs", "mixture_binary_diffusion_coeffs"):
        assert callable(getattr(ck.Mixture, name))
    for name in ("binary_diffusion", "mixture_diffusion", "multicomponent_diffusion"):
        assert callable(getattr(_native.DeviceTransport, name))
    assert callable(transport.diffusion_fits)


def test_chemistry_diffusion_fits(gri):
    import pychemkin_amd as ck
    from conftest import CHEM, THERM, TRAN

    c = ck.Chemistry(chem=CHEM, therm=THERM, tran=TRAN, label="GRI 3.0 diffusion")
    c.preprocess()
    assert np.array_equal(c.diffusion_fits, gri[2])
    bare = ck.Chemistry(chem=CHEM, therm=THERM, label="GRI 3.0 no transport")
    bare.preprocess()
    with pytest.raises(Exception, match="no transport data"):
        bare.diffusion_fits


@pytest.mark.parametrize("name", list(dc.MECHS))
def test_reference_invariants(name):
    """The float64 reference on the six test states of every mechanism: D_ii = 0, mass conservation and the
    Stefan-Maxwell equations to 1e-12 (measured <= 2.5e-15 and <= 1.8e-13), and its element-wise error against
    the partial-pivoting Gauss-Jordan in longdouble (measured <= 6.4e-15 of max |D|), which sets the GPU test's
    tolerance."""
    mech = dc.mechanism(name)
    assert mech.KK == dc.MECHS[name]
    labels, T, P, Y = dc.states(name)
    ref = dc.reference(name)
    for s, lab in enumerate(labels):
        D = ref["multi"][s]
        print(f"{name:7s} {lab:26s} mass {ref['mass'][s]:.2e}  Stefan-Maxwell {ref['sm'][s]:.2e}  "
              f"vs longdouble {ref['err'][s]:.2e}")
        assert np.all(np.isfinite(D)) and np.all(np.diag(D) == 0.0)
        assert ref["mass"][s] < 1e-12
        assert ref["sm"][s] < 1e-12
        assert ref["err"][s] < 1e-10 / 100  # the GPU bar, 100 x this, stays below 1e-8 (no row equilibration needed)
    # the states are what they claim: zeros, traces and negative mass fractions are present
    assert np.any(Y[:, 3] == 0.0) and np.any((Y[:, 3] > 0) & (Y[:, 3] < 1e-6))
    assert np.any(Y[:, 4] < 0.0)
    assert np.count_nonzero(Y[:, 2]) == 1


def test_two_species_limit(gri):
    """A binary mixture: the multicomponent coefficient is the binary one, whatever the composition (H2 / N2 with
    their coefficient from the native fit table)."""
    mech, _, nf = gri
    pair = [mech.species.index("H2"), mech.species.index("N2")]
    Db = dr.binary_from_fits([1000.0], [P_ATM], nf)[0][np.ix_(pair, pair)]
    for x in (0.5, 0.03, 1e-9):
        D = dr.multicomponent_state(1000.0, P_ATM, np.array([x, 1.0 - x]), mech.wt[pair], Db)
        assert abs(D[0, 1] / Db[0, 1] - 1) < 1e-12 and abs(D[1, 0] / Db[0, 1] - 1) < 1e-12
        assert D[0, 0] == 0.0 and D[1, 1] == 0.0


def test_l_matrix_has_a_zero_diagonal(gri):
    """The triple sum cancels for j = i, so the first pivot of an elimination without row exchanges is rounding
    noise: the reason the kernels pivot."""
    mech, _, _ = gri
    _, T, P, _ = dc.states("gri")
    ref = dc.reference("gri")
    L = dr.l_matrix(T[3], P[3], ref["X"][3], mech.wt, ref["binary"][3])
    assert np.max(np.abs(np.diag(L))) < 1e-14 * np.max(np.abs(L))
