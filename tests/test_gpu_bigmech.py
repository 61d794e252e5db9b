"""Large-mechanism kernels (configs[4] size) on the synthetic 161-species mechanism.

No ~160-species mechanism exists offline, so these results are checked against the oracle
(itself checked against the numpy restatement on the same mechanism, test_oracle_independent.py)
and LAPACK, not against the reference: parity with Chemkin is unpinned for this size.
Tolerances as for GRI-3.0 (test_gpu_kernels.py): 1e-11 of the largest |wdot| of a state.
"""
import numpy as np
import pytest
import scipy.linalg as sla

from conftest import P_ATM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def big(big_mech):
    from oracle.oracle import Oracle
    from pychemkin_amd import _native

    return big_mech, Oracle(big_mech), _native.DeviceMechanism(big_mech.to_tables())


def _states(KK, n, seed):
    rng = np.random.default_rng(seed)
    T = rng.uniform(300.0, 3000.0, n)
    P = P_ATM * 10.0 ** rng.uniform(-1.0, 2.0, n)
    Y = rng.dirichlet(0.5 * np.ones(KK), n).T.copy()
    return T, P, Y


@pytest.mark.parametrize("n", [1, 7, 8, 17, 1000])
def test_rop_thermo_161_species(big, n):
    mech, orc, dm = big
    T, P, Y = _states(mech.KK, n, seed=n)
    w, cp, h = (x.cpu().numpy() for x in dm.rop_thermo(T, P, Y))
    wo, cpo, ho = orc.rop_batch(T, P, Y)
    scale = np.max(np.abs(wo), axis=0, keepdims=True)
    assert np.max(np.abs(w - wo) / scale) < 1e-11
    assert np.max(np.abs(cp / cpo - 1)) < 1e-12
    assert np.max(np.abs(h - ho) / np.max(np.abs(ho))) < 1e-12
    # the tracer block (species 53..160) is active, not all zero
    assert np.max(np.abs(w[53:])) > 0


def test_reaction_rates_and_thermo_161_species(big):
    mech, orc, dm = big
    T, P, Y = _states(mech.KK, 19, seed=3)
    qf, qr = (x.cpu().numpy() for x in dm.reaction_rates(T, P, Y))
    for j in range(T.size):
        qfo, qro, _ = orc.rates(T[j], P[j], Y[:, j])
        sc = max(np.max(np.abs(qfo)), np.max(np.abs(qro)))
        assert np.max(np.abs(qf[:, j] - qfo)) < 1e-11 * sc
        assert np.max(np.abs(qr[:, j] - qro)) < 1e-11 * sc
    cp, hh, s = (x.cpu().numpy() for x in dm.species_thermo(T))
    for j in range(T.size):
        cpo, ho, so = orc.thermo(T[j])
        assert np.allclose(cp[:, j], cpo, rtol=1e-13, atol=0)
        assert np.allclose(hh[:, j], ho, rtol=1e-12, atol=1e-12)


def test_newton_matrices_161_species_lu(big):
    """Newton matrices I - gamma J of the 161-species mechanism (n = 162, J from the oracle's
    analytic Jacobian at burning states) through ckmi_lu_factor_batched: LAPACK pivots exactly,
    factors to rounding."""
    import torch
    from pychemkin_amd import _native

    mech, orc, _ = big
    rng = np.random.default_rng(11)
    mats = []
    for i in range(12):
        T = rng.uniform(1200.0, 2800.0)
        Y = rng.dirichlet(0.5 * np.ones(mech.KK))
        y = np.concatenate([[T], Y])
        _, J = orc.rhs_jac(y, problem=1 + i % 2, P0=P_ATM * 10.0 ** rng.uniform(0, 2))
        gamma = 10.0 ** rng.uniform(-9, -6)
        mats.append(np.eye(y.size) - gamma * J)
    A = np.stack(mats)
    At = torch.as_tensor(A.copy(), device="cuda:0")
    _, piv, info = _native.lu_factor_batched(At)
    LU, piv, info = At.cpu().numpy(), piv.cpu().numpy(), info.cpu().numpy()
    assert np.all(info == 0)
    for s in range(A.shape[0]):
        lu_ref, piv_ref = sla.lu_factor(A[s])
        np.testing.assert_array_equal(piv[s], piv_ref)
        np.testing.assert_allclose(LU[s], lu_ref, rtol=0, atol=1e-12 * np.abs(lu_ref).max())


def test_reactor_run_rejects_more_than_191_species_loudly(tmp_path):
    """161 species run on the workgroup-per-reactor kernel (test_gpu_bigreactor.py); above KK = 191 the
    Newton matrix no longer fits the register file of a CU, and ckmi_reactor_run says so."""
    import sys

    from pychemkin_amd import _native
    from pychemkin_amd.mechanism import Mechanism

    sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1] / "data"))
    from make_tracer_mechanism import write_big_mechanism

    cp, tp = write_big_mechanism(str(tmp_path), n_tracer=150)  # 203 species
    mech = Mechanism.from_files(cp, tp)
    assert mech.KK == 203
    dm = _native.DeviceMechanism(mech.to_tables())
    Y0 = np.zeros((1, mech.KK))
    Y0[0, mech.species.index("N2")] = 1.0
    with pytest.raises(_native.NativeError, match="191 species"):
        dm.reactor_run(_native.make_cfg(energy=1, t_end=1e-3), np.ones(1, np.int32), [1000.0], [P_ATM], [1.0], Y0)
    # the rate kernels still take it (mechanism image up to 255 species): the oracle's rates at this file's bars
    from oracle.oracle import Oracle

    T, P, Y = np.array([1500.0]), np.array([P_ATM]), np.full((mech.KK, 1), 1.0 / mech.KK)
    w, cp, h = (x.cpu().numpy() for x in dm.rop_thermo(T, P, Y))
    wo, cpo, ho = Oracle(mech).rop_batch(T, P, Y)
    assert np.max(np.abs(w - wo)) < 1e-11 * np.max(np.abs(wo))
    assert np.max(np.abs(cp / cpo - 1)) < 1e-12 and np.max(np.abs(h - ho) / np.max(np.abs(ho))) < 1e-12
    assert np.max(np.abs(w[53:])) > 0


def test_drop_in_api_on_161_species_mechanism(big):
    """Chemistry.preprocess / Mixture.ROP / RxnRates / HML / CPBL (the reference's public names,
    mixture.py:1693-1808) on the 161-species mechanism, through the GPU kernels."""
    import pychemkin_amd as ck
    from conftest import BIG_CHEM, BIG_THERM

    mech, orc, _ = big
    chem = ck.Chemistry(label="tracer161")
    chem.chemfile = BIG_CHEM
    chem.thermfile = BIG_THERM
    chem.preprocess()
    assert chem.KK == 161 and chem.IIGas == 505
    m = ck.Mixture(chem)
    m.temperature = 1700.0
    m.pressure = 3 * P_ATM
    m.X = [("CH4", 0.05), ("O2", 0.15), ("N2", 0.6), ("OH", 0.01), ("AX1", 0.1), ("AX60", 0.05), ("AX108", 0.04)]
    qfo, qro, wo = orc.rates(1700.0, 3 * P_ATM, m.Y)
    assert np.max(np.abs(m.ROP() - wo)) < 1e-11 * np.max(np.abs(wo))
    qf, qr = m.RxnRates(reference_compat=False)
    assert np.max(np.abs(qf - qfo)) < 1e-11 * np.max(np.abs(qfo))
    assert np.max(np.abs(qr - qro)) < 1e-11 * np.max(np.abs(qro))
    # tracer exchange AX1 + H <=> AX2 + H carries a nonzero rate
    assert np.abs(m.ROP()[chem.get_specindex("AX2")]) > 0
