"""Host side of the equilibrium functions: signatures, argument errors, the options the drop-in refuses,
fraction modes.  No GPU: the device call is replaced by the numpy reference where a result is needed."""
import inspect

import numpy as np
import pytest

from conftest import P_ATM
from equilibrium_reference import EquilibriumReference


def test_names_and_signatures():
    import pychemkin_amd as ck
    from pychemkin_amd import mixture

    for name in ("calculate_equilibrium", "equilibrium", "detonation"):
        assert getattr(ck, name) is getattr(mixture, name)
    assert list(inspect.signature(ck.calculate_equilibrium).parameters) == [
        "chemID", "p", "t", "frac", "wt", "mode_in", "mode_out", "EQOption", "useRealGas"]
    sig = inspect.signature(ck.calculate_equilibrium).parameters
    assert sig["EQOption"].default == 1 and sig["useRealGas"].default == 0
    assert list(inspect.signature(ck.equilibrium).parameters) == ["mixture", "opt"]
    assert inspect.signature(ck.equilibrium).parameters["opt"].default == 1
    assert list(inspect.signature(ck.detonation).parameters) == ["mixture"]
    assert list(inspect.signature(ck.Mixture.Find_Equilibrium).parameters) == ["self"]
    assert list(inspect.signature(ck.BatchEquilibrium.run).parameters) == ["self", "option", "T", "P", "X", "Y"]
    assert [f for f in ck.EquilibriumResult.__dataclass_fields__][:7] == [
        "T", "P", "Y", "sound", "detspeed", "iterations", "status"]
    assert sorted(mixture.EQUILIBRIUM_OPTIONS) == list(range(1, 11))


def _mix(chem):
    import pychemkin_amd as ck

    m = ck.Mixture(chem)
    m.temperature, m.pressure = 1000.0, P_ATM
    m.X = [("CH4", 0.1), ("O2", 0.21), ("N2", 0.79)]
    return m


def test_argument_errors(chem):
    import pychemkin_amd as ck
    from pychemkin_amd.mixture import MixtureError

    m = _mix(chem)
    wt = chem.WT
    with pytest.raises(MixtureError, match="invalid chemistry"):
        ck.calculate_equilibrium(-1, P_ATM, 1000.0, m.X, wt, "mole", "mole")
    with pytest.raises(MixtureError, match="pressure and/or temperature"):
        ck.calculate_equilibrium(chem.chemID, -1.0, 1000.0, m.X, wt, "mole", "mole")
    with pytest.raises(MixtureError, match="pressure and/or temperature"):
        ck.calculate_equilibrium(chem.chemID, P_ATM, 0.0, m.X, wt, "mole", "mole")
    with pytest.raises(MixtureError, match="same size"):
        ck.calculate_equilibrium(chem.chemID, P_ATM, 1000.0, m.X[:-1], wt, "mole", "mole")
    with pytest.raises(MixtureError, match='"mole" or "mass"'):
        ck.calculate_equilibrium(chem.chemID, P_ATM, 1000.0, m.X, wt, "volume", "mole")
    with pytest.raises(MixtureError, match='"mole" or "mass"'):
        ck.calculate_equilibrium(chem.chemID, P_ATM, 1000.0, m.X, wt, "mole", "volume")
    with pytest.raises(MixtureError, match="Mixture object"):
        ck.equilibrium("not a mixture", 1)
    with pytest.raises(MixtureError, match="Mixture object"):
        ck.detonation(None)


@pytest.mark.parametrize("opt", [3, 6, 9, 10])
def test_equilibrium_refuses_the_options_the_reference_refuses(chem, opt):
    import pychemkin_amd as ck
    from pychemkin_amd.mixture import MixtureError

    with pytest.raises(MixtureError, match=f"option {opt} is not available"):
        ck.equilibrium(_mix(chem), opt)


def test_real_gas_raises(chem):
    import pychemkin_amd as ck
    from pychemkin_amd.mixture import MixtureError

    m = _mix(chem)
    with pytest.raises(MixtureError, match="real-gas"):
        ck.calculate_equilibrium(chem.chemID, P_ATM, 1000.0, m.X, chem.WT, "mole", "mole", useRealGas=1)
    m._EOS, m.userealgas = 1, True
    with pytest.raises(MixtureError, match="real-gas"):
        ck.equilibrium(m, 1)
    with pytest.raises(MixtureError, match="real-gas"):
        ck.detonation(m)


class _FakeDevice:
    """Stands in for DeviceMechanism.equil_run with the numpy reference (host tensors)."""

    def __init__(self, mech):
        self.ref = EquilibriumReference(mech)
        self.calls = []

    def equil_run(self, option, T, P, Y, **kw):
        import torch

        self.calls.append((np.asarray(option).tolist(), np.asarray(Y).copy()))
        r = self.ref.solve(option, T, P, Y)
        st = np.stack([r["iterations"], r["status"], r["cj_iterations"], 0 * r["status"]], axis=1).astype(np.int32)
        return {k: torch.as_tensor(v) for k, v in dict(T=r["T"], P=r["P"], Y=r["Y"], sound=r["sound"],
                                                       detspeed=r["detspeed"], stats=st).items()}


def test_fraction_modes_and_option_handling(chem, mech, monkeypatch):
    """'mass' and 'mole' in and out describe the same state; an option outside 1..10 is read as 1; the
    mixture functions return copies at the equilibrium T and P."""
    import pychemkin_amd as ck

    fake = _FakeDevice(mech)
    monkeypatch.setattr(type(chem), "device_mechanism", lambda self, device=None: fake)
    m = _mix(chem)
    sv_x, x = ck.calculate_equilibrium(chem.chemID, P_ATM, 1000.0, 5 * m.X, chem.WT, "mole", "mole", EQOption=5)
    sv_y, y = ck.calculate_equilibrium(chem.chemID, P_ATM, 1000.0, m.Y, chem.WT, "mass", "mass", EQOption=5)
    # the same mass fractions go down: two normalisation orders of fractions <= 1, a few ulp (2.2e-16) apart
    assert np.max(np.abs(fake.calls[0][1] - fake.calls[1][1])) < 1e-15
    assert abs(sv_x[1] / sv_y[1] - 1) < 1e-12 and sv_x[0] == P_ATM and sv_x[2] == sv_x[3] == 0.0
    assert abs(x.sum() - 1) < 1e-14 and abs(y.sum() - 1) < 1e-14
    assert np.max(np.abs(ck.Mixture.mole_fraction_to_mass_fraction(x, chem.WT) - y)) < 1e-12
    ck.calculate_equilibrium(chem.chemID, P_ATM, 1000.0, m.X, chem.WT, "mole", "mole", EQOption=42)
    assert fake.calls[-1][0] == [1]
    hp = ck.equilibrium(m, 5)
    assert hp is not m and m.temperature == 1000.0 and abs(hp.temperature / sv_y[1] - 1) < 1e-12
    assert np.max(np.abs(hp.Y - y)) < 1e-12
    speeds, cj = ck.detonation(m)
    assert fake.calls[-1][0] == [10] and speeds[1] > speeds[0] > 0 and cj.pressure > 5 * P_ATM
    tp = m.Find_Equilibrium()
    assert fake.calls[-1][0] == [1] and tp.temperature == 1000.0 and tp.pressure == P_ATM
