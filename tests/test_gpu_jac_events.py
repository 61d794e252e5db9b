"""A reactor's result does not depend on who shares its workgroup.

The waves of a workgroup of reactor_kernel share one FP64 Jacobian scratch behind a lock.  A with_j call of
reactor_rhs takes the lock itself, at its first touch of the scratch (behind its prologue), zeroes the scratch
and returns holding the lock; ST_NLS_J copies the Jacobian out and releases it.  Two waves inside one scratch,
or a scratch zeroed under another wave, cannot leave its N^2 entries bitwise intact, so every reactor must
return bit for bit what it returns when it runs alone (n = 1: one wave, nobody to share with), whether it ran
in a full workgroup (12 reactors on the FP32-inverse kernel, 8 on the FP64-inverse one: every wave wants the
scratch at step 0 and again at every refresh) or beside a second workgroup (13 reactors).

The comparison is exact (every bit of tau, T, P, V, Y, stats, t_stop): no tolerance is involved.
"""
import numpy as np
import pytest

import mechanism_variants as mv
from conftest import P_ATM, gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

RUN = dict(energy=1, t_end=1.0, atol=1e-10, rtol=1e-8, ign_mode="TIFP")  # RUN of test_gpu_jac_single_eval.py
NJE, STATUS = 2, 6
KEYS = ("tau", "T", "P", "V", "Y", "stats", "t_stop")


def _np(res):
    return {k: res[k].cpu().numpy() for k in KEYS}


def _run(dm, inp, sel, path):
    """One launch of the reactors inp[sel] on the forced path."""
    from pychemkin_amd import _native

    prob, T0, P0, Y0 = (np.ascontiguousarray(inp[k][sel]) for k in ("prob", "T0", "P0", "Y0"))
    _native.set_reactor_path(path)
    try:
        return _np(dm.reactor_run(_native.make_cfg(**RUN), prob, T0, P0, np.ones(len(prob)), Y0))
    finally:
        _native.set_reactor_path(0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _assert_same(joint, solo, what):
    """joint: the result of one launch of n reactors; solo[i]: the result of reactor i run alone."""
    n = len(solo)
    assert np.all(joint["stats"][:, NJE] >= 1), (what, joint["stats"][:, NJE])
    for i in range(n):
        assert solo[i]["stats"][0, NJE] >= 1, (what, i, solo[i]["stats"][0].tolist())
        for k in KEYS:
            a, b = joint[k][i], solo[i][k][0]
            assert np.array_equal(_bits(a), _bits(b)), (what, "reactor", i, k, a, b)


@pytest.fixture(scope="module")
def gri(mech, tables):
    """The first 13 reactors of the mix of test_gpu_jac_single_eval.py, and each of them run alone."""
    import bench
    from pychemkin_amd import _native

    T0, P0, Y0, prob = bench.sweep_c4(mech, 1, 0)
    idx = (16411 * np.arange(64))[:13]
    inp = dict(T0=T0[idx], P0=P0[idx], Y0=Y0[idx], prob=prob[idx])
    dm = _native.DeviceMechanism(tables)
    yield dict(dm=dm, inp=inp, solo={})
    dm.close()


def _solo(g, path, n):
    """Reactors 0..n-1 alone on `path`, run once per module and path and never changed."""
    for i in range(n):
        if (path, i) not in g["solo"]:
            g["solo"][(path, i)] = _run(g["dm"], g["inp"], slice(i, i + 1), path)
    return [g["solo"][(path, i)] for i in range(n)]


def test_one_full_workgroup_fp32_inverse(gri):
    """12 reactors on reactor_kernel<54, false, false>: grid = ceil(12 / 12) = 1, all 12 waves share the scratch."""
    joint = _run(gri["dm"], gri["inp"], slice(0, 12), 3)
    _assert_same(joint, _solo(gri, 3, 12), "12 joint, path 3")


def test_two_workgroups_fp32_inverse(gri):
    """13 reactors: a full workgroup and a second one whose other waves find the queue empty."""
    joint = _run(gri["dm"], gri["inp"], slice(0, 13), 3)
    _assert_same(joint, _solo(gri, 3, 13), "13 joint, path 3")


def test_one_full_workgroup_fp64_inverse(gri):
    """8 reactors on reactor_kernel<54, false, true>, the 8-wave variant (CONP / CONV, the plug-flow build)."""
    joint = _run(gri["dm"], gri["inp"], slice(0, 8), 2)
    _assert_same(joint, _solo(gri, 2, 8), "8 joint, path 2")


def _subset_inputs(mech):
    """12 CH4/air reactors around the conditions of mechanism_variants.wave_reference, CONP / CONV alternating."""
    cases = [(1200, 1, 1.0), (1400, 10, 1.0), (1600, 50, 1.5), (1300, 30, 0.5), (1250, 2, 0.8), (1500, 20, 1.2),
             (1350, 5, 0.6), (1450, 40, 1.0), (1550, 1, 2.0), (1700, 10, 0.7), (1150, 50, 1.0), (1650, 3, 1.3)]
    T0 = np.array([c[0] for c in cases], float)
    P0 = np.array([c[1] for c in cases], float) * P_ATM
    Y0 = np.stack([mv.wave_Y(mech, c[2])[0] for c in cases])
    prob = np.array([1, 2] * 6, np.int32)
    return dict(T0=T0, P0=P0, Y0=Y0, prob=prob)


@pytest.mark.parametrize("name", ["subset31", "subset32"])
def test_small_variants(name):
    """subset31: reactor_kernel<32>, nvar 32, the matrix exactly full (N / 2 = 16 column pairs per pivot step);
    subset32: nvar 33 on reactor_kernel<54>, 21 padded columns.  12 reactors in one workgroup against each alone."""
    from pychemkin_amd import _native

    mech = mv.wave_mechanism(name)
    assert mv.wave_variant(mech.KK + 1, False)[0] == mv.WAVE_CASES[name][1][0]
    inp = _subset_inputs(mech)
    dm = _native.DeviceMechanism(mech.to_tables())
    try:
        joint = _run(dm, inp, slice(0, 12), 3)
        solo = [_run(dm, inp, slice(i, i + 1), 3) for i in range(12)]
    finally:
        dm.close()
    assert np.all(joint["stats"][:, STATUS] == 0), joint["stats"][:, STATUS]
    _assert_same(joint, solo, name)
