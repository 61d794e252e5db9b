"""The reactor kernel's strips read a slot's records as one batch (strip_head, ckmi_reactor.hpp): every lane of a
strip, padding lanes included, reads info, the species slots, the Arrhenius terms and GFAC ahead of the test that
skips an empty slot.  Checked where that can go wrong: at the padding of the last strip.

Three images cut from GRI-Mech 3.0 by leaving reactions out (same 53 species, so the states and the metrics of
tests/jacobian_cases.py apply unchanged):

* full64    the first 320 reactions: 320 slots, exactly five strips, no padding lane anywhere;
* plus1     the first 256 elementary reactions and the file's last falloff reaction: four full elementary strips and
            a falloff strip that holds ONE reaction in its first lane and 63 padding lanes (257 slots, IIp = 320).
            Cutting from the end of the reaction block alone never gives 64 k + 1 slots: the builder pads the
            elementary block to a strip boundary whenever that adds no strip (order_slots, ckmi_mech_host.cpp), so
            the count jumps past it; the third-body and the other falloff reactions are left out as well;
* one       the first 63 reactions: one strip of mixed types with one padding lane.

The host half (no GPU) proves these numbers from the images themselves, built by tests/strip_layout_host.cpp
(II, IIp, slots in use, padding slots inside); the GPU half checks the device's own slot map against them, then
(a) f of both passes and every Jacobian entry of ckmi_reactor_rhs_jac -- the integrator's own reactor_rhs -- against
    the oracle at the allowances of tests/test_gpu_jacobian.py, four states x problems 1, 2 per image;
(b) twelve reactors (one full workgroup of the wave kernel) through reactor_run against the oracle at the bars of
    tests/test_gpu_reactor.py;
(c) GFAC = 2 on plus1, and an A-factor perturbation of the first and of the last slot of the last strip of full64
    (lanes 0 and 63) and of plus1's lone falloff slot, entry by entry as in (a): GFAC and the perturbation are read
    at other places than the slot's records.
"""
import functools
import os
import tempfile

import numpy as np
import pytest

import jacobian_cases as jc
from mechanism_variants import CHEM, P_ATM, THERM

IMAGES = ("full64", "plus1", "one")
# name -> (slots in use, IIp, padding slots below the slots in use)
EXPECT = {"full64": (320, 320, 0), "plus1": (257, 320, 0), "one": (63, 64, 0)}
STATES = (0, 1, 2, 3)  # unburnt, induction, max dT/dt, burnt (jacobian_cases.STATE_NAMES) of the GRI-3.0 run
RUN = dict(energy=1, t_end=0.05, atol=1e-10, rtol=1e-8, ign_mode="TIFP")
MAJOR = ("CH4", "O2", "N2", "H2O", "CO2", "CO", "H2")  # tests/test_gpu_reactor.py
_TMP = []


# ---------------------------------------------------------------------- inputs
def _reaction_blocks():
    """(head lines, [lines of reaction i with its auxiliary lines], tail) of GRI-Mech 3.0's file."""
    lines = open(CHEM).read().split("\n")
    i0 = next(i for i, l in enumerate(lines) if l.strip().upper().startswith("REACTIONS"))
    i1 = max(i for i, l in enumerate(lines) if l.strip().upper() == "END")
    blocks = []
    for l in lines[i0 + 1:i1]:
        if "=" in l.split("!")[0]:
            blocks.append([l])
        elif blocks and l.split("!")[0].strip():
            blocks[-1].append(l)
    return lines[:i0 + 1], blocks, ["END", ""]


@functools.lru_cache(maxsize=None)
def kept_reactions(name):
    """Indices (file order) of the GRI-3.0 reactions an image keeps."""
    rtype = np.asarray(jc.mechanism("gri").to_tables()["rtype"])
    if name == "full64":
        return tuple(range(320))
    if name == "one":
        return tuple(range(63))
    last_falloff = int(np.nonzero(rtype == 2)[0][-1])
    return tuple(int(i) for i in np.nonzero(rtype == 0)[0][:256]) + (last_falloff,)


@functools.lru_cache(maxsize=None)
def image_files(name):
    if not _TMP:
        _TMP.append(tempfile.TemporaryDirectory(prefix="ckmi_strip_reads_"))
    head, blocks, tail = _reaction_blocks()
    path = os.path.join(_TMP[0].name, name + "_chem.inp")
    with open(path, "w") as f:
        f.write("\n".join(head + [l for i in kept_reactions(name) for l in blocks[i]] + tail))
    return path, THERM


@functools.lru_cache(maxsize=None)
def mechanism(name):
    from pychemkin_amd.mechanism import Mechanism

    return Mechanism.from_files(*image_files(name))


@functools.lru_cache(maxsize=None)
def oracle(name):
    from oracle.oracle import Oracle

    return Oracle(mechanism(name))


def probe_arrays():
    """The launch of (a): STATES x problems 1, 2 of GRI-3.0's probe states (jacobian_cases.launch_arrays)."""
    a = jc.launch_arrays(jc.Case("strip-reads", "gri"))
    sel = np.isin(a["state"], STATES)
    return {k: v[sel] for k, v in a.items()}


def reactor_inputs(mech):
    """Twelve CH4/air reactors: one full workgroup of the wave kernel, CONP and CONV alternating."""
    from conftest import ch4_air_Y

    # (hot enough that the one-strip image, which lacks most of the chain, ignites well inside t_end everywhere)
    T0 = np.linspace(1600.0, 1900.0, 12)
    P0 = P_ATM * np.tile([1.0, 10.0, 40.0], 4)
    Y0 = ch4_air_Y(mech, np.tile([0.6, 1.0, 1.0, 1.6], 3))
    prob = np.where(np.arange(12) % 2 == 0, 1, 2).astype(np.int32)
    return T0, P0, Y0, prob


# ---------------------------------------------------------------------- host half
@pytest.fixture(scope="module")
def layouts():
    from test_strip_layout_host import run_layout

    out, last = run_layout([image_files(n) for n in IMAGES])
    assert last.endswith(" 0 violations"), last
    return {n: [l for l in out if os.path.basename(l["where"]) == n + "_chem.inp"] for n in IMAGES}


@pytest.mark.parametrize("name", IMAGES)
def test_images_have_the_padding_they_are_named_for(name, layouts):
    used, IIp, pads = EXPECT[name]
    mech = mechanism(name)
    assert mech.species == jc.mechanism("gri").species and mech.II == len(kept_reactions(name))
    both = layouts[name]
    assert [l["order"] for l in both] == ["annealed", "file_order"], both
    for l in both:
        assert (l["KK"], l["II"], l["IIp"], l["used"], l["pads_inside"]) == (53, mech.II, IIp, used, pads), l
    assert used == mech.II + pads
    if name == "full64":
        assert used % 64 == 0 and used == IIp              # no padding lane in any strip
    elif name == "plus1":
        assert used % 64 == 1 and IIp - used == 63         # 63 padding lanes beside one reaction
        rtype = np.asarray(mech.to_tables()["rtype"])
        assert rtype[-1] == 2 and np.all(rtype[:-1] == 0)  # that reaction is a falloff reaction
    else:
        assert used < 64 and IIp == 64                     # one strip
        assert set(np.asarray(mech.to_tables()["rtype"]).tolist()) == {0, 1, 2}  # of every type


def test_probe_states_and_reactors_are_what_the_gpu_half_assumes():
    a = probe_arrays()
    assert a["t"].size == 8 and sorted(set(a["state"].tolist())) == list(STATES)
    assert sorted(set(a["problem"].tolist())) == [1, 2]
    for name in IMAGES:
        T0, P0, Y0, prob = reactor_inputs(mechanism(name))
        assert T0.size == 12 and np.allclose(Y0.sum(axis=1), 1.0) and set(prob.tolist()) == {1, 2}


# ---------------------------------------------------------------------- GPU half
@pytest.fixture(scope="module")
def devs():
    from pychemkin_amd import _native

    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _native.DeviceMechanism(mechanism(name).to_tables(), device=0)
        return cache[name]

    yield get
    for dm in cache.values():
        dm.close()


def _probe(dm, a, jac, cfg=None, afac_rxn=None, afac=None):
    from pychemkin_amd import _native

    kw = {}
    if afac_rxn is not None:
        kw = dict(afac_rxn=np.full(a["t"].size, afac_rxn, np.int32), afac=np.full(a["t"].size, afac))
    f, J = dm.rhs_jac(_native.make_cfg(energy=1, **(cfg or {})), a["problem"], a["T0"], a["P0"], a["V0"], a["Y0"],
                      a["t"], a["y"], jac=jac, **kw)
    return f.cpu().numpy(), (J.cpu().numpy() if J is not None else None)


def _reference(name, a, **cfg):
    orc, mech = oracle(name), mechanism(name)
    n = a["t"].size
    f, J = np.zeros((n, mech.KK + 1)), np.zeros((n, mech.KK + 1, mech.KK + 1))
    for i in range(n):
        rho0 = a["P0"][i] / (jc.RU * a["T0"][i]) / np.sum(a["Y0"][i] / mech.wt)
        f[i], J[i] = orc.rhs_jac(a["y"][i], problem=int(a["problem"][i]), energy=1, rho0=rho0, V0=a["V0"][i],
                                 P0=a["P0"][i], t=a["t"][i], **cfg)
    return f, J


def _check_probe(tag, name, dm, cfg=None, ref_cfg=None, afac_rxn=None, afac=None):
    """f of both passes and every Jacobian entry against the oracle, at test_gpu_jacobian.py's allowances."""
    from test_gpu_jacobian import BOUND_F, BOUND_J

    a = probe_arrays()
    f_plain, _ = _probe(dm, a, False, cfg, afac_rxn, afac)
    f_j, J = _probe(dm, a, True, cfg, afac_rxn, afac)
    f_ref, J_ref = _reference(name, a, **(ref_cfg or {}))
    case = jc.Case(tag, "gri")  # the metrics need the species' thermodynamics and weights only: GRI-3.0's
    wt = mechanism(name).wt
    assert np.isfinite(f_plain).all() and np.isfinite(f_j).all() and np.isfinite(J).all()
    ep, ej = jc.f_errors(case, a, f_plain, f_ref), jc.f_errors(case, a, f_j, f_ref)
    eb = [jc.j_error(wt, J[i], J_ref[i]) for i in range(J.shape[0])]
    print(f"STRIP {tag}: f plain {ep[0].max():.2e} {ep[1].max():.2e}  with_j {ej[0].max():.2e} {ej[1].max():.2e}  "
          f"J {max(eb):.2e}  (bounds {BOUND_F:.2e}, {BOUND_J:.2e})")
    for e in ep + ej:
        assert e.max() <= BOUND_F, (tag, jc.STATE_NAMES[a["state"][int(np.argmax(e))]], e.max())
    assert max(eb) <= BOUND_J, (tag, jc.STATE_NAMES[a["state"][int(np.argmax(eb))]], max(eb))
    return f_plain, J


@pytest.mark.gpu
@pytest.mark.parametrize("name", IMAGES)
def test_device_slot_map_matches_the_host_image(name, devs):
    slot = devs(name).slot_of()
    assert len(set(slot.tolist())) == slot.size and int(slot.max()) + 1 == EXPECT[name][0]
    if name == "plus1":
        assert int(slot[-1]) == 256  # the falloff reaction: first lane of the last strip


@pytest.mark.gpu
@pytest.mark.parametrize("name", IMAGES)
def test_rhs_and_jacobian_entry_by_entry(name, devs):
    _check_probe(name, name, devs(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", IMAGES)
def test_twelve_reactors_match_the_oracle(name, devs):
    from pychemkin_amd import _native

    mech, dm = mechanism(name), devs(name)
    T0, P0, Y0, prob = reactor_inputs(mech)
    res = {k: v.cpu().numpy() for k, v in dm.reactor_run(_native.make_cfg(**RUN), prob, T0, P0, np.ones(12), Y0).items()}
    nfail, ref, Yref = oracle(name).reactor_batch(T0, P0, Y0, problem=prob, V0=np.ones(12), **RUN)
    assert nfail == 0
    worst = [0.0, 0.0, 0.0]
    for i, r in enumerate(ref):  # the bars of tests/test_gpu_reactor.py _check
        assert res["stats"][i, 6] == r.status == 0, (name, i)
        if r.tau > 0:
            worst[0] = max(worst[0], abs(res["tau"][i] / r.tau - 1))
            assert abs(res["tau"][i] / r.tau - 1) < 1e-4, (name, i, res["tau"][i], r.tau)
        else:
            assert res["tau"][i] == r.tau, (name, i, res["tau"][i], r.tau)
        worst[1] = max(worst[1], abs(res["T"][i] / r.T - 1))
        assert abs(res["T"][i] / r.T - 1) < 1e-4, (name, i, res["T"][i], r.T)
        for sp in MAJOR:
            k = mech.species.index(sp)
            worst[2] = max(worst[2], abs(res["Y"][i, k] - Yref[i][k]) / max(abs(Yref[i][k]), 1e-3))
            assert abs(res["Y"][i, k] - Yref[i][k]) <= 1e-4 * max(abs(Yref[i][k]), 1e-3), (name, i, sp)
    print(f"STRIP reactors {name}: tau {worst[0]:.2e} T {worst[1]:.2e} major Y {worst[2]:.2e}")


@pytest.mark.gpu
def test_gfac_on_the_padded_falloff_strip(devs):
    f2, J2 = _check_probe("plus1-gfac2", "plus1", devs("plus1"), cfg=dict(gfac=2.0), ref_cfg=dict(gfac=2.0))
    f1, _ = _probe(devs("plus1"), probe_arrays(), False)
    assert not np.array_equal(f1, f2)  # GFAC reached the kernel


@pytest.mark.gpu
@pytest.mark.parametrize("name,lane", [("full64", 0), ("full64", 63), ("plus1", 0)])
def test_afactor_perturbation_at_the_ends_of_the_last_strip(name, lane, devs):
    dm = devs(name)
    slot = dm.slot_of()
    last = (int(slot.max()) // 64) * 64
    hit = np.nonzero(slot == last + lane)[0]
    assert hit.size == 1, (name, lane)  # a reaction sits in that lane
    if lane == 63 or name == "plus1":
        assert int(slot.max()) == last + lane  # and it is the last slot in use
    rxn = int(hit[0])
    fp, _ = _check_probe(f"{name}-afac-lane{lane}", name, dm, afac_rxn=rxn, afac=1.7,
                         ref_cfg=dict(pert_rxn=rxn, pert_fac=1.7))
    f0, _ = _probe(dm, probe_arrays(), False)
    assert not np.array_equal(f0, fp)  # the perturbation reached the kernel
