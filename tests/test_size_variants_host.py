"""Preconditions of test_gpu_size_variants.py, proved on the CPU: every mechanism has the size it is meant to
have, every size maps to the compiled variant it is meant to reach, and the reference alone passes on every
input -- so that a failure on the GPU cannot be an artefact of the inputs, and no GPU test filters a case.
"""
import filecmp
import inspect

import numpy as np
import pytest

import mechanism_variants as mv
from conftest import BIG_CHEM, BIG_THERM


def test_default_generator_output_is_byte_identical(tmp_path):
    """write_big_mechanism with its defaults writes the two committed data/gri30_tracer161_* files."""
    cp, tp = mv.write_big_mechanism(str(tmp_path))
    assert filecmp.cmp(cp, BIG_CHEM, shallow=False)
    assert filecmp.cmp(tp, BIG_THERM, shallow=False)


def test_h2_subset_is_unchanged():
    """gri_subset_text on the H2 tuple keeps the 10 species and 29 reactions test_gpu_hotloop_paths.py ran."""
    m = mv.equil_mechanism(4)
    assert tuple(m.species) == mv.H2_SPECIES and m.II == 29


# ---------------------------------------------------------------------- 3.1
# nvar = KK + 1 -> NB of big_reactor_kernel<NB, PL> (ckmi_big.hip launch_big_reactors: plain
# `switch ((nvar + 15) / 16)`, extended `nvar <= 128 -> 8, <= 176 -> 11, else 12`) and the Newton matrix
# (ckmi_big_matrix.hpp BigMat<NB>: BigMatrixM up to NB = 11, BigMatrix at 12)
BIG_TABLE = {
    (65, False): 5, (80, False): 5, (81, False): 6, (96, False): 6, (97, False): 7, (112, False): 7,
    (113, False): 8, (128, False): 8, (129, False): 9, (144, False): 9, (145, False): 10, (160, False): 10,
    (161, False): 11, (176, False): 11, (177, False): 12, (192, False): 12,
    (65, True): 8, (128, True): 8, (129, True): 11, (176, True): 11, (177, True): 12, (192, True): 12,
}


def test_big_sizes_reach_every_variant_at_both_edges():
    assert set(mv.BIG_CASES) == set(BIG_TABLE) and len(mv.BIG_CASES) == 22
    for (nvar, plog), nb in BIG_TABLE.items():
        assert mv.big_variant(nvar, plog) == (nb, plog)
        assert mv.big_matrix(nb) == ("BigMatrix" if nb == 12 else "BigMatrixM")
    for nb in range(5, 13):       # plain: most padded and exactly full
        assert BIG_TABLE[(16 * (nb - 1) + 1, False)] == BIG_TABLE[(16 * nb, False)] == nb
    for lo, hi, nb in ((65, 128, 8), (129, 176, 11), (177, 192, 12)):   # extended: the smallest and largest size
        assert BIG_TABLE[(lo, True)] == BIG_TABLE[(hi, True)] == nb


@pytest.mark.parametrize("nvar,plog", mv.BIG_CASES)
def test_big_reactor_inputs(nvar, plog):
    """The oracle integrates all four reactors of the size; the last two tracers (beside the padding) end at
    Yref >= 1e-3, so the species bar 1e-4 max(|Yref|, 1e-3) is a relative bound on them, and have moved."""
    r = mv.big_reference(nvar, plog)
    mech = r["mech"]
    assert mech.KK == nvar - 1 and mech.species[-1] == f"AX{nvar - 54}"
    assert bool(mech.to_tables()["plog_ptr"][-1] > 0) == plog
    assert r["nfail"] == 0
    assert all(x.status == 0 and x.tau > 0 for x in r["ref"])
    last = mv.last_tracers(mech)
    assert len(last) == 2
    for sp in last:
        k = mech.species.index(sp)
        assert np.all(r["Yref"][:, k] >= 1e-3), (sp, r["Yref"][:, k])
        assert np.all(np.abs(r["Yref"][:, k] - r["Y0"][:, k]) >= 1e-3), sp
    assert np.all(r["Y0"][:, mech.KK - 1] > 0.05) and np.all(r["Y0"][:, mech.species.index("AX1")] > 0.05)


def test_thinning_keeps_the_chain_and_the_high_end():
    """The option for an image that does not fit: the low tracers lose their extra reactions, nothing else."""
    full, thin = mv.tracer_mechanism(138), mv.tracer_mechanism(138, False, 100)
    assert thin.KK == full.KK == 191 and thin.species == full.species
    assert 325 + 137 < thin.II < full.II
    assert mv.BIG_THIN == {}   # no size needs it today: every image of the family fits the kernel's LDS


# ---------------------------------------------------------------------- 3.2
# name -> (nvar, (N, PL) of reactor_kernel<N, PL, F64, PSR>; ckmi.hip, the dispatch that ends
# ckmi_reactor_run_ex: PLOG -> 64; nvar <= 32 -> 32 (FP32 inverse only); <= 54 -> 54; else 64.  ckmi_psr.hip's
# dispatch takes the same N with PSR = true)
WAVE_TABLE = {"subset31": (32, (32, False)), "subset32": (33, (54, False)), "plain_t1": (55, (64, False)),
              "plain_t10": (64, (64, False)), "plog_t1": (55, (64, True)), "plog_t10": (64, (64, True))}


# ---------------------------------------------------------------------- the chooser itself
# ckmi_reactor_variant (include/ckmi.h) reads wave_plan / big_plan of csrc/ckmi_dispatch.hpp, the functions
# every launcher calls.  out: [1 wave | 2 workgroup, N of the FP32-inverse launch or 0 | NB, N of the FP64-inverse
# launch, PL, 0 all | 1 plug flow and engines | 2 those and the FP32 failures]
CKMI_OK, CKMI_ERR_UNSUPPORTED = 0, 4   # include/ckmi.h
# the PSR rows (nvar, plog) -> reactor_kernel<N, PL, true, true>
PSR_TABLE = {(64, False): (64, False), (54, False): (54, False), (54, True): (64, True)}


def _variant(nvar, plog, general, rtol, path, psr):
    import ctypes as ct

    from pychemkin_amd import _native

    out = (ct.c_int32 * 5)(*[-1] * 5)
    rc = _native.lib().ckmi_reactor_variant(nvar, int(plog), int(general), rtol, path, int(psr), out)
    return rc, tuple(out)


def test_chooser_agrees_with_the_restatement_and_the_rules():
    """Every input of the chooser: the kernel family, N / NB and PL against mechanism_variants (written before the
    chooser existed and not edited for it), the FP64 rule, the FP64 launch's N and the retry flag against the rules
    as ckmi_dispatch.hpp states them, written out here."""
    ncase = 0
    for nvar in range(2, 194):
        for plog in (False, True):
            for general in (False, True):
                for rtol in (1e-6, 1e-9, 1e-10):
                    for path in range(4):
                        for psr in (False, True):
                            rc, out = _variant(nvar, plog, general, rtol, path, psr)
                            what = (nvar, plog, general, rtol, path, psr)
                            ncase += 1
                            if nvar > (64 if psr else 192):
                                assert rc == CKMI_ERR_UNSUPPORTED, what
                                continue
                            assert rc == CKMI_OK, what
                            if not psr and (nvar > 64 or path == 1):
                                nb, pl = mv.big_variant(nvar, plog)
                                assert out == (2, nb, 0, int(pl), 0), what
                                continue
                            n, pl = mv.wave_variant(nvar, plog)
                            # FP64 inverse alone: forced (2), or not forced off (3) and tight or general orders;
                            # an open reactor always
                            f64 = psr or path == 2 or (path != 3 and (rtol < 1e-9 or general))
                            n64 = 64 if (plog or nvar > 54) else 54      # no 32-wide FP64-inverse variant
                            if f64:
                                assert out == (1, 0, n64, int(pl), 0), what
                            else:
                                retry = path == 0 and n64 == 64          # automatic path, 64-wide variants only
                                assert out == (1, n, n64, int(pl), 2 if retry else 1), what
    assert ncase == 192 * 2 * 2 * 3 * 4 * 2


def test_chooser_gives_the_tables_variants():
    """WAVE_CASES on the paths they force, BIG_CASES and the PSR rows of DESIGN.md section 10 get the variant the
    table names."""
    for name, (nvar, (n, pl), paths) in mv.WAVE_CASES.items():
        for path in paths:
            rc, out = _variant(nvar, pl, False, mv.WAVE_RUN["rtol"], path, False)
            assert rc == CKMI_OK and out[0] == 1 and out[3] == int(pl), (name, path)
            if path == 2:
                assert out[1:3] == (0, n), (name, path)           # one launch, FP64 inverse
            else:
                assert out[1] == n and out[4] == (2 if path == 0 else 1), (name, path)
    for (nvar, plog), nb in BIG_TABLE.items():
        for path in (0, 1):
            assert _variant(nvar, plog, False, mv.BIG_RUN["rtol"], path, False) == (CKMI_OK, (2, nb, 0, int(plog), 0))
    assert _variant(54, False, False, 1e-8, 1, False) == (CKMI_OK, (2, 4, 0, 0, 0))   # GRI-3.0 forced: <4, false>
    for (nvar, plog), (n, pl) in PSR_TABLE.items():
        for path in range(4):
            assert _variant(nvar, plog, False, 1e-6, path, True) == (CKMI_OK, (1, 0, n, int(pl), 0))


@pytest.mark.parametrize("name", list(mv.WAVE_CASES))
def test_wave_reactor_inputs(name):
    nvar, variant, _ = mv.WAVE_CASES[name]
    assert (nvar, variant) == WAVE_TABLE[name]
    r = mv.wave_reference(name)
    mech = r["mech"]
    assert mech.KK + 1 == nvar and mv.wave_variant(nvar, variant[1]) == variant
    assert bool(mech.to_tables()["plog_ptr"][-1] > 0) == variant[1]
    assert mech.II >= 184   # the subsets keep their reactions (31 species: 184, 32: 186)
    assert r["nfail"] == 0 and all(x.status == 0 and x.tau > 0 for x in r["ref"])
    if mech.KK > mv.KK_GRI:   # the last tracer is live; with more than one tracer (exchange reactions) it moves
        k = mech.KK - 1
        assert np.all(r["Yref"][:, k] >= 1e-3)
        assert mech.KK == mv.KK_GRI + 1 or np.all(np.abs(r["Yref"][:, k] - r["Y0"][:, k]) >= 1e-3)


def test_subset_sizes():
    m31, m32 = mv.wave_mechanism("subset31"), mv.wave_mechanism("subset32")
    assert (m31.KK, m31.II, m32.KK, m32.II) == (31, 184, 32, 186)


# ---------------------------------------------------------------------- 3.3
# KK -> NCH of rop_kernel<MODE, NCH, PL> (ckmi.hip launch_rop: `switch (KKp / 64)`, KKp = KK + 1 rounded up to
# a multiple of 64, ckmi_mech_create); KK = 256 is past KK_IMAGE_MAX = 255 (ckmi_image.hpp)
ROP_TABLE = {63: 1, 64: 2, 127: 2, 128: 3, 191: 3, 192: 4, 220: 4, 221: 4, 224: 4, 225: 4, 255: 4}


@pytest.mark.parametrize("plog", [False, True])
def test_rop_sizes(plog):
    """Every NCH at both edges of its species range; NCH = 4 up to the largest tracer count the rate kernels'
    LDS takes (mechanism_variants.ROP_TOP), the refusal above it pinned on the GPU."""
    assert mv.ROP_KK == (63, 64, 127, 128, 191, 192, 255) and mv.ROP_TOP == {False: 224, True: 220}
    sizes = [KK for KK, pl in mv.ROP_CASES if pl == plog]
    assert sizes == [63, 64, 127, 128, 191, 192, mv.ROP_TOP[plog]]
    for KK in sizes + [mv.ROP_TOP[plog] + 1, 255]:
        assert mv.rop_variant(KK) == ROP_TABLE[KK]
        mech = mv.tracer_mechanism(KK - mv.KK_GRI, plog)
        assert mech.KK == KK and bool(mech.to_tables()["plog_ptr"][-1] > 0) == plog
    assert [ROP_TABLE[k] for k in sizes] == [1, 2, 2, 3, 3, 4, 4]
    assert mv.tracer_mechanism(256 - mv.KK_GRI, plog).KK == 256   # parses; the device has to refuse it


# ---------------------------------------------------------------------- 3.4
# n -> NB of lu_factor_kernel<NB> (ckmi_lu.hip: kFactor[(n + 15) / 16 - 1])
EXISTING_LU_N = (1, 5, 16, 17, 54, 100, 161, 192)   # test_gpu_lu.py::test_lu_matches_lapack


def test_lu_sizes_reach_every_variant_at_both_edges():
    """With the sizes test_gpu_lu.py already runs, every NB = 1..12 is factored most padded (16 (NB - 1) + 1)
    and exactly full (16 NB)."""
    assert len(mv.LU_N) == 23 and max(mv.LU_N) <= 192
    ran = set(mv.LU_N) | set(EXISTING_LU_N)
    for nb in range(1, 13):
        lo, hi = 16 * (nb - 1) + 1, 16 * nb
        assert lo in ran and hi in ran, nb
        assert mv.lu_variant(lo) == mv.lu_variant(hi) == nb
    assert {mv.lu_variant(n) for n in mv.LU_N} == set(range(1, 13))


# ---------------------------------------------------------------------- 3.5
# elements that occur -> MM of equil_kernel<MM> (ckmi_equil.hip ckmi_equil_run: `switch (m->eq_mm)`)
@pytest.mark.parametrize("MM", mv.EQ_MM)
def test_equilibrium_inputs(MM):
    """EquilibriumReference.solve reports status 0 on every state the GPU test launches: options 1-9 on three
    (T, P) x every mixture, option 10 on the detonable mixtures only (the reference itself fails option 10 on
    pure O2, pure H2 and at 2800 K / 0.05 atm)."""
    r = mv.equil_reference(MM)
    mech = r["mech"]
    ncf = np.asarray(mech.ncf)
    assert int(np.any(ncf > 0, axis=1).sum()) == MM == ncf.shape[0]
    assert np.all(r["ref"]["status"] == 0)
    opt = r["opt"]
    nmix = len(mv.EQ_MIXES[MM])
    assert 2 <= nmix <= 3 and np.sum(opt < 10) == 9 * 3 * nmix
    assert all(np.sum(opt == o) == 3 * nmix for o in range(1, 10))
    # option 10: the detonable mixtures at two temperatures; nothing detonates among {O, O2}
    assert np.sum(opt == 10) == (0 if MM == 1 else 2 * sum(cj for _, cj in mv.EQ_MIXES[MM]))
    assert MM == 1 or np.sum(opt == 10) >= 4
    b = (r["Y"] / mech.wt) @ ncf.T
    assert np.any(np.all(b > 0, axis=1))                    # a mixture with every element
    if MM >= 2:
        assert np.any(np.any(b == 0, axis=1))               # and one from which an element is absent
    D = r["ref"]["detspeed"][opt == 10]
    assert np.all(D > 1e5)
    # the states are well posed: two ulps on the input move the reference's own answer by less than a fifth of the
    # bound the kernel is held to.  An exactly stoichiometric cold mixture is not (its trace species hang on the
    # rounding of the element balance; the first GPU run of this file differed from the reference by 0.9 - 3 in
    # ln x of O2 at 1e-13 and NH3 at 1e-16 there, and nowhere else), which is why no mixture is stoichiometric.
    from test_gpu_equilibrium import BOUND

    sens = mv.equil_input_sensitivity(MM)
    print(f"MM {MM}: the reference moves by {sens:.2e} under two ulps of input noise")
    assert sens <= BOUND / 5
    if MM >= 2:
        assert mv.equil_input_sensitivity(MM, stoichiometric=True) > 10 * BOUND


def test_psr_input():
    """The burnt estimate exists and the reference's own PSR root from it is ignited, with both tracers live."""
    p = mv.psr_reference()
    assert p["status"] == 0 and p["mech"].KK + 1 == 64 and p["Tb"] > 2000.0
    assert p["root"][0] > 1700.0 and p["root"][-1] > 1e-3 and p["Yin"][-1] > 0.04


@pytest.mark.parametrize("plog", [False, True])
def test_rate_inputs(plog):
    """The oracle's rates are finite at every state, each state has a non-zero largest |wdot| and q to scale by,
    and the last species reacts in some state."""
    for KK in [k for k, pl in mv.ROP_CASES if pl == plog] + [255]:
        for n in mv.ROP_N:
            o = mv.rop_reference(KK, plog, n)
            assert all(np.isfinite(o[k]).all() for k in ("w", "cp", "h", "qf", "qr", "cpk", "hk"))
            assert np.all(np.max(np.abs(o["w"]), axis=0) > 0) and np.all(np.max(np.abs(o["qf"]), axis=0) > 0)
        assert np.max(np.abs(mv.rop_reference(KK, plog, 65)["w"][-1])) > 0


def test_lu_solve_inputs_do_not_judge_lapack():
    """numpy.linalg.solve is itself within a tenth of test_lu_solve's bar (rtol 1e-10, atol 1e-12 max |x|) of
    the extended-precision solution on every system the GPU test solves; every matrix is non-singular."""
    worst = 0.0
    for n in mv.LU_N:
        for nsys in (1, 5, 67):
            A, b = mv.lu_solve_systems(n, nsys)
            assert np.linalg.cond(A).max() <= mv.LU_SOLVE_COND
            for s in range(nsys):
                x, xr = np.linalg.solve(A[s], b[s]), mv.refined_solution(A[s], b[s])
                worst = max(worst, np.max(np.abs(x - xr) / (1e-10 * np.abs(xr) + 1e-12 * np.abs(xr).max())))
    print("LAPACK's own error / bar:", worst)
    assert worst <= 0.1


def test_lu_tie_matrix():
    import scipy.linalg as sla

    for n in mv.LU_N:
        A = mv.tie_matrix(n)
        assert set(np.abs(A[:, 0])) == {1.0} and sla.lu_factor(A)[1][0] == 0


def test_no_gpu_case_is_skipped_or_filtered():
    """The cap: inputs are chosen so that the reference passes on all of them, so the GPU tests hold no skip,
    expected failure or filter of their own."""
    import test_gpu_size_variants as g

    src = inspect.getsource(g)
    for word in ("pytest.skip(", "xfail", "importorskip"):
        assert word not in src, word
    assert src.count("skipif(") == 1   # the module's one mark: no GPU in the machine
