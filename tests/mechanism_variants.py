"""Mechanisms of chosen size for the tests that walk the compiled size variants of the kernels
(test_size_variants_host.py, test_gpu_size_variants.py; DESIGN.md "Compiled size variants").

Four families, all cut from or appended to the repository's own GRI-Mech 3.0 files:

* tracer_mechanism: GRI-3.0 (or its PLOG stand-in) + n argon tracers AX1..AXn, KK = 53 + n
  (data/make_tracer_mechanism.py); `thin` drops the low-index tracers' extra reactions for an image that
  has to fit a kernel's LDS;
* gri_subset_text: the GRI reactions among a chosen tuple of species (KK < 53);
* extra_element_mechanism: GRI-3.0 + one inert species per extra element (MM = 6, 7, 8);
* ends_Y: the tracer workload with the first and the LAST tracer live, so that the species next to the
  padding of a size variant takes part.

The size lists and the reactor / equilibrium cases of the tests are kept here, so that the host test that
proves every input's precondition on the CPU and the GPU test that uses the input read one definition.
"""
import functools
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")
if DATA not in sys.path:
    sys.path.insert(0, DATA)

from make_tracer_mechanism import write_big_mechanism  # noqa: E402

CHEM = os.path.join(DATA, "grimech30_chem.inp")
THERM = os.path.join(DATA, "grimech30_thermo.dat")
PLOG_CHEM = os.path.join(DATA, "gri30_plog_chem.inp")
P_ATM = 1.01325e6
KK_GRI = 53


# ---------------------------------------------------------------------- generators
def gri_species():
    """GRI-Mech 3.0's species in file order."""
    lines = open(CHEM).read().split("\n")
    i0 = next(i for i, l in enumerate(lines) if l.strip().upper() == "SPECIES")
    i1 = next(i for i in range(i0, len(lines)) if lines[i].strip().upper() == "END")
    return tuple(" ".join(lines[i0 + 1:i1]).split())


def gri_subset_text(species, elements):
    """The subsystem of GRI-Mech 3.0 on `species`, cut from the repository's own file: reactions whose
    species all belong to the tuple, with their LOW / TROE / SRI / REV / DUP lines, and third-body
    efficiencies of other species dropped."""
    species = tuple(species)
    lines = open(CHEM).read().split("\n")
    i0 = next(i for i, l in enumerate(lines) if l.strip().upper().startswith("REACTIONS"))
    out = ["ELEMENTS", " ".join(elements), "END", "SPECIES"]
    out += [" ".join(species[i:i + 8]) for i in range(0, len(species), 8)]
    out += ["END", lines[i0]]
    keep = False
    for l in lines[i0 + 1:]:
        s = l.split("!")[0].strip()
        if not s or s.upper() == "END":
            continue
        if "=" in s:  # a reaction line
            eq = s.split()[0]
            sides = re.split(r"<=>|=>|=", eq.replace("(+M)", ""))
            sp = [re.sub(r"^\d+", "", x) for side in sides for x in side.split("+")]
            keep = all(x == "M" or x in species for x in sp)
            if keep:
                out.append(l)
        elif keep:
            if re.match(r"\s*(LOW|TROE|SRI|REV|DUP)", l, re.I):
                out.append(l)
            else:  # efficiencies: NAME/ value/ pairs
                pairs = re.findall(r"([^\s/]+)\s*/\s*([^/]+?)\s*/", l)
                eff = " ".join(f"{n}/{v}/" for n, v in pairs if n in species)
                if eff:
                    out.append(eff)
    out.append("END")
    return "\n".join(out) + "\n"


def _thin_tracer_reactions(text, thin):
    """Drop the coefficient-2, third-body and falloff reactions of the tracers AXk with k <= thin (the chain
    AXk + H <=> AXk+1 + H stays, and so does every reaction type at the high-index end)."""
    out, drop = [], False
    for l in text.split("\n"):
        m = re.match(r"^2?AX(\d+)(\+M|\(\+M\))?<=>", l)
        if m or "=" in l.split("!")[0]:
            drop = bool(m) and int(m.group(1)) <= thin
        elif l.strip().upper() == "END":
            drop = False
        if not drop:
            out.append(l)
    return "\n".join(out)


def write_tracer_mechanism(dirpath, n_tracer, plog=False, thin=0):
    """(chem_path, therm_path) of GRI-3.0 (plog: data/gri30_plog_chem.inp) + n_tracer tracers."""
    os.makedirs(dirpath, exist_ok=True)
    cp, tp = write_big_mechanism(str(dirpath), n_tracer=n_tracer, chem=PLOG_CHEM if plog else CHEM)
    if thin:
        text = open(cp).read()
        with open(cp, "w") as f:
            f.write(_thin_tracer_reactions(text, thin))
    return cp, tp


def extra_element_mechanism(dirpath, extra):
    """GRI-3.0 plus one inert species per element of `extra` (from HE, NE, KR): XHE, XNE, XKR, each with AR's
    NASA-7 block and its own element, the element added to ELEMENTS: MM = 5 + len(extra), KK = 53 + len(extra).
    Returns (chem_path, therm_path)."""
    extra = tuple(extra)
    assert extra and set(extra) <= {"HE", "NE", "KR"}, extra
    os.makedirs(dirpath, exist_ok=True)
    chem = open(CHEM).read().split("\n")
    out, section = [], None
    for l in chem:
        u = l.strip().upper()
        if u in ("ELEMENTS", "SPECIES"):
            section = u
        elif u == "END" and section:
            out.append("  ".join(extra) if section == "ELEMENTS" else "  ".join("X" + e for e in extra))
            section = None
        out.append(l)
    therm = open(THERM).read().split("\n")
    i_ar = next(i for i, t in enumerate(therm) if t.startswith("AR "))
    ar = therm[i_ar:i_ar + 4]
    assert ar[0][24:29] == "AR  1", ar[0]
    i_end = max(i for i, t in enumerate(therm) if t.strip().upper() == "END")
    block = []
    for e in extra:
        block += [("X" + e).ljust(18) + ar[0][18:24] + e.ljust(2) + ar[0][26:]] + ar[1:]
    therm = therm[:i_end] + block + therm[i_end:]
    tag = "".join(e.lower() for e in extra)
    cp, tp = os.path.join(str(dirpath), f"gri30_{tag}_chem.inp"), os.path.join(str(dirpath), f"gri30_{tag}_thermo.dat")
    with open(cp, "w") as f:
        f.write("\n".join(out))
    with open(tp, "w") as f:
        f.write("\n".join(therm))
    return cp, tp


# ---------------------------------------------------------------------- cached mechanisms
_TMP = None


def _tmp(name):
    global _TMP
    if _TMP is None:
        _TMP = tempfile.TemporaryDirectory(prefix="ckmi_variants_")
    d = os.path.join(_TMP.name, name)
    os.makedirs(d, exist_ok=True)
    return d


@functools.lru_cache(maxsize=None)
def tracer_mechanism(n_tracer, plog=False, thin=0):
    from pychemkin_amd.mechanism import Mechanism

    return Mechanism.from_files(*write_tracer_mechanism(_tmp(f"t{n_tracer}_{int(plog)}_{thin}"), n_tracer, plog, thin))


@functools.lru_cache(maxsize=None)
def subset_mechanism(species, elements):
    from pychemkin_amd.mechanism import Mechanism

    path = os.path.join(_tmp(f"s{len(species)}_{len(elements)}"), "subset_chem.inp")
    with open(path, "w") as f:
        f.write(gri_subset_text(species, elements))
    return Mechanism.from_files(path, THERM)


@functools.lru_cache(maxsize=None)
def element_mechanism(extra):
    from pychemkin_amd.mechanism import Mechanism

    return Mechanism.from_files(*extra_element_mechanism(_tmp("e" + "".join(extra)), extra))


# ---------------------------------------------------------------------- workloads
def last_tracers(mech):
    """The (at most two) highest-index tracers: the species next to the padding of a size variant."""
    n = mech.KK - KK_GRI
    assert mech.species[-1] == f"AX{n}"
    return tuple(f"AX{k}" for k in range(max(1, n - 1), n + 1))


def ends_Y(mech, phi, frac=0.2):
    """CH4/air at phi with `frac` of the N2 replaced by tracers, split between AX1 and the LAST tracer (the
    workload of test_gpu_bigreactor.tracer_Y with the highest-index species live)."""
    phi = np.atleast_1d(np.asarray(phi, dtype=np.float64))
    X = np.zeros((phi.size, mech.KK))
    X[:, mech.species.index("CH4")] = phi
    X[:, mech.species.index("O2")] = 2.0
    X[:, mech.species.index("N2")] = 7.52 * (1.0 - frac)
    X[:, mech.species.index("AX1")] += 7.52 * frac / 2
    X[:, mech.KK - 1] += 7.52 * frac / 2
    Y = X * mech.wt
    return Y / Y.sum(axis=1, keepdims=True)


# ---------------------------------------------------------------------- 3.1 workgroup reactor kernel
BIG_PLAIN_NVAR = (65, 80, 81, 96, 97, 112, 113, 128, 129, 144, 145, 160, 161, 176, 177, 192)
BIG_PLOG_NVAR = (65, 128, 129, 176, 177, 192)
BIG_CASES = [(nv, False) for nv in BIG_PLAIN_NVAR] + [(nv, True) for nv in BIG_PLOG_NVAR]
BIG_THIN = {}  # (nvar, plog) -> thin: sizes whose full tracer family does not fit the kernel's LDS (none)
BIG_RUN = dict(energy=1, t_end=0.02, atol=1e-10, rtol=1e-8, ign_mode="TIFP")  # RUN of test_gpu_bigreactor.py
BIG_MAJOR = ("CH4", "O2", "N2", "H2O", "CO2", "CO", "H2", "AX1")              # its MAJOR


def big_variant(nvar, plog):
    """(NB, PL) of big_reactor_kernel that ckmi_big.hip launch_big_reactors picks for nvar = KK + 1 > 64."""
    if plog:
        return (8 if nvar <= 128 else 11 if nvar <= 176 else 12), True
    return max(4, (nvar + 15) // 16), False


def big_matrix(nb):
    """ckmi_big_matrix.hpp BigMat<NB>: the MFMA Gauss-Jordan up to NB = 11, the per-column VALU one at 12."""
    return "BigMatrixM" if nb <= 11 else "BigMatrix"


def big_cases(n, seed):
    """_cases of test_gpu_bigreactor.py."""
    rng = np.random.default_rng(seed)
    T0 = rng.uniform(1250.0, 1700.0, n)
    P0 = P_ATM * rng.uniform(10.0, 60.0, n)
    phi = rng.uniform(0.5, 2.0, n)
    prob = np.where(np.arange(n) % 2 == 0, 1, 2).astype(np.int32)
    return T0, P0, phi, prob


@functools.lru_cache(maxsize=None)
def big_reference(nvar, plog):
    """The 4 reactors of one size (big_cases(4, 11), composition ends_Y) and the oracle's answers, computed once
    per session: dict(mech, T0, P0, Y0, prob, nfail, ref, Yref)."""
    from oracle.oracle import Oracle

    mech = tracer_mechanism(nvar - 1 - KK_GRI, plog, BIG_THIN.get((nvar, plog), 0))
    T0, P0, phi, prob = big_cases(4, 11)
    Y0 = ends_Y(mech, phi)
    nfail, ref, Yref = Oracle(mech).reactor_batch(T0, P0, Y0, problem=prob, V0=np.ones(4), **BIG_RUN)
    return dict(mech=mech, T0=T0, P0=P0, Y0=Y0, prob=prob, nfail=nfail, ref=list(ref), Yref=np.asarray(Yref))


# ---------------------------------------------------------------------- 3.2 wave kernel edges
SUBSET31 = gri_species()[:30] + ("N2",)
SUBSET32 = SUBSET31 + ("AR",)
WAVE_RUN = dict(energy=1, t_end=1.0, atol=1e-10, rtol=1e-8, ign_mode="TIFP")  # RUN of test_gpu_hotloop_paths.py
WAVE_MAJOR = ("CH4", "O2", "N2", "H2O", "CO2", "CO", "H2")
# name -> (nvar, reactor_kernel<N, PL, ...> the dispatch of ckmi.hip ckmi_reactor_run_ex picks, paths to force)
WAVE_CASES = {
    "subset31": (32, (32, False), (3,)),
    "subset32": (33, (54, False), (3,)),
    "plain_t1": (55, (64, False), (3, 2)),
    "plain_t10": (64, (64, False), (3, 2)),
    "plog_t1": (55, (64, True), (0, 2)),
    "plog_t10": (64, (64, True), (0, 2)),
}


def wave_mechanism(name):
    if name == "subset31":
        return subset_mechanism(SUBSET31, ("O", "H", "C", "N"))
    if name == "subset32":
        return subset_mechanism(SUBSET32, ("O", "H", "C", "N", "AR"))
    kind, n = name.split("_t")
    return tracer_mechanism(int(n), kind == "plog")


def wave_variant(nvar, plog):
    """N of the wave reactor_kernel<N, PL, ...> (ckmi.hip, the dispatch at the end of ckmi_reactor_run_ex)."""
    assert nvar <= 64
    return (64 if plog or nvar > 54 else 32 if nvar <= 32 else 54), plog


def wave_Y(mech, phi):
    """CH4/air; with tracers, ends_Y (first and last tracer live)."""
    from conftest import ch4_air_Y

    return ends_Y(mech, phi) if mech.KK > KK_GRI else ch4_air_Y(mech, phi)


@functools.lru_cache(maxsize=None)
def wave_reference(name):
    """4 reactors (the conditions of test_gpu_hotloop_paths.test_plog_mechanism_n64) and the oracle's answers."""
    from oracle.oracle import Oracle

    mech = wave_mechanism(name)
    cases = [(1200, 1, 1.0, 1), (1400, 10, 1.0, 2), (1600, 50, 1.5, 1), (1300, 30, 0.5, 2)]
    T0 = np.array([c[0] for c in cases], float)
    P0 = np.array([c[1] for c in cases], float) * P_ATM
    Y0 = np.stack([wave_Y(mech, c[2])[0] for c in cases])
    prob = np.array([c[3] for c in cases], np.int32)
    nfail, ref, Yref = Oracle(mech).reactor_batch(T0, P0, Y0, problem=prob, V0=np.ones(4), **WAVE_RUN)
    return dict(mech=mech, T0=T0, P0=P0, Y0=Y0, prob=prob, nfail=nfail, ref=list(ref), Yref=np.asarray(Yref))


# ---------------------------------------------------------------------- 3.3 rates and thermo
ROP_KK = (63, 64, 127, 128, 191, 192, 255)
ROP_N = (1, 65)
# KK = 255 is the last the image holds, but the rate kernels refuse the tracer family above these counts: image +
# ROP work space no longer fit the 160 KiB LDS of a CU (CKMI_ERR_SIZE; measured on an MI355X: plain 224 accepted,
# 225 refused; PLOG base 220 accepted, 221 refused).  They are the top sizes of test_rates_at_image_edges.
ROP_TOP = {False: 224, True: 220}
ROP_CASES = [(KK, plog) for plog in (False, True) for KK in ROP_KK[:-1] + (ROP_TOP[plog],)]


def rop_variant(KK):
    """NCH of rop_kernel<MODE, NCH, PL> (ckmi.hip launch_rop: KKp / 64, KKp = KK + 1 rounded up to 64)."""
    return (KK + 1 + 63) // 64


# ---------------------------------------------------------------------- 3.4 batched LU
LU_N = (2, 15, 31, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128, 129, 144, 145, 160, 176, 177, 191)


def lu_variant(n):
    """NB of lu_factor_kernel<NB> (ckmi_lu.hip, kFactor[(n + 15) / 16 - 1])."""
    return (n + 15) // 16


# ---------------------------------------------------------------------- 3.5 equilibrium
H2_SPECIES = ("H2", "H", "O", "O2", "OH", "H2O", "HO2", "H2O2", "N2", "AR")
HO_SPECIES = H2_SPECIES[:8]
EQ_MM = (1, 2, 3, 4, 6, 7, 8)
EQ_TP = ((1500.0, 1.0), (300.0, 20.0), (2800.0, 0.05))
# per MM: mixtures (mole numbers) for options 1-9; the first holds every element, the last lacks one (MM >= 2);
# `cj` marks the detonable ones, which option 10 takes at 300 K and 1500 K, 1 atm.
# No mixture is exactly stoichiometric: a cold state that burns out completely leaves its trace species (O2 at
# 1e-13, NH3 at 1e-16) to the rounding of the element balance b_O - b_H / 2 = 0, where the convergence rule
# (n_j |d ln n_j| / n <= 1e-12) does not hold them and the reference itself moves by O(1) in ln x_j when the
# input moves by an ulp (test_size_variants_host.py::test_equilibrium_inputs measures this).
EQ_MIXES = {
    1: [({"O2": 1.0}, False), ({"O": 0.3, "O2": 0.7}, False)],
    2: [({"H2": 2.4, "O2": 1.0}, True), ({"H2": 1.0, "O2": 2.0}, True), ({"H2": 1.0}, False)],
    3: [({"H2": 2.4, "O2": 1.0, "N2": 3.76}, True), ({"NH3": 4.0, "O2": 3.6}, True), ({"H2": 1.6, "O2": 1.0}, True)],
    4: [({"H2": 2.4, "O2": 1.0, "N2": 3.76, "AR": 0.5}, True), ({"H2": 1.6, "O2": 1.0, "AR": 7.0}, True),
        ({"H2": 1.6, "O2": 1.0, "N2": 3.76}, True)],
}
_CH4_AIR = {"CH4": 1.2, "O2": 2.0, "N2": 7.52, "AR": 0.1}
for _i, _extra in enumerate((("HE",), ("HE", "NE"), ("HE", "NE", "KR"))):
    _all = dict(_CH4_AIR, **{"X" + e: 0.2 + 0.1 * j for j, e in enumerate(_extra)})
    _some = {k: v for k, v in _all.items() if k != "X" + _extra[-1]}   # the newest element absent
    EQ_MIXES[6 + _i] = [(_all, True), ({"H2": 1.6, "O2": 1.0, **{"X" + e: 1.0 for e in _extra}}, True), (_some, True)]


def equil_mechanism(MM):
    if MM == 1:
        return subset_mechanism(("O", "O2"), ("O",))
    if MM == 2:
        return subset_mechanism(HO_SPECIES, ("O", "H"))
    if MM == 3:
        return subset_mechanism(HO_SPECIES + ("N2", "N", "NO", "NO2", "N2O", "NH3"), ("O", "H", "N"))
    if MM == 4:
        return subset_mechanism(H2_SPECIES, ("O", "H", "N", "AR"))
    return element_mechanism(("HE", "NE", "KR")[:MM - 5])


def equil_states(MM):
    """(option, T, P, Y) of every state of one mechanism, in launch order: options 1-9 on every (T, P) x mixture,
    then option 10 on the detonable mixtures at 300 K and 1500 K, 1 atm."""
    from equilibrium_reference import _Y_of

    mech = equil_mechanism(MM)
    opt, T, P, Y = [], [], [], []
    for o in range(1, 10):
        for t, p in EQ_TP:
            for mix, _ in EQ_MIXES[MM]:
                opt.append(o), T.append(t), P.append(p * P_ATM), Y.append(_Y_of(mech, mix))
    for t in (300.0, 1500.0):
        for mix, cj in EQ_MIXES[MM]:
            if cj:
                opt.append(10), T.append(t), P.append(P_ATM), Y.append(_Y_of(mech, mix))
    return np.array(opt, np.int32), np.array(T), np.array(P), np.stack(Y)


@functools.lru_cache(maxsize=None)
def equil_reference(MM):
    from equilibrium_reference import EquilibriumReference

    opt, T, P, Y = equil_states(MM)
    mech = equil_mechanism(MM)
    return dict(mech=mech, opt=opt, T=T, P=P, Y=Y, ref=EquilibriumReference(mech).solve(opt, T, P, Y))


# ---------------------------------------------------------------------- 3.2 PSR on the plain nvar = 64 mechanism
PSR_TIN, PSR_MDOT, PSR_TAU = 300.0, 1.0, 1e-3


@functools.lru_cache(maxsize=None)
def psr_reference():
    """One ignited PSR of GRI-3.0 + 10 tracers (test_gpu_psr.py's inlet, 300 K, 1 atm, tau = 1 ms, with the first
    and last tracer in the feed): the burnt estimate from the oracle and the reference's own root."""
    from oracle.oracle import Oracle
    from psr_reference import PSRReference

    mech = wave_mechanism("plain_t10")
    orc = Oracle(mech)
    Yin = ends_Y(mech, 1.0)[0]
    r, Yb = orc.reactor(1600.0, P_ATM, 1.0, Yin, problem=1, energy=1, t_end=1e-2, atol=1e-12, rtol=1e-8)
    root, its = PSRReference(orc, P_ATM, PSR_TIN, Yin, PSR_MDOT, tau=PSR_TAU).solve(r.T, Yb)
    return dict(mech=mech, oracle=orc, Yin=Yin, status=r.status, Tb=r.T, Yb=Yb, root=root)


# ---------------------------------------------------------------------- 3.3 states and the oracle's rates
def rop_states(KK, n, seed):
    """_states of test_gpu_bigmech.py."""
    rng = np.random.default_rng(seed)
    T = rng.uniform(300.0, 3000.0, n)
    P = P_ATM * 10.0 ** rng.uniform(-1.0, 2.0, n)
    Y = rng.dirichlet(0.5 * np.ones(KK), n).T.copy()
    return T, P, Y


@functools.lru_cache(maxsize=None)
def rop_reference(KK, plog, n):
    """n states (seed n) of GRI-3.0 / PLOG GRI + (KK - 53) tracers and the oracle's wdot, cp, h, qf, qr and
    species cp/R, h/RT."""
    from oracle.oracle import Oracle

    mech = tracer_mechanism(KK - KK_GRI, plog)
    orc = Oracle(mech)
    T, P, Y = rop_states(KK, n, seed=n)
    w, cp, h = orc.rop_batch(T, P, Y)
    q = [orc.rates(T[j], P[j], Y[:, j]) for j in range(n)]
    th = [orc.thermo(T[j]) for j in range(n)]
    return dict(mech=mech, T=T, P=P, Y=Y, w=w, cp=cp, h=h, qf=np.stack([x[0] for x in q], axis=1),
                qr=np.stack([x[1] for x in q], axis=1), cpk=np.stack([x[0] for x in th], axis=1),
                hk=np.stack([x[1] for x in th], axis=1))


# ---------------------------------------------------------------------- 3.4 matrices
def newton_like_parts(rng, nsys, n):
    """(J, gamma) of newton_like: a chemistry-like spread of magnitudes, gamma in 1e-9..1e-5."""
    J = rng.standard_normal((nsys, n, n)) * 10.0 ** rng.uniform(-3, 6, (nsys, n, n))
    gamma = 10.0 ** rng.uniform(-9, -5, (nsys, 1, 1))
    return J, gamma


def newton_like(rng, nsys, n):
    """_newton_like of test_gpu_lu.py: I - gamma J with a chemistry-like spread of magnitudes."""
    J, gamma = newton_like_parts(rng, nsys, n)
    return np.eye(n)[None] - gamma * J


def lu_matrices(n, nsys=5):
    """nsys matrices of order n: the first half Newton-like, the rest standard normal."""
    rng = np.random.default_rng(1000 + n)
    A = rng.standard_normal((nsys, n, n))
    A[: nsys // 2] = newton_like(rng, nsys // 2, n)
    return A


LU_SOLVE_COND = 1e3


def lu_solve_systems(n, nsys):
    """(A, b) of test_gpu_lu.py::test_lu_solve's kind.  A system whose condition number is above LU_SOLVE_COND is
    drawn again: at 1e6 (met among these draws) LAPACK's own solution is off by the bar of 1e-10, and the
    comparison would judge the reference, not the kernel (test_size_variants_host.py measures LAPACK's error
    on every system kept)."""
    rng = np.random.default_rng(7 + 1000 * nsys + n)
    A = newton_like(rng, nsys, n)
    for s in range(nsys):
        while np.linalg.cond(A[s]) > LU_SOLVE_COND:
            A[s] = newton_like(rng, 1, n)[0]
    return A, rng.standard_normal((nsys, n))


def refined_solution(A, b):
    """x of A x = b with the residual accumulated in extended precision (two refinement steps)."""
    x = np.linalg.solve(A, b)
    for _ in range(2):
        r = (b.astype(np.longdouble) - A.astype(np.longdouble) @ x.astype(np.longdouble)).astype(np.float64)
        x = (x.astype(np.longdouble) + np.linalg.solve(A, r).astype(np.longdouble))
        x = x.astype(np.float64)
    return x


def tie_matrix(n, seed=0):
    """A matrix whose first column is all +-1 (every row ties for the first pivot; dgetrf takes row 0)."""
    rng = np.random.default_rng(seed + n)
    A = rng.standard_normal((n, n))
    A[:, 0] = np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
    return A


def equil_input_sensitivity(MM, stoichiometric=False):
    """Largest move of the reference's own answer (the measure of test_gpu_equilibrium.disagreement, options 1-9)
    when every mass fraction of the input moves by two ulps at random: what an equally good solver may differ
    by.  stoichiometric=True measures the same on H2 : O2 = 2 : 1 in place of the first mixture (MM >= 2)."""
    from equilibrium_reference import EquilibriumReference, _Y_of

    mech = equil_mechanism(MM)
    opt, T, P, Y = equil_states(MM)
    if stoichiometric:
        Y = np.where(np.all(Y == Y[0], axis=1)[:, None], _Y_of(mech, {"H2": 2.0, "O2": 1.0}), Y)
    rng = np.random.default_rng(MM)
    Yp = Y * (1.0 + 2.0 ** -51 * rng.choice([-1.0, 1.0], Y.shape))
    eq = EquilibriumReference(mech)
    a, b = eq.solve(opt, T, P, Y), eq.solve(opt, T, P, Yp)
    m9 = (opt < 10) & (a["status"] == 0) & (b["status"] == 0)
    keep = (a["X"] >= 1e-20) & (b["X"] >= 1e-20)
    with np.errstate(divide="ignore", invalid="ignore"):
        dx = np.where(keep, np.abs(np.log(np.where(keep, a["X"], 1.0)) - np.log(np.where(keep, b["X"], 1.0))), 0.0)
    d = np.maximum.reduce([np.abs(a["T"] / b["T"] - 1), np.abs(a["P"] / b["P"] - 1), dx.max(axis=1)])
    return float(d[m9].max())
