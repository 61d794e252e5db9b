"""ctypes loader for the CPU ORACLE (test infrastructure only).

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may
import this module.  It builds ``oracle/_build/libckoracle.so`` from ``ckoracle.c`` with
gcc on first use and exposes numpy-friendly wrappers of the C restatement.

Mechanism tables come from ``pychemkin_amd.mechanism.Mechanism.to_tables()`` (the parsed
mechanism is data, not the computation under test).
"""
from __future__ import annotations

import ctypes as ct
import os
import subprocess
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "_build", "libckoracle.so")
_lib = None


def build(force: bool = False) -> str:
    src = os.path.join(_HERE, "ckoracle.c")
    if force or not os.path.exists(_LIB) or os.path.getmtime(_LIB) < os.path.getmtime(src):
        subprocess.run(["make", "-s", "-C", _HERE], check=True)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ct.CDLL(_LIB)
    return _lib


_P = ct.c_void_p


def lu_factor_batch(A: np.ndarray, nthreads: int = 0):
    """Batched partial-pivoting LU of (nsys, n, n) row-major matrices (ckoracle.c cko_lu_factor_batch: the
    integrator's own dense LU): returns (LU, piv, info), info[s] = 1 + the first zero pivot column or 0."""
    L = lib()
    L.cko_lu_factor_batch.argtypes = [ct.c_int, ct.c_int, _P, _P, _P, ct.c_int]
    A = np.array(A, dtype=np.float64, order="C", copy=True)
    nsys, n = A.shape[0], A.shape[1]
    piv = np.zeros((nsys, n), dtype=np.int32)
    info = np.zeros(nsys, dtype=np.int32)
    L.cko_lu_factor_batch(n, nsys, A.ctypes.data, piv.ctypes.data, info.ctypes.data, int(nthreads))
    return A, piv, info


class _Mech(ct.Structure):
    _fields_ = [("KK", ct.c_int), ("II", ct.c_int)] + [
        (n, _P) for n in ("wt", "thermo", "rtype", "rev", "nr", "np", "rsp", "psp", "rnu", "pnu", "arr", "low",
                          "revp", "has_rev", "ftype", "fpar", "tbsp", "eff_ptr", "eff_sp", "eff_val",
                          "plog_ptr", "plog_par", "ford", "rord")
    ] + [("MM", ct.c_int), ("ncf", _P)]


class _Cfg(ct.Structure):
    _fields_ = [
        ("problem", ct.c_int), ("energy", ct.c_int), ("t_end", ct.c_double), ("atol", ct.c_double),
        ("rtol", ct.c_double), ("h0", ct.c_double), ("hmax", ct.c_double), ("nneg", ct.c_int),
        ("ign_mode", ct.c_int), ("ign_val", ct.c_double), ("ign_species", ct.c_int), ("ign_stop", ct.c_int),
        ("max_steps", ct.c_int), ("nprof", ct.c_int), ("prof_t", _P), ("prof_v", _P), ("prof_kind", ct.c_int),
        ("gfac", ct.c_double), ("qloss", ct.c_double), ("htc", ct.c_double), ("areaq", ct.c_double),
        ("tamb", ct.c_double), ("pert_rxn", ct.c_int), ("pert_fac", ct.c_double), ("nprof2", ct.c_int),
        ("prof2_kind", ct.c_int), ("prof2_t", _P), ("prof2_v", _P), ("nprof3", ct.c_int), ("prof3_t", _P),
        ("prof3_v", _P), ("eng", _P), ("tran", _P), ("no_elem_proj", ct.c_int),
    ]


class Result(ct.Structure):
    _fields_ = [
        ("tau", ct.c_double), ("t_end", ct.c_double), ("T", ct.c_double), ("P", ct.c_double), ("V", ct.c_double),
        ("status", ct.c_int), ("nst", ct.c_int), ("nfe", ct.c_int), ("nje", ct.c_int), ("nlu", ct.c_int),
        ("ncf", ct.c_int), ("nef", ct.c_int),
    ]


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


IGN_MODES = {None: 0, "none": 0, "T_inflection": 1, "TIFP": 1, "T_rise": 2, "DTIGN": 2, "T_ignition": 3,
             "TLIM": 3, "Species_peak": 4, "KLIM": 4}


class Oracle:
    """CPU restatement bound to one mechanism."""

    def __init__(self, mech):
        self.mech = mech
        t = mech.to_tables()
        self._keep = {}
        for k, v in t.items():
            if isinstance(v, np.ndarray) and v.ndim > 0:
                self._keep[k] = np.ascontiguousarray(v)
        self.KK = int(t["KK"])
        self.II = int(t["II"])
        self.wt = t["wt"]
        s = _Mech()
        s.KK, s.II = self.KK, self.II
        for name, _ in _Mech._fields_[2:-2]:
            setattr(s, name, _ptr(self._keep[name]))
        # element counts: the corrector's element projection (ckoracle.c elem_project)
        ncf = getattr(mech, "ncf", None)
        if ncf is not None:
            self._keep["ncf"] = np.ascontiguousarray(ncf, np.int32)
            s.MM, s.ncf = int(self._keep["ncf"].shape[0]), _ptr(self._keep["ncf"])
        self._mech = s
        L = lib()
        L.cko_thermo.argtypes = [ct.POINTER(_Mech), ct.c_double, _P, _P, _P]
        L.cko_rates.argtypes = [ct.POINTER(_Mech), ct.c_double, ct.c_double, _P, _P, _P, _P]
        L.cko_rop_batch.argtypes = [ct.POINTER(_Mech), ct.c_int, _P, _P, _P, _P, _P, _P, ct.c_int]
        L.cko_reactor.argtypes = [ct.POINTER(_Mech), ct.POINTER(_Cfg), ct.c_double, ct.c_double, ct.c_double, _P, _P,
                                  ct.POINTER(Result), ct.c_int, _P, _P, _P, _P]
        L.cko_reactor_batch.argtypes = [ct.POINTER(_Mech), ct.POINTER(_Cfg), ct.c_int, _P, _P, _P, _P, _P, _P,
                                        ct.POINTER(Result), ct.c_int]
        L.cko_reactor_batch_pert.argtypes = [ct.POINTER(_Mech), ct.POINTER(_Cfg), ct.c_int, _P, _P, _P, _P, _P, _P,
                                             _P, _P, ct.POINTER(Result), ct.c_int]
        L.cko_rhs_jac.argtypes = [ct.POINTER(_Mech), ct.POINTER(_Cfg), ct.c_double, _P, ct.c_double, ct.c_double,
                                  ct.c_double, _P, _P]
        L.cko_rhs_jac_engine.argtypes = [ct.POINTER(_Mech), ct.POINTER(_Cfg), ct.c_double, _P, ct.c_double, ct.c_double,
                                         _P, _P, _P]
        self.L = L

    # ---------------------------------------------------------------- thermo / rop
    def thermo(self, T: float):
        cp, h, s = (np.zeros(self.KK) for _ in range(3))
        self.L.cko_thermo(ct.byref(self._mech), T, _ptr(cp), _ptr(h), _ptr(s))
        return cp, h, s

    def rates(self, T: float, P: float, Y: Sequence[float]):
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        qf, qr, w = np.zeros(self.II), np.zeros(self.II), np.zeros(self.KK)
        self.L.cko_rates(ct.byref(self._mech), T, P, _ptr(Y), _ptr(qf), _ptr(qr), _ptr(w))
        return qf, qr, w

    def rop_batch(self, T: np.ndarray, P: np.ndarray, Y_soa: np.ndarray, nthreads: int = 0):
        n = T.shape[0]
        T = np.ascontiguousarray(T, np.float64)
        P = np.ascontiguousarray(P, np.float64)
        Y_soa = np.ascontiguousarray(Y_soa, np.float64)
        w = np.zeros((self.KK, n))
        cp = np.zeros(n)
        h = np.zeros(n)
        self.L.cko_rop_batch(ct.byref(self._mech), n, _ptr(T), _ptr(P), _ptr(Y_soa), _ptr(w), _ptr(cp), _ptr(h),
                             nthreads)
        return w, cp, h

    # ---------------------------------------------------------------- reactors
    @staticmethod
    def make_cfg(problem=1, energy=1, t_end=1.0, atol=1e-12, rtol=1e-6, h0=0.0, hmax=0.0, nneg=False,
                 ign_mode=None, ign_val=0.0, ign_species=0, ign_stop=False, max_steps=0, profile=None,
                 prof_kind=0, gfac=1.0, qloss=0.0, htc=0.0, areaq=0.0, tamb=300.0, asteps=0, pert_rxn=-1,
                 pert_fac=1.0, profile2=None, prof2_kind=0, avar=-1, avalue=0.0, profile3=None, engine=None,
                 tran=None, elem_proj=True):
        """asteps / avar / avalue (adaptive output points) do not change the integration and are
        accepted for signature parity with pychemkin_amd._native.make_cfg.  elem_proj=False turns the
        element projection of the corrector off (A/B and drift diagnostics)."""
        c = _Cfg()
        c.no_elem_proj = 0 if elem_proj else 1
        c.prof_kind, c.gfac, c.qloss, c.htc, c.areaq, c.tamb = int(prof_kind), gfac, qloss, htc, areaq, tamb
        c.pert_rxn, c.pert_fac = int(pert_rxn), float(pert_fac)
        c.problem, c.energy, c.t_end, c.atol, c.rtol = problem, energy, t_end, atol, rtol
        c.h0, c.hmax, c.nneg = h0, hmax, int(bool(nneg))
        c.ign_mode = IGN_MODES[ign_mode] if not isinstance(ign_mode, int) else ign_mode
        c.ign_val, c.ign_species, c.ign_stop, c.max_steps = ign_val, ign_species, int(bool(ign_stop)), max_steps
        keep = None
        c.nprof2, c.prof2_kind = 0, int(prof2_kind)
        if profile2 is not None:
            x2 = np.ascontiguousarray(profile2[0], np.float64)
            v2 = np.ascontiguousarray(profile2[1], np.float64)
            c.nprof2, c.prof2_t, c.prof2_v = len(x2), _ptr(x2), _ptr(v2)
            keep = [(x2, v2)]
        c.nprof3 = 0
        if profile3 is not None:  # AEXT beside a QPRO profile2
            x3 = np.ascontiguousarray(profile3[0], np.float64)
            v3 = np.ascontiguousarray(profile3[1], np.float64)
            c.nprof3, c.prof3_t, c.prof3_v = len(x3), _ptr(x3), _ptr(v3)
            keep = (keep or []) + [(x3, v3)]
        if profile is not None:
            x = np.ascontiguousarray(profile[0], np.float64)
            v = np.ascontiguousarray(profile[1], np.float64)
            c.nprof, c.prof_t, c.prof_v = len(x), _ptr(x), _ptr(v)
            keep = (keep or []) + [(x, v)]
        else:
            c.nprof = 0
        if engine is not None:  # problem 4: the CKO_ENG_* parameter block (ckoracle.h)
            e = np.zeros(20)
            e[:len(engine)] = np.asarray(engine, np.float64)
            c.eng = _ptr(e)
            keep = (keep or []) + [e]
        if tran is not None:  # [KK][8] viscosity / conductivity fits (engine heat transfer)
            tf = np.ascontiguousarray(tran, np.float64)
            c.tran = _ptr(tf)
            keep = (keep or []) + [tf]
        return c, keep

    def reactor(self, T0, P0, V0, Y0, t_save: Optional[np.ndarray] = None, **cfg):
        c, keep = self.make_cfg(**cfg)
        Y0 = np.ascontiguousarray(Y0, np.float64)
        Yend = np.zeros(self.KK)
        res = Result()
        if t_save is not None:
            ts = np.ascontiguousarray(t_save, np.float64)
            ys = np.zeros((len(ts), self.KK + 1))
            ps = np.zeros(len(ts))
            vs = np.zeros(len(ts))
            self.L.cko_reactor(ct.byref(self._mech), ct.byref(c), T0, P0, V0, _ptr(Y0), _ptr(Yend), ct.byref(res),
                               len(ts), _ptr(ts), _ptr(ys), _ptr(ps), _ptr(vs))
            return res, Yend, (ts, ys, ps, vs)
        self.L.cko_reactor(ct.byref(self._mech), ct.byref(c), T0, P0, V0, _ptr(Y0), _ptr(Yend), ct.byref(res), 0,
                           None, None, None, None)
        del keep
        return res, Yend

    def reactor_batch(self, T0, P0, Y0, problem=None, V0=None, nthreads: int = 0, **cfg):
        c, keep = self.make_cfg(**cfg)
        n = len(T0)
        T0 = np.ascontiguousarray(T0, np.float64)
        P0 = np.ascontiguousarray(P0, np.float64)
        Y0 = np.ascontiguousarray(Y0, np.float64).reshape(n, self.KK)
        prob = np.ascontiguousarray(problem, np.int32) if problem is not None else None
        V = np.ascontiguousarray(V0, np.float64) if V0 is not None else None
        Yend = np.zeros((n, self.KK))
        res = (Result * n)()
        nfail = self.L.cko_reactor_batch(ct.byref(self._mech), ct.byref(c), n, _ptr(prob) if prob is not None else None,
                                         _ptr(T0), _ptr(P0), _ptr(V) if V is not None else None, _ptr(Y0), _ptr(Yend),
                                         res, nthreads)
        del keep
        return nfail, res, Yend

    def reactor_batch_pert(self, T0, P0, Y0, pert_rxn, pert_fac, problem=None, V0=None, nthreads: int = 0, **cfg):
        """Batch with reactor i's A factor of reaction pert_rxn[i] multiplied by pert_fac[i]."""
        c, keep = self.make_cfg(**cfg)
        n = len(T0)
        T0 = np.ascontiguousarray(T0, np.float64)
        P0 = np.ascontiguousarray(P0, np.float64)
        Y0 = np.ascontiguousarray(Y0, np.float64).reshape(n, self.KK)
        prob = np.ascontiguousarray(problem, np.int32) if problem is not None else None
        V = np.ascontiguousarray(V0, np.float64) if V0 is not None else None
        pr = np.ascontiguousarray(pert_rxn, np.int32)
        pf = np.ascontiguousarray(pert_fac, np.float64)
        Yend = np.zeros((n, self.KK))
        res = (Result * n)()
        nfail = self.L.cko_reactor_batch_pert(ct.byref(self._mech), ct.byref(c), n,
                                              _ptr(prob) if prob is not None else None, _ptr(T0), _ptr(P0),
                                              _ptr(V) if V is not None else None, _ptr(Y0), _ptr(pr), _ptr(pf),
                                              _ptr(Yend), res, nthreads)
        del keep
        return nfail, res, Yend

    def rhs_jac(self, y, problem=1, energy=1, rho0=None, V0=1.0, P0=1.01325e6, t=0.0, **cfg):
        c, keep = self.make_cfg(problem=problem, energy=energy, **cfg)
        y = np.ascontiguousarray(y, np.float64)
        n = self.KK + 1
        f = np.zeros(n)
        J = np.zeros((n, n))
        if rho0 is None:
            Y = y[1:]
            rho0 = P0 / (8.31447247e7 * y[0]) / np.sum(Y / self.wt)
        self.L.cko_rhs_jac(ct.byref(self._mech), ct.byref(c), t, _ptr(y), rho0, V0, P0, _ptr(f), _ptr(J))
        return f, J

    def rhs_jac_engine(self, y, T0, P0, Y0, t=0.0, energy=1, **cfg):
        """f and J of the engine (problem 4) at (t, y) for the cylinder whose initial state is (T0, P0, Y0)."""
        c, keep = self.make_cfg(problem=4, energy=energy, **cfg)
        y = np.ascontiguousarray(y, np.float64)
        Y0 = np.ascontiguousarray(Y0, np.float64)
        n = self.KK + 1
        f = np.zeros(n)
        J = np.zeros((n, n))
        self.L.cko_rhs_jac_engine(ct.byref(self._mech), ct.byref(c), t, _ptr(y), float(T0), float(P0), _ptr(Y0),
                                  _ptr(f), _ptr(J))
        del keep
        return f, J
