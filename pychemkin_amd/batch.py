"""Batched reactor sweeps: the GPU-native replacement of the reference's serial run() loop.

The reference integrates a sweep one reactor at a time from Python
(tests/integration_tests/ignitiondelay.py:127-144, sensitivity.py:141-160).  ``BatchSweep``
takes the whole set of initial conditions, shards it by condition across the visible GPUs
(strided, so that cheap and expensive conditions are spread evenly) and
runs one ckmi_reactor_run launch per GPU.  There is no exchange between shards; results are
gathered on the host.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _native
from .chemistry import Chemistry
from .mixture import Mixture

PROBLEMS = {"CONP": 1, "CONV": 2, 1: 1, 2: 2}
ENERGIES = {"ENERGY": 1, "ENRG": 1, "GivenT": 2, "TGIV": 2, 1: 1, 2: 2}


@dataclass
class BatchResult:
    tau: np.ndarray          # ignition delay [s] (-1: not detected)
    T: np.ndarray            # final temperature [K]
    P: np.ndarray            # final pressure [dyn/cm2]
    V: np.ndarray            # final volume [cm3]
    Y: np.ndarray            # final mass fractions [n, KK]
    stats: np.ndarray        # [n, 8] int32 solver statistics (see _native.STAT_NAMES)
    wt: np.ndarray

    @property
    def ignition_delay_ms(self) -> np.ndarray:
        return self.tau * 1.0e3

    @property
    def status(self) -> np.ndarray:
        return self.stats[:, 6]

    @property
    def X(self) -> np.ndarray:
        x = self.Y / self.wt
        return x / x.sum(axis=1, keepdims=True)

    def statistics(self) -> Dict[str, np.ndarray]:
        return {k: self.stats[:, i] for i, k in enumerate(_native.STAT_NAMES)}


class BatchSweep:
    """Run many independent batch reactors that share one configuration."""

    def __init__(self, chem: Chemistry, problem="CONP", energy="ENERGY", t_end: float = 1.0, atol: float = 1.0e-12,
                 rtol: float = 1.0e-6, ignition: Optional[str] = "T_inflection", ign_val: float = 0.0,
                 ign_target: str = "", nneg: bool = False, h0: float = 0.0, hmax: float = 0.0,
                 ign_stop: bool = False, profile=None, max_steps: int = 0, devices: Optional[Sequence[int]] = None,
                 **keywords):
        """keywords: the remaining typed reactor keywords of _native.make_cfg -- gfac (GFAC), qloss (QLOS,
        cal/s), htc (HTC), areaq (AREAQ), tamb (TAMB), prof_kind (1: `profile` is TPRO), profile2 /
        prof2_kind (QPRO / AEXT), asteps / avar / avalue (adaptive solution points)."""
        self.chem = chem
        self.problem = PROBLEMS[problem]
        sp = chem.get_specindex(ign_target) if ignition == "Species_peak" else 0
        self.cfg = _native.make_cfg(energy=ENERGIES[energy], t_end=t_end, atol=max(atol, 1e-20),
                                    rtol=max(rtol, 1e-12), h0=h0, hmax=hmax, nneg=nneg, ign_mode=ignition,
                                    ign_val=ign_val, ign_species=sp, ign_stop=ign_stop, max_steps=max_steps,
                                    profile=profile, **keywords)
        self.devices = list(devices) if devices is not None else None

    def _devices(self) -> List[int]:
        import torch

        if self.devices is not None:
            return self.devices
        return list(range(torch.cuda.device_count()))

    def run(self, T0, P0, X0=None, Y0=None, V0=None, problem=None, afac_rxn=None, afac=None) -> BatchResult:
        """Integrate reactors i = 0..n-1 from (T0[i], P0[i], X0[i] or Y0[i], V0[i]).

        afac_rxn[i] / afac[i]: reactor i runs with the A factor of reaction afac_rxn[i] (0-based,
        -1 none) multiplied by afac[i] -- the batched form of set_reaction_AFactor + run()."""
        import torch

        T0 = np.asarray(T0, dtype=np.float64).reshape(-1)
        n = T0.size
        P0 = np.broadcast_to(np.asarray(P0, dtype=np.float64), (n,)).copy()
        V0 = np.ones(n) if V0 is None else np.broadcast_to(np.asarray(V0, dtype=np.float64), (n,)).copy()
        wt = self.chem.WT
        if Y0 is None:
            if X0 is None:
                raise ValueError("X0 or Y0 is required")
            X = np.atleast_2d(np.asarray(X0, dtype=np.float64))
            X = np.broadcast_to(X, (n, wt.size))
            Y = X * wt
            Y0 = Y / Y.sum(axis=1, keepdims=True)
        Y0 = np.ascontiguousarray(np.broadcast_to(np.atleast_2d(np.asarray(Y0, dtype=np.float64)), (n, wt.size)))
        if problem is None:
            prob = np.full(n, self.problem, np.int32)
        else:
            prob = np.asarray([PROBLEMS[p] for p in np.broadcast_to(np.asarray(problem, dtype=object), (n,))], np.int32)
        devs = self._devices()
        if not devs:
            raise _native.NativeError("no ROCm GPU visible: BatchSweep requires at least one MI355X")
        shards = [np.arange(r, n, len(devs)) for r in range(len(devs))]
        pending = []
        for d, idx in zip(devs, shards):
            if idx.size == 0:
                continue
            dm = self.chem.device_mechanism(d)
            pert = {}
            if afac_rxn is not None:
                pert = dict(afac_rxn=np.asarray(afac_rxn, np.int32).reshape(-1)[idx],
                            afac=np.broadcast_to(np.asarray(afac, np.float64), (n,))[idx])
            with torch.cuda.device(d):
                res = dm.reactor_run(self.cfg, prob[idx], T0[idx], P0[idx], V0[idx], Y0[idx], **pert)
            pending.append((idx, res))
        out = BatchResult(tau=np.empty(n), T=np.empty(n), P=np.empty(n), V=np.empty(n), Y=np.empty((n, wt.size)),
                          stats=np.empty((n, _native.NSTAT), np.int32), wt=wt)
        for idx, res in pending:
            out.tau[idx] = res["tau"].cpu().numpy()
            out.T[idx] = res["T"].cpu().numpy()
            out.P[idx] = res["P"].cpu().numpy()
            out.V[idx] = res["V"].cpu().numpy()
            out.Y[idx] = res["Y"].cpu().numpy()
            out.stats[idx] = res["stats"].cpu().numpy()
        return out

    def run_mixtures(self, mixtures: Sequence[Mixture], V0=None, problem=None) -> BatchResult:
        T0 = [m.temperature for m in mixtures]
        P0 = [m.pressure for m in mixtures]
        Y0 = np.stack([m.Y for m in mixtures])
        return self.run(T0, P0, Y0=Y0, V0=V0, problem=problem)


@dataclass
class PSRResult:
    T: np.ndarray            # steady-state temperature [K]
    Y: np.ndarray            # steady-state mass fractions [n, KK]
    rho: np.ndarray          # density [g/cm3]
    tau: np.ndarray          # residence time [s] (given, or rho V / mdot)
    volume: np.ndarray       # reactor volume [cm3] (given, or tau mdot / rho)
    resid: np.ndarray        # largest scaled residual of the steady-state rule (<= 1: steady)
    mdot: np.ndarray         # exit mass flow rate [g/s] (= the inlet's: steady state)
    P: np.ndarray            # pressure [dyn/cm2]
    stats: np.ndarray        # [n, 8] int32 solver statistics (see _native.STAT_NAMES)
    wt: np.ndarray

    @property
    def status(self) -> np.ndarray:
        """0 steady; 6 (_native.RUN_NOT_STEADY) t_max reached first; 1-4 as for the closed reactors."""
        return self.stats[:, 6]

    @property
    def X(self) -> np.ndarray:
        x = self.Y / self.wt
        return x / x.sum(axis=1, keepdims=True)


class BatchPSR:
    """Many independent steady-state perfectly stirred reactors in one launch per GPU.

    Each reactor marches the open-reactor equations (include/ckmi.h ckmi_psr_run) from its estimate
    until they are steady.  The result is therefore the steady state that the transient reaches FROM THE
    ESTIMATE: on an S-curve a burnt estimate stays on the ignited branch, an unburnt one may blow out to
    the inlet state, whereas Chemkin's damped Newton solver can land on either branch from the same
    estimate.  ``estimate="burnt"`` is the estimate to use for the ignited branch.
    """

    def __init__(self, chem: Chemistry, mode: str = "residence_time", energy="ENERGY", ss_rtol: float = 1.0e-8,
                 ss_atol: float = 1.0e-14, rtol: float = 1.0e-8, atol: float = 1.0e-14, t_max: float = 0.0,
                 qloss: float = 0.0, htc: float = 0.0, areaq: float = 0.0, tamb: float = 300.0, gfac: float = 1.0,
                 max_steps: int = 0, devices: Optional[Sequence[int]] = None):
        """mode: "residence_time" (tau given) or "volume" (V given); energy: "ENERGY" or "TGIV" (the
        temperature stays at the estimate's); ss_rtol / ss_atol: the steady-state rule; rtol / atol: the
        time integrator; t_max: give up (status 6) after this time [s], 0 = 1000 residence times; qloss
        [cal/s], htc [cal/(cm2 K s)], areaq [cm2], tamb [K]: Q = qloss + htc areaq (T - tamb)."""
        if mode not in ("residence_time", "volume"):
            raise ValueError('mode must be "residence_time" or "volume"')
        self.chem = chem
        self.mode = 1 if mode == "residence_time" else 2
        self.ss_rtol, self.ss_atol = float(ss_rtol), float(ss_atol)
        self.energy = ENERGIES[energy]
        self.cfg = _native.make_cfg(energy=self.energy, t_end=t_max, atol=max(atol, 1e-20), rtol=max(rtol, 1e-12),
                                    qloss=qloss, htc=htc, areaq=areaq, tamb=tamb, gfac=gfac, max_steps=max_steps)
        self.devices = list(devices) if devices is not None else None

    _devices = BatchSweep._devices

    def _fractions(self, n, X, Y, what):
        wt = self.chem.WT
        if Y is None:
            if X is None:
                raise ValueError(f"{what}: X or Y is required")
            Yv = np.broadcast_to(np.atleast_2d(np.asarray(X, dtype=np.float64)), (n, wt.size)) * wt
            Y = Yv / Yv.sum(axis=1, keepdims=True)
        return np.ascontiguousarray(np.broadcast_to(np.atleast_2d(np.asarray(Y, dtype=np.float64)), (n, wt.size)))

    def burnt_estimate(self, P, Yin):
        """End state (T, Y) of an adiabatic constant-pressure closed reactor started from the inlet
        composition at 1600 K and run for 10 ms: one BatchSweep launch over the distinct (P, Yin) rows."""
        key = np.concatenate([P[:, None], Yin], axis=1)
        uniq, inv = np.unique(key, axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        sweep = BatchSweep(self.chem, problem="CONP", energy="ENERGY", t_end=1.0e-2, atol=1e-12, rtol=1e-8,
                           ignition=None, devices=self.devices)
        r = sweep.run(np.full(uniq.shape[0], 1600.0), uniq[:, 0], Y0=uniq[:, 1:])
        if np.any(r.status != 0):
            raise _native.NativeError("the burnt estimate's closed reactors failed: status " + str(r.status.tolist()))
        return r.T[inv], r.Y[inv]

    def equilibrium_estimate(self, Tin, P, Yin):
        """HP equilibrium (T, Y) of each inlet -- the reference PSR model's own estimate (stirreactors/PSR.py:
        324,362): one BatchEquilibrium launch over the distinct (Tin, P, Yin) rows."""
        key = np.concatenate([Tin[:, None], P[:, None], Yin], axis=1)
        uniq, inv = np.unique(key, axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        r = BatchEquilibrium(self.chem, devices=self.devices).run(5, uniq[:, 0], uniq[:, 1], Y=uniq[:, 2:])
        if np.any(r.status != 0):
            raise _native.NativeError("the equilibrium estimate did not converge: status " + str(r.status.tolist()))
        return r.T[inv], r.Y[inv]

    def run(self, Tin, P, mdot, tau=None, volume=None, Xin=None, Yin=None, estimate="inlet",
            T_estimate=None, X_estimate=None, Y_estimate=None) -> PSRResult:
        """Solve reactors i = 0..n-1 (every input broadcasts over the reactors).

        Tin [K], P [dyn/cm2], mdot [g/s], Xin or Yin: the one effective inlet of each reactor; tau [s] or
        volume [cm3] by the mode.  estimate: "inlet" (the inlet state; T_estimate overrides its
        temperature), "burnt" (burnt_estimate), "equilibrium" (equilibrium_estimate: the HP equilibrium of the
        inlet), or "given" with T_estimate and X_estimate / Y_estimate."""
        import torch

        tv = tau if self.mode == 1 else volume
        if tv is None:
            raise ValueError("tau is required" if self.mode == 1 else "volume is required")
        arrs = np.broadcast_arrays(*[np.asarray(v, dtype=np.float64).reshape(-1) for v in (Tin, P, mdot, tv)])
        n = arrs[0].size
        if Xin is not None and np.ndim(Xin) == 2:
            n = max(n, np.shape(Xin)[0])
        if Yin is not None and np.ndim(Yin) == 2:
            n = max(n, np.shape(Yin)[0])
        if T_estimate is not None:
            n = max(n, np.asarray(T_estimate).size)
        Tin, P, mdot, tv = (np.broadcast_to(a, (n,)).copy() for a in arrs)
        if np.any(Tin <= 0) or np.any(P <= 0) or np.any(mdot <= 0) or np.any(tv <= 0):
            raise ValueError("Tin, P, mdot and tau / volume must be > 0")
        Yin = self._fractions(n, Xin, Yin, "inlet")
        if estimate == "burnt":
            Tg, Yg = self.burnt_estimate(P, Yin)
        elif estimate == "equilibrium":
            Tg, Yg = self.equilibrium_estimate(Tin, P, Yin)
        elif estimate == "inlet":
            Tg, Yg = Tin.copy(), Yin
            if T_estimate is not None:
                Tg = np.broadcast_to(np.asarray(T_estimate, dtype=np.float64).reshape(-1), (n,)).copy()
        elif estimate == "given":
            if T_estimate is None:
                raise ValueError('estimate="given" needs T_estimate')
            Tg = np.broadcast_to(np.asarray(T_estimate, dtype=np.float64).reshape(-1), (n,)).copy()
            Yg = self._fractions(n, X_estimate, Y_estimate, "estimate")
        else:
            raise ValueError('estimate must be "inlet", "burnt", "equilibrium" or "given"')
        devs = self._devices()
        if not devs:
            raise _native.NativeError("no ROCm GPU visible: BatchPSR requires at least one MI355X")
        shards = [np.arange(r, n, len(devs)) for r in range(len(devs))]
        pending = []
        for d, idx in zip(devs, shards):
            if idx.size == 0:
                continue
            dm = self.chem.device_mechanism(d)
            with torch.cuda.device(d):
                res = dm.psr_run(self.cfg, self.mode, P[idx], Tin[idx], Yin[idx], mdot[idx], tv[idx], Tg[idx],
                                 Yg[idx], ss_rtol=self.ss_rtol, ss_atol=self.ss_atol)
            pending.append((idx, res))
        wt = self.chem.WT
        out = PSRResult(T=np.empty(n), Y=np.empty((n, wt.size)), rho=np.empty(n), tau=np.empty(n),
                        volume=np.empty(n), resid=np.empty(n), mdot=mdot, P=P,
                        stats=np.empty((n, _native.NSTAT), np.int32), wt=wt)
        for idx, res in pending:
            out.T[idx] = res["T"].cpu().numpy()
            out.Y[idx] = res["Y"].cpu().numpy()
            out.rho[idx] = res["rho"].cpu().numpy()
            out.tau[idx] = res["tau"].cpu().numpy()
            out.volume[idx] = res["vol"].cpu().numpy()
            out.resid[idx] = res["resid"].cpu().numpy()
            out.stats[idx] = res["stats"].cpu().numpy()
        return out


@dataclass
class NetworkResult:
    T: np.ndarray            # [n, R] steady-state temperatures [K]
    Y: np.ndarray            # [n, R, KK] mass fractions
    mdot: np.ndarray         # [n, R] through-flow of every reactor [g/s] (the linear flow balance)
    rho: np.ndarray          # [n, R] density [g/cm3]
    tau: np.ndarray          # [n, R] residence time [s]
    volume: np.ndarray       # [n, R] volume [cm3]
    resid: np.ndarray        # [n, R] scaled residual of the steady-state rule at the last solve (<= 1: steady)
    stats: np.ndarray        # [n, R, 8] int32 solver statistics of the last solve (see _native.STAT_NAMES)
    P: np.ndarray            # [n, R] pressure [dyn/cm2]
    split: np.ndarray        # [n, R, R + 1] the outflow split the networks were run with (column R: the exit)
    status: np.ndarray       # [n] 0 ok, 10 tear iteration limit, 11 a reactor failed, 12 flow balance singular
    sweeps: np.ndarray       # [n] Gauss-Seidel sweeps taken
    tear_resid: np.ndarray   # [n] scaled change of the tear points over the last sweep (<= 1: converged)
    feed_forward: np.ndarray  # [n] bool: no recycle, solved in one sweep
    wt: np.ndarray

    @property
    def X(self) -> np.ndarray:
        x = self.Y / self.wt
        return x / x.sum(axis=-1, keepdims=True)

    @property
    def reactor_status(self) -> np.ndarray:
        """[n, R] status of every reactor's last solve (0 steady, -1 no inlet stream reached it)."""
        return self.stats[:, :, 6]

    @property
    def exit_mdot(self) -> np.ndarray:
        """[n, R] mass flow rate that leaves the network from every reactor [g/s] (0: no exit there)."""
        return self.mdot * self.split[:, :, -1]

    def exit_streams(self, net: int = 0):
        """The exit streams of network `net`: a list of (reactor index, mdot [g/s], T [K], Y) for every reactor
        with an exit fraction."""
        return [(i, float(self.exit_mdot[net, i]), float(self.T[net, i]), self.Y[net, i].copy())
                for i in range(self.T.shape[1]) if self.split[net, i, -1] > 0.0]


class BatchPSRNetwork:
    """Many independent networks of R steady-state PSRs with recycle streams, one ckmi_psr_network_run call per
    GPU (the reference's hybridreactornetwork.ReactorNetwork solves one network, one reactor at a
    time).  Gauss-Seidel over the reactors in the order given, tear-stream iteration when there is recycle.

    Every per-position option (mode, energy, the tolerances, heat loss) is a scalar or a sequence of R values."""

    ESTIMATES = ("given", "inlet", "burnt")

    def __init__(self, chem: Chemistry, R: int, mode="residence_time", energy="ENERGY", ss_rtol=1.0e-8, ss_atol=1.0e-14,
                 rtol=1.0e-8, atol=1.0e-14, t_max=0.0, qloss=0.0, htc=0.0, areaq=0.0, tamb=300.0, gfac=1.0,
                 max_steps: int = 0, max_sweeps: int = 200, tear_rtol: float = 1.0e-6, tear_atol: float = 1.0e-8,
                 relax: float = 1.0, devices: Optional[Sequence[int]] = None):
        R = int(R)
        if R < 1 or R > _native.NET_RMAX:
            raise ValueError(f"a network has 1..{_native.NET_RMAX} reactors")

        def per(v, what):
            seq = [v] * R if isinstance(v, (str, int, float, np.floating, np.integer)) else list(v)
            if len(seq) != R:
                raise ValueError(f"{what} needs one value or {R} values")
            return seq

        self.chem, self.R = chem, R
        modes = per(mode, "mode")
        if any(m not in ("residence_time", "volume") for m in modes):
            raise ValueError('mode must be "residence_time" or "volume"')
        self.modes = [1 if m == "residence_time" else 2 for m in modes]
        en = [ENERGIES[e] for e in per(energy, "energy")]
        self.ss_tols = list(zip(map(float, per(ss_rtol, "ss_rtol")), map(float, per(ss_atol, "ss_atol"))))
        self.max_sweeps, self.tear_rtol, self.tear_atol, self.relax = int(max_sweeps), float(tear_rtol), \
            float(tear_atol), float(relax)
        if self.max_sweeps < 1 or self.tear_rtol <= 0.0 or self.tear_atol < 0.0 or self.relax <= 0.0:
            raise ValueError("max_sweeps must be >= 1, tear_rtol > 0, tear_atol >= 0 and relax > 0")
        if any(self.tear_rtol < t[0] for t in self.ss_tols):
            raise ValueError("tear_rtol must be >= ss_rtol of every position: the tear test cannot resolve changes "
                             "below the steady-state rule of the reactors")
        opts = [per(v, k) for k, v in (("rtol", rtol), ("atol", atol), ("t_max", t_max), ("qloss", qloss), ("htc", htc),
                                       ("areaq", areaq), ("tamb", tamb), ("gfac", gfac))]
        self.cfgs = [_native.make_cfg(energy=en[i], t_end=opts[2][i], atol=max(opts[1][i], 1e-20),
                                      rtol=max(opts[0][i], 1e-12), qloss=opts[3][i], htc=opts[4][i], areaq=opts[5][i],
                                      tamb=opts[6][i], gfac=opts[7][i], max_steps=max_steps) for i in range(R)]
        self.devices = list(devices) if devices is not None else None

    _devices = BatchSweep._devices

    @staticmethod
    def check_split(split: np.ndarray) -> None:
        """ValueError unless every split row sums to 1 within 1e-12, every fraction lies in [0, 1] and no reactor
        feeds itself.  split [..., R, R + 1]."""
        if np.any(~np.isfinite(split)) or np.any(split < 0.0) or np.any(split > 1.0):
            raise ValueError("split fractions must lie in [0, 1]")
        if np.any(np.abs(split.sum(axis=-1) - 1.0) > 1e-12):
            raise ValueError("every split row must sum to 1 (within 1e-12): a reactor's outflow goes somewhere")
        R = split.shape[-2]
        if np.any(split[..., np.arange(R), np.arange(R)] != 0.0):
            raise ValueError("a reactor cannot feed itself")

    def run(self, P, split, ext_mdot, ext_T, ext_X=None, ext_Y=None, tau=None, volume=None, estimate="burnt",
            T_estimate=None, X_estimate=None, Y_estimate=None, tear=None) -> NetworkResult:
        """Solve networks 0..n-1; every input broadcasts over the networks (give it without the leading axis).

        P [n, R] dyn/cm2; split [n, R, R + 1] (row j: where reactor j's outflow goes, last column the exit);
        ext_mdot, ext_T [n, R, E] and ext_X or ext_Y [n, R, E, KK]: the external inlets in E padded slots
        (mdot = 0: unused); tau / volume [n, R] by each position's mode; tear [n, R] marks the tear points.
        estimate: one of "given" (T_estimate and X_estimate / Y_estimate), "inlet" (T_estimate with the effective
        inlet's composition) and "burnt" (BatchPSR.burnt_estimate on the network's combined external feed at the
        reactor's pressure; T_estimate overrides its temperature), or one per reactor."""
        import torch

        R, KK = self.R, self.chem.KK
        wt = self.chem.WT
        split = np.asarray(split, dtype=np.float64)
        ext_mdot = np.asarray(ext_mdot, dtype=np.float64)
        ext_T = np.asarray(ext_T, dtype=np.float64)
        if split.shape[-2:] != (R, R + 1):
            raise ValueError(f"split must be [..., {R}, {R + 1}]")
        if ext_mdot.ndim < 2 or ext_mdot.shape[-2] != R:
            raise ValueError(f"ext_mdot must be [..., {R}, E]")
        E = ext_mdot.shape[-1]
        ext_f = ext_Y if ext_Y is not None else ext_X
        if ext_f is None:
            raise ValueError("ext_X or ext_Y is required")
        ext_f = np.asarray(ext_f, dtype=np.float64)
        if ext_f.shape[-3:] != (R, E, KK):
            raise ValueError(f"the external inlets' fractions must be [..., {R}, {E}, {KK}]")
        tv_in = [None if v is None else np.asarray(v, dtype=np.float64) for v in (tau, volume)]
        n = 1
        for a, nd in ((split, 3), (ext_mdot, 3), (ext_T, 3), (ext_f, 4), (np.asarray(P), 2), (tv_in[0], 2),
                      (tv_in[1], 2), (None if T_estimate is None else np.asarray(T_estimate), 2),
                      (None if tear is None else np.asarray(tear), 2)):
            if a is not None and a.ndim == nd:
                n = max(n, a.shape[0])
        split = np.ascontiguousarray(np.broadcast_to(split, (n, R, R + 1)))
        ext_mdot = np.ascontiguousarray(np.broadcast_to(ext_mdot, (n, R, E)))
        ext_T = np.ascontiguousarray(np.broadcast_to(ext_T, (n, R, E)))
        ext_f = np.broadcast_to(ext_f, (n, R, E, KK))
        if ext_Y is None:
            yy = ext_f * wt
            s = yy.sum(axis=-1, keepdims=True)
            ext_f = np.where(s > 0.0, yy / np.where(s > 0.0, s, 1.0), 0.0)
        ext_Yv = np.ascontiguousarray(ext_f)
        P = np.ascontiguousarray(np.broadcast_to(np.asarray(P, dtype=np.float64), (n, R)))
        tv = np.empty((n, R))
        for i, m in enumerate(self.modes):
            v = tv_in[m - 1]
            if v is None:
                raise ValueError(f"reactor {i}: " + ("tau is required" if m == 1 else "volume is required"))
            tv[:, i] = np.broadcast_to(v, (n, R))[:, i]
        tear = np.zeros((n, R), np.int32) if tear is None else \
            np.ascontiguousarray(np.broadcast_to(np.asarray(tear).astype(np.int32), (n, R)))
        # ---- validation
        self.check_split(split)
        if np.any(ext_mdot < 0.0) or np.any(~np.isfinite(ext_mdot)):
            raise ValueError("external mass flow rates must be >= 0")
        if np.any(ext_mdot[:, 0].sum(axis=-1) <= 0.0):
            raise ValueError("the first reactor of a network needs an external inlet")
        used = ext_mdot > 0.0
        if np.any(P <= 0.0) or np.any(tv <= 0.0) or np.any(ext_T[used] <= 0.0):
            raise ValueError("P, tau / volume and the inlet temperatures must be > 0")
        if np.any(np.abs(ext_Yv[used].sum(axis=-1) - 1.0) > 1e-9):
            raise ValueError("the fractions of a used external inlet must sum to 1")
        # ---- estimates
        est = [estimate] * R if isinstance(estimate, str) else list(estimate)
        if len(est) != R or any(e not in self.ESTIMATES for e in est):
            raise ValueError(f'estimate must be one of {self.ESTIMATES}, or {R} of them')
        Tg = np.full((n, R), np.nan) if T_estimate is None else \
            np.broadcast_to(np.asarray(T_estimate, dtype=np.float64), (n, R)).copy()
        Yg = np.zeros((n, R, KK))
        Yg[:, :, 0] = 1.0
        if any(e == "given" for e in est):
            f = Y_estimate if Y_estimate is not None else X_estimate
            if f is None:
                raise ValueError('estimate="given" needs X_estimate or Y_estimate')
            f = np.broadcast_to(np.asarray(f, dtype=np.float64), (n, R, KK))
            if Y_estimate is None:
                f = f * wt
                f = f / f.sum(axis=-1, keepdims=True)
            for i in range(R):
                if est[i] == "given":
                    Yg[:, i] = f[:, i]
        if any(e == "burnt" for e in est):
            m_all = ext_mdot.reshape(n, R * E)
            feed = np.einsum("ns,nsk->nk", m_all, ext_Yv.reshape(n, R * E, KK)) / m_all.sum(axis=1, keepdims=True)
            cols = [i for i in range(R) if est[i] == "burnt"]
            helper = BatchPSR(self.chem, devices=self.devices)
            Tb, Yb = helper.burnt_estimate(P[:, cols].reshape(-1), np.repeat(feed, len(cols), axis=0))
            Tb, Yb = Tb.reshape(n, len(cols)), Yb.reshape(n, len(cols), KK)
            for c, i in enumerate(cols):
                Yg[:, i] = Yb[:, c]
                Tg[:, i] = np.where(np.isnan(Tg[:, i]), Tb[:, c], Tg[:, i])
        if np.any(np.isnan(Tg)) or np.any(Tg <= 0.0):
            raise ValueError('estimates "given" and "inlet" need T_estimate > 0')
        gmode = [1 if e == "inlet" else 0 for e in est]
        # ---- launches
        devs = self._devices()
        if not devs:
            raise _native.NativeError("no ROCm GPU visible: BatchPSRNetwork requires at least one MI355X")
        shards = [np.arange(r, n, len(devs)) for r in range(len(devs))]
        pending = []
        for d, idx in zip(devs, shards):
            if idx.size == 0:
                continue
            dm = self.chem.device_mechanism(d)
            with torch.cuda.device(d):
                res = dm.psr_network_run(self.cfgs, self.modes, self.ss_tols, gmode, P[idx], split[idx], ext_mdot[idx],
                                         ext_T[idx], ext_Yv[idx], tv[idx], Tg[idx], Yg[idx], tear[idx],
                                         max_sweeps=self.max_sweeps, tear_rtol=self.tear_rtol, tear_atol=self.tear_atol,
                                         relax=self.relax)
            pending.append((idx, res))
        out = NetworkResult(T=np.empty((n, R)), Y=np.empty((n, R, KK)), mdot=np.empty((n, R)), rho=np.empty((n, R)),
                            tau=np.empty((n, R)), volume=np.empty((n, R)), resid=np.empty((n, R)),
                            stats=np.empty((n, R, _native.NSTAT), np.int32), P=P, split=split,
                            status=np.empty(n, np.int32), sweeps=np.empty(n, np.int32), tear_resid=np.empty(n),
                            feed_forward=np.empty(n, bool), wt=wt)
        for idx, res in pending:
            for name, key in (("T", "T"), ("Y", "Y"), ("mdot", "mdot"), ("rho", "rho"), ("tau", "tau"),
                              ("volume", "vol"), ("resid", "resid"), ("stats", "stats"), ("tear_resid", "tear_resid")):
                getattr(out, name)[idx] = res[key].cpu().numpy()
            ns = res["net_stats"].cpu().numpy()
            out.status[idx], out.sweeps[idx], out.feed_forward[idx] = ns[:, 0], ns[:, 1], (ns[:, 2] & 1) != 0
        return out


@dataclass
class EquilibriumResult:
    T: np.ndarray            # equilibrium temperature [K]
    P: np.ndarray            # equilibrium pressure [dyn/cm2]
    Y: np.ndarray            # equilibrium mass fractions [n, KK]
    sound: np.ndarray        # option 10: sound speed of the burnt gas [cm/s] (= D V2 / V1), else 0
    detspeed: np.ndarray     # option 10: detonation wave speed D [cm/s], else 0
    iterations: np.ndarray   # Newton iterations
    status: np.ndarray       # 0 converged, 7 (_native.RUN_EQ_NOT_CONVERGED) not: the state is the last iterate
    wt: np.ndarray

    @property
    def X(self) -> np.ndarray:
        x = self.Y / self.wt
        return x / x.sum(axis=1, keepdims=True)


class BatchEquilibrium:
    """Many independent chemical-equilibrium and Chapman-Jouguet states in one launch per GPU
    (include/ckmi.h ckmi_equil_run): flame-temperature maps, equilibrium tables, estimates for PSRs."""

    def __init__(self, chem: Chemistry, devices: Optional[Sequence[int]] = None, tol: float = 0.0, max_iter: int = 0):
        """tol / max_iter: the Newton tolerance and iteration cap (0: the defaults, 1e-12 and 200)."""
        self.chem = chem
        self.devices = list(devices) if devices is not None else None
        self.tol, self.max_iter = float(tol), int(max_iter)

    _devices = BatchSweep._devices
    _fractions = BatchPSR._fractions

    def run(self, option, T, P, X=None, Y=None) -> EquilibriumResult:
        """States i = 0..n-1 from (T[i] K, P[i] dyn/cm2, X[i] or Y[i]) under option[i] (1..10, see
        mixture.calculate_equilibrium); every input broadcasts over the states."""
        import torch

        wt = self.chem.WT
        arrs = [np.asarray(option).reshape(-1), np.asarray(T, dtype=np.float64).reshape(-1),
                np.asarray(P, dtype=np.float64).reshape(-1)]
        n = max(a.size for a in arrs)
        for f in (X, Y):
            if f is not None and np.ndim(f) == 2:
                n = max(n, np.shape(f)[0])
        option, T, P = (np.broadcast_to(a, (n,)).copy() for a in arrs)
        if np.any(option != option.astype(np.int32)) or np.any((option < 1) | (option > 10)):
            raise ValueError("option must be an integer 1..10 for every state")
        if np.any(T <= 0) or np.any(P <= 0):
            raise ValueError("T and P must be > 0")
        Yv = self._fractions(n, X, Y, "state")
        option = option.astype(np.int32)
        devs = self._devices()
        if not devs:
            raise _native.NativeError("no ROCm GPU visible: BatchEquilibrium requires at least one MI355X")
        shards = [np.arange(r, n, len(devs)) for r in range(len(devs))]
        pending = []
        for d, idx in zip(devs, shards):
            if idx.size == 0:
                continue
            dm = self.chem.device_mechanism(d)
            with torch.cuda.device(d):
                res = dm.equil_run(option[idx], T[idx], P[idx], Yv[idx], tol=self.tol, max_iter=self.max_iter)
            pending.append((idx, res))
        out = EquilibriumResult(T=np.empty(n), P=np.empty(n), Y=np.empty((n, wt.size)), sound=np.empty(n),
                                detspeed=np.empty(n), iterations=np.empty(n, np.int32), status=np.empty(n, np.int32),
                                wt=wt)
        for idx, res in pending:
            out.T[idx] = res["T"].cpu().numpy()
            out.P[idx] = res["P"].cpu().numpy()
            out.Y[idx] = res["Y"].cpu().numpy()
            out.sound[idx] = res["sound"].cpu().numpy()
            out.detspeed[idx] = res["detspeed"].cpu().numpy()
            st = res["stats"].cpu().numpy()
            out.iterations[idx] = st[:, 0]
            out.status[idx] = st[:, 1]
        return out


def afactor_sensitivity(chem: Chemistry, mixture: Mixture, factor: float = 1.001, reactions: Optional[Sequence[int]] = None,
                        volume: float = 1.0, **sweep_kw) -> Dict[str, np.ndarray]:
    """Brute-force A-factor sensitivity of the ignition delay (reference sensitivity.py:122-160).

    The reference perturbs one reaction's A by `factor` and re-runs the reactor serially (326
    native runs for GRI-3.0).  Here the nominal reactor and every perturbed one are reactors of
    ONE batch (per-reactor A multiplier, ckmi_reactor_run_ex), sharded over the visible GPUs.
    Returns S_i = (tau_i - tau_0) / (factor - 1) [s] per 0-based reaction, tau_0 [s], and the
    per-reactor status.
    """
    II = chem.IIGas
    rx = np.arange(II) if reactions is None else np.asarray(list(reactions), dtype=np.int64)
    if np.any(rx < 0) or np.any(rx >= II):
        raise ValueError("reaction indices must be 0-based and < IIGas")
    n = rx.size + 1
    sweep = BatchSweep(chem, **sweep_kw)
    afac_rxn = np.concatenate([[-1], rx]).astype(np.int32)
    r = sweep.run(np.full(n, mixture.temperature), np.full(n, mixture.pressure), Y0=np.tile(mixture.Y, (n, 1)),
                  V0=np.full(n, volume), afac_rxn=afac_rxn, afac=np.full(n, float(factor)))
    tau0 = float(r.tau[0])
    sens = (r.tau[1:] - tau0) / (factor - 1.0)
    return {"reactions": rx, "sensitivity": sens, "tau0": tau0, "status": r.status.copy()}
