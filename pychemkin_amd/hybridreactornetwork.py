"""Hybrid reactor network: PSRs joined by outflow splits and recycle streams (drop-in for the reference's
hybridreactornetwork.py:39-1463), solved on the GPU.

``ReactorNetwork`` keeps the reference's public methods and signatures.  ``run()`` is ONE
``pychemkin_amd.batch.BatchPSRNetwork`` call with a single network built from the member PSR objects: their
external inlets, residence time or volume, estimate, tolerances and heat loss, one configuration per position
(DESIGN.md §13).  The reactors are solved in the order they were added (Gauss-Seidel); with recycle the sweeps
repeat until the declared tear points stop changing.  Reactor indices are 1-based as in the reference.

Differences from the reference, all on purpose:
  * errors raise ReactorError; nothing calls exit();
  * the tear test asks EVERY tear point to meet the tolerance (the reference joins them by `or`);
  * a network with recycle but no declared tear point is iterated with every reactor as a tear point (the
    reference makes one pass and ignores the recycle);
  * a member's steady-state rule is tightened to a tenth of the tear tolerance where it is looser: time marching,
    unlike a converged Newton iteration, leaves an error of the size of its rule in every solve, and a tear test at
    the same level would be judging that error instead of the coupling;
  * plug-flow members, reactor clusters, surface chemistry and heat exchange between reactors are not covered.
"""
from __future__ import annotations

import copy
from typing import Dict, List, Tuple, Union

import numpy as np

from .chemistry import Chemistry
from .flowreactors.PFR import PlugFlowReactor as PFR
from .inlet import Stream
from .logger import logger
from .reactormodel import ReactorError
from .stirreactors.PSR import perfectlystirredreactor as PSR


class ReactorNetwork:
    """Reactors solved one after another, with outflow splitting and tear-stream iteration for recycle."""

    def __init__(self, chem: Chemistry):
        if not isinstance(chem, Chemistry):
            raise ReactorError('the parameter must be a "Chemistry Set" object')
        self.network_chem = chem
        self.numb_reactors = 0
        self.last_reactor = 0
        self._exit_index = -10
        self._exit_name = "EXIT>>"
        self.numb_external_outlet = 0
        self.external_outlets: Dict[int, int] = {}           # {outlet index: reactor index}
        self.external_outlet_streams: Dict[int, Stream] = {}
        self.reactor_map: Dict[str, int] = {}                # {label: reactor index}
        self.reactor_objects: Dict[int, Union[PSR, PFR]] = {}
        self.reactor_solutions: Dict[int, Stream] = {}       # {reactor index: solution Stream with the through-flow}
        self.outflow_targets: Dict[int, List[Tuple[int, float]]] = {}
        self._declared: Dict[int, List[Tuple[int, float]]] = {}  # what add_outflow_connections was given
        self.outflow_altered = True
        self.external_connections: Dict[int, int] = {}
        self.inflow_sources: Dict[int, List[Tuple[int, float]]] = {}
        self.numb_tearpoints = 0
        self.tearpoint: List[int] = []
        self.max_tearloop_count = 200
        self.tolerance = 1.0e-6
        self.relaxation_factor = 1.0
        self.tear_converged = False
        self.network_run_status = -100
        self.result = None  # the NetworkResult of the last run (sweeps, tear residual, per-reactor statistics)

    # ------------------------------------------------------------------ members
    def get_reactor_label(self, reactor_index: int) -> str:
        for name, idx in self.reactor_map.items():
            if idx == reactor_index:
                return name
        logger.warning("reactor # %s is NOT found in the network.", reactor_index)
        return ""

    def add_reactor(self, reactor: Union[PSR, PFR]):
        """Add a reactor; the order of addition is the order of solution."""
        if isinstance(reactor, PFR):
            raise ReactorError(f"reactor {reactor.label}: plug-flow members are not on this path (PSR networks only)")
        if not isinstance(reactor, PSR):
            raise ReactorError("a network member must be a PSR object")
        label = reactor.label
        if label in self.reactor_map:
            logger.warning("reactor already in the network.")
            return
        if self.numb_reactors == 0 and reactor.numbexternalinlets <= 0:
            raise ReactorError(f"reactor number 1 {label} has NO external inlet.")
        self.numb_reactors += 1
        self.last_reactor = self.numb_reactors
        self.reactor_map[label] = self.numb_reactors
        self.reactor_objects[self.numb_reactors] = reactor
        self.external_connections[self.numb_reactors] = reactor.number_external_inlets
        self.outflow_altered = True

    def add_reactor_list(self, reactor_list: List[Union[PSR, PFR]]):
        for rxtor in reactor_list:
            self.add_reactor(rxtor)

    def show_reactors(self):
        if self.numb_reactors <= 0:
            logger.info("reactor network contains no reactor.")
        for name, idx in self.reactor_map.items():
            print(f"  Reactor No. {idx}: {name}")

    @property
    def number_reactors(self) -> int:
        return self.numb_reactors

    @property
    def number_external_outlets(self) -> int:
        return self.numb_external_outlet

    # ------------------------------------------------------------------ connections
    def show_internal_outflow_connections(self):
        table = self.outflow_targets if self.outflow_targets else self._chain_table()
        for idx in sorted(table):
            print(f"reactor number {idx}: {self.get_reactor_label(idx)}")
            print("-- outflow connections --")
            for target, frac in table[idx]:
                if target == self._exit_index:
                    print(f"  *external outlet flow*: {frac}")
                else:
                    if target == idx + 1:
                        print("  *through flow*")
                    print(f"  reactor no. {target} {self.get_reactor_label(target)}: {frac}")
            print("-" * 10)

    def show_internal_inflow_connections(self):
        sources = self._sources(self.outflow_targets if self.outflow_targets else self._chain_table())
        for idx in self.reactor_map.values():
            print(f"reactor number {idx}: {self.get_reactor_label(idx)}")
            print("-- internal inlet sources --")
            if not sources.get(idx):
                print("  *no internal inlet stream from other reactors*")
            for src, frac in sources.get(idx, []):
                if src == idx - 1:
                    print("  *through flow*")
                print(f"  reactor no. {src} {self.get_reactor_label(src)}: {frac}")
            print("-" * 10)

    def add_outflow_connections(self, source_label: str, outflow_split: List[Tuple[str, float]]):
        """Outflow of `source_label` as (target label, mass fraction) pairs; "EXIT>>" leaves the network.  What is
        left below 1 is the through-flow to the next reactor unless that is listed; a table that lists it (or sums
        to 1 and over) is normalised, as in the reference."""
        if source_label not in self.reactor_map:
            raise ReactorError(f'reactor NOT in the network: "add" reactor {source_label} to the network first')
        idx = self.reactor_map[source_label]
        downstream = idx + 1
        table, total, thruflow, has_exit = [], 0.0, False, False
        for name, frac in outflow_split:
            if name == self._exit_name:
                target, has_exit = self._exit_index, True
            else:
                target = self.reactor_map.get(name, 0)
                if target <= 0:
                    raise ReactorError(f"target reactor {name} is NOT in the network.")
                if target == idx:
                    raise ReactorError(f"outflow connection to self {source_label} is not allowed.")
                thruflow = thruflow or target == downstream
            if frac < 0.0 or frac > 1.0:
                raise ReactorError(f"outflow split fraction to {name} must be >= 0 and <= 1.")
            total += frac
            table.append((target, float(frac)))
        if total > 1.0 + 1e-12:
            raise ReactorError(f"sum of outflow fraction = {total} which is > 1.")
        if idx in self._declared:
            logger.warning("outflow connection exists for %s; the existing connection data will be reset.", source_label)
        self._drop_outlet(idx)
        if not thruflow and total < 1.0 - 1e-12:
            table.append((downstream, 1.0 - total))
        else:
            if total <= 0.0:
                raise ReactorError(f"sum of outflow fraction = {total} which is ~ 0.")
            table = [(t, f / total) for t, f in table]
        self.outflow_targets[idx] = table
        self._declared[idx] = list(table)
        if has_exit:
            self.set_external_outlet(idx)
        self.outflow_altered = True

    def clear_connections(self):
        self.outflow_targets.clear()
        self._declared.clear()
        self.inflow_sources.clear()
        self.outflow_altered = True
        self.external_outlets.clear()
        self.numb_external_outlet = 0

    def remove_reactor(self, name: str):
        """Remove the named reactor and every connection to it.  The reactors behind it move up by one, so that
        indices stay the order of solution; the fractions that went to the removed reactor are not redistributed
        (run() reports a split row that no longer sums to 1)."""
        idx = self.reactor_map.get(name, 0)
        if idx <= 0:
            logger.warning("reactor %s is NOT in the network.", name)
            return

        def moved(i):
            return i if i < idx else i - 1

        self._drop_outlet(idx)
        targets = {}
        for src, table in self._declared.items():
            if src == idx:
                continue
            targets[moved(src)] = [(t if t == self._exit_index else moved(t), f) for t, f in table if t != idx]
        self._declared = targets
        self.outflow_targets = copy.deepcopy(targets)
        self.external_outlets = {k: moved(v) for k, v in self.external_outlets.items()}
        self.tearpoint = [moved(t) for t in self.tearpoint if t != idx]
        self.numb_tearpoints = len(self.tearpoint)
        objs = [r for i, r in sorted(self.reactor_objects.items()) if i != idx]
        self.reactor_objects = {i + 1: r for i, r in enumerate(objs)}
        self.reactor_map = {r.label: i for i, r in self.reactor_objects.items()}
        self.external_connections = {i: r.number_external_inlets for i, r in self.reactor_objects.items()}
        self.numb_reactors = len(objs)
        self.last_reactor = self.numb_reactors
        self.reactor_solutions.clear()
        self.inflow_sources.clear()
        self.outflow_altered = True

    def _drop_outlet(self, reactor_index: int):
        for k in [k for k, v in self.external_outlets.items() if v == reactor_index]:
            del self.external_outlets[k]
        self.external_outlets = {i + 1: v for i, (_, v) in enumerate(sorted(self.external_outlets.items()))}
        self.numb_external_outlet = len(self.external_outlets)

    def set_external_outlet(self, reactor_index: int):
        if reactor_index in self.external_outlets.values():
            return
        self.numb_external_outlet += 1
        self.external_outlets[self.numb_external_outlet] = reactor_index

    def _chain_table(self) -> Dict[int, List[Tuple[int, float]]]:
        """R1 -> R2 -> ... -> EXIT: the network without any declared connection."""
        n = self.numb_reactors
        return {i: [(i + 1, 1.0)] if i < n else [(self._exit_index, 1.0)] for i in range(1, n + 1)}

    @staticmethod
    def _sources(table) -> Dict[int, List[Tuple[int, float]]]:
        src: Dict[int, List[Tuple[int, float]]] = {}
        for i, targets in sorted(table.items()):
            for t, f in targets:
                if t > 0 and f > 0.0:
                    src.setdefault(t, []).append((i, f))
        return src

    def set_reactor_outflow(self):
        """Complete and verify the outflow table: a reactor without declared connections passes everything to the
        next one, the last one to the exit; a through-flow past the last reactor is an exit."""
        n = self.numb_reactors
        if n <= 0:
            raise ReactorError("reactor network contains no reactor.")
        chain = self._chain_table()
        table = {}
        for i in range(1, n + 1):
            row = []
            for t, f in self._declared.get(i, chain[i]):
                row.append((self._exit_index if t > n else t, f))
            table[i] = row
            if any(t == self._exit_index and f > 0.0 for t, f in row):
                self.set_external_outlet(i)
            else:
                self._drop_outlet(i)
        self.outflow_targets = table
        self.set_inflow_connections()
        self.outflow_altered = False

    def set_inflow_connections(self):
        self.inflow_sources = self._sources(self.outflow_targets)

    def split_matrix(self) -> np.ndarray:
        """[R][R + 1]: row j is where reactor j + 1's outflow goes; the last column is the exit."""
        if self.outflow_altered:
            self.set_reactor_outflow()
        n = self.numb_reactors
        S = np.zeros((n, n + 1))
        for i, row in self.outflow_targets.items():
            for t, f in row:
                S[i - 1, n if t == self._exit_index else t - 1] += f
        return S

    # ------------------------------------------------------------------ tear points
    def add_tearingpoint(self, reactor_name: str):
        idx = self.reactor_map.get(reactor_name, 0)
        if idx <= 0:
            raise ReactorError("reactor is NOT in the network.")
        if idx in self.tearpoint:
            raise ReactorError(f"reactor {reactor_name} already declared as a tear point.")
        self.tearpoint.append(idx)
        self.numb_tearpoints += 1

    def remove_tearpoint(self, reactor_name: str):
        idx = self.reactor_map.get(reactor_name, 0)
        if idx <= 0:
            raise ReactorError("reactor is NOT in the network.")
        if idx not in self.tearpoint:
            raise ReactorError("reactor is NOT a tear point.")
        self.tearpoint.remove(idx)
        self.numb_tearpoints -= 1

    def set_tear_tolerance(self, tol: float = 1.0e-6):
        if tol <= 0.0:
            raise ReactorError("tolerance must > 0.")
        self.tolerance = float(tol)

    def set_tear_iteration_limit(self, max_count: int):
        if max_count <= 0:
            raise ReactorError("iteration limit must > 0.")
        self.max_tearloop_count = int(max_count)

    def set_relaxation_factor(self, relax: float):
        if relax <= 0.0:
            raise ReactorError("relaxation factor must > 0.")
        self.relaxation_factor = float(relax)

    # ------------------------------------------------------------------ run
    def _network_inputs(self):
        """The single-network arrays of BatchPSRNetwork.run and the per-position options, from the members."""
        S = self.split_matrix()
        from .batch import BatchPSRNetwork

        try:
            BatchPSRNetwork.check_split(S)
        except ValueError as e:
            raise ReactorError(f"faulty connection configuration: {e}") from None
        n, KK = self.numb_reactors, self.network_chem.KK
        members = [self.reactor_objects[i] for i in range(1, n + 1)]
        E = max(1, max(r.numbexternalinlets for r in members))
        ext_mdot, ext_T, ext_Y = np.zeros((n, E)), np.full((n, E), 300.0), np.zeros((n, E, KK))
        opts = {k: [] for k in ("mode", "energy", "ss_rtol", "ss_atol", "rtol", "atol", "qloss", "htc", "areaq", "tamb",
                                "gfac")}
        P, tau, vol, Tg, Yg = np.zeros(n), np.ones(n), np.ones(n), np.zeros(n), np.zeros((n, KK))
        recycle = any(S[j, i] > 0.0 for j in range(n) for i in range(j + 1))
        est = []
        for i, r in enumerate(members):
            if super(PSR, r).validate_inputs() != 0:   # a member need not have an external inlet of its own
                raise ReactorError(f"reactor {r.label}: required inputs are missing")
            if r.numbexternalinlets <= 0 and not any(S[j, i] > 0.0 for j in range(i)):
                raise ReactorError(f"run failure: reactor {r.label} is not connected to an upstream reactor or inlet")
            for e, s in enumerate(r.externalinlets.values()):
                ext_mdot[i, e], ext_T[i, e], ext_Y[i, e] = s.mass_flowrate, s.temperature, s.Y
            given_tau = r._problemtype == r.ProblemTypes["SETTAU"]
            energy = r._energytype == r.EnergyTypes["ENERGY"]
            ss_atol, ss_rtol = r.steady_state_tolerances
            atol, rtol = r.time_stepping_tolerances
            ss_rtol, ss_atol = min(ss_rtol, 0.1 * self.tolerance), min(ss_atol, 1.0e-9)
            for k, v in (("mode", "residence_time" if given_tau else "volume"), ("energy", "ENERGY" if energy else "TGIV"),
                         ("ss_rtol", ss_rtol), ("ss_atol", ss_atol), ("rtol", min(rtol, ss_rtol)),
                         ("atol", min(atol, ss_atol)), ("qloss", r._heat_loss_rate if energy else 0.0),
                         ("htc", r._heat_transfer_coeff if energy else 0.0),
                         ("areaq", r._heat_transfer_area if energy else 0.0), ("tamb", r._ambient_temperature),
                         ("gfac", r._gasratemultiplier)):
                opts[k].append(v)
            P[i] = r.reactormixture.pressure
            tau[i], vol[i] = (r._restime, 1.0) if given_tau else (1.0, r._volume)
            Tg[i] = r.reactormixture.temperature
            Yg[i] = r.reactormixture.Y if r._estimate_Y is None else r._estimate_Y
            # run_without_tearstream: a reactor fed from inside the network starts from its inlet's composition
            internal = any(S[j, i] > 0.0 for j in range(n))
            est.append("inlet" if (self.numb_tearpoints == 0 and not recycle and internal) else "given")
        tear = np.zeros(n, np.int32)
        for t in self.tearpoint:
            tear[t - 1] = 1
        return dict(S=S, ext_mdot=ext_mdot, ext_T=ext_T, ext_Y=ext_Y, opts=opts, P=P, tau=tau, vol=vol, Tg=Tg, Yg=Yg,
                    est=est, tear=tear)

    def run(self) -> int:
        """Solve the network.  Returns 0, 10 when the tear iteration limit was reached, or the failed reactor's
        status; ``self.result`` keeps the NetworkResult (sweeps, tear residual, statistics)."""
        from .batch import BatchPSRNetwork

        a = self._network_inputs()
        n = self.numb_reactors
        batch = BatchPSRNetwork(self.network_chem, n, max_sweeps=self.max_tearloop_count, tear_rtol=self.tolerance,
                                tear_atol=1.0e-8, relax=self.relaxation_factor, **a["opts"])
        res = batch.run(a["P"], a["S"], a["ext_mdot"], a["ext_T"], ext_Y=a["ext_Y"], tau=a["tau"], volume=a["vol"],
                        estimate=a["est"], T_estimate=a["Tg"], Y_estimate=a["Yg"], tear=a["tear"])
        self.result = res
        status = int(res.status[0])
        self.tear_converged = status == 0
        self.reactor_solutions.clear()
        for i in range(1, n + 1):
            r = self.reactor_objects[i]
            code = int(res.reactor_status[0, i - 1])
            solved = np.isfinite(res.T[0, i - 1])
            r.setrunstatus(code if solved else -100)
            if solved and code == 0:
                out = Stream(self.network_chem, label=r.label + "_exit")
                out.pressure = float(res.P[0, i - 1])
                out.temperature = float(res.T[0, i - 1])
                out.Y = np.maximum(res.Y[0, i - 1], 0.0)
                out.volume = float(res.volume[0, i - 1])
                out.mass_flowrate = float(res.mdot[0, i - 1])
                self.reactor_solutions[i] = out
        if status == 12:
            raise ReactorError("the flow balance of the network has no solution: a closed loop with no exit, or a "
                               "reactor nothing flows through")
        if status == 11:
            bad = [i for i in range(1, n + 1) if self.reactor_objects[i].runstatus not in (0, -100)]
            code = self.reactor_objects[bad[0]].runstatus if bad else 11
            logger.error("run failure: reactor %s, error code = %s", self.get_reactor_label(bad[0]) if bad else "?", code)
            self.network_run_status = code
            return code
        if status == 10:
            logger.error("failure to solve the reactor network: max tear iteration count reached %d, "
                         "max tear loop residual = %.3e", self.max_tearloop_count, float(res.tear_resid[0]))
            self.network_run_status = 10
            return 10
        self.network_run_status = 0
        self.set_external_streams()
        return 0

    def get_network_run_status(self) -> int:
        """0 = solved; -100 = not run; other = failed."""
        return self.network_run_status

    def _need_solution(self):
        if self.get_network_run_status() != 0:
            raise ReactorError("reactor network has NOT been solved successfully: adjust reactor parameters and rerun")

    def get_reactor_stream(self, reactor_name: str) -> Stream:
        self._need_solution()
        idx = self.reactor_map.get(reactor_name, 0)
        if idx == 0:
            raise ReactorError(f"reactor {reactor_name} is NOT found in the network.")
        return self.reactor_solutions[idx]

    def set_external_streams(self):
        self.external_outlet_streams.clear()
        for ioutlet, nrxtor in self.external_outlets.items():
            frac = 1.0
            for t, f in self.outflow_targets.get(nrxtor, []):
                if t == self._exit_index:
                    frac = f
            out = copy.deepcopy(self.reactor_solutions[nrxtor])
            out.mass_flowrate = out.mass_flowrate * frac
            self.external_outlet_streams[ioutlet] = out

    def get_external_stream(self, stream_index: int) -> Stream:
        if self.numb_external_outlet <= 0:
            raise ReactorError("no external outlet defined.")
        self._need_solution()
        if stream_index not in self.external_outlet_streams:
            raise ReactorError(f"external outlet {stream_index} does not exist")
        return self.external_outlet_streams[stream_index]
