"""Generic open (steady-state, flow-through) reactor: external inlets and the steady-state solver controls
(drop-in for the reference's stirreactors/openreactor.py).

The GPU solves a PSR with ONE effective inlet (include/ckmi.h ckmi_psr_run), so several external inlets
are mixed on the host first: mass flow rates add, mass fractions mix by mass, and the inlet temperature
is the one that conserves the total enthalpy -- the constant-enthalpy mixing of
``mixture.adiabatic_mixing``, evaluated here from the mechanism's NASA-7 tables on the host and iterated
to convergence (adiabatic_mixing stops within 0.1 K and needs a GPU for the species enthalpies), so that a
reactor fed by two streams equals the one fed by their premixed stream.
"""
from __future__ import annotations

import copy
from typing import Dict, Optional, Tuple

import numpy as np

from ..constants import R_GAS
from ..inlet import Stream
from ..logger import logger
from ..mixture import Mixture
from ..reactormodel import Keyword, ReactorError, ReactorModel
from ..steadystatesolver import SteadyStateSolver


def _nasa7_h_cp(thermo: np.ndarray, wt: np.ndarray, T: float) -> Tuple[np.ndarray, np.ndarray]:
    """Species enthalpy [erg/g] and cp [erg/(g K)] at T from the [KK][17] NASA-7 table of the mechanism
    (columns 1: T_mid, 3..9: low range, 10..16: high range)."""
    a = np.where((T > thermo[:, 1])[:, None], thermo[:, 10:17], thermo[:, 3:10])
    cpR = a[:, 0] + T * (a[:, 1] + T * (a[:, 2] + T * (a[:, 3] + T * a[:, 4])))
    hRT = a[:, 0] + T * (a[:, 1] / 2 + T * (a[:, 2] / 3 + T * (a[:, 3] / 4 + T * a[:, 4] / 5))) + a[:, 5] / T
    return hRT * R_GAS * T / wt, cpR * R_GAS / wt


def mix_streams(chem, streams) -> Tuple[float, np.ndarray, float]:
    """The one effective inlet (T [K], Y, mdot [g/s]) of several streams: mass flow rates add, Y mixes by
    mass, T conserves the total enthalpy sum_i mdot_i h_i(T_i).  A single stream is returned as it is."""
    streams = list(streams)
    if not streams:
        raise ReactorError("the reactor has no inlet")
    md = np.array([s.mass_flowrate for s in streams])
    if len(streams) == 1:
        return float(streams[0].temperature), np.array(streams[0].Y), float(md[0])
    tables = chem.mechanism.to_tables()
    thermo, wt = np.asarray(tables["thermo"], dtype=np.float64), np.asarray(tables["wt"], dtype=np.float64)
    mdot = float(md.sum())
    Y = sum(m * s.Y for m, s in zip(md, streams)) / mdot
    H = sum(m * float(np.dot(s.Y, _nasa7_h_cp(thermo, wt, s.temperature)[0])) for m, s in zip(md, streams)) / mdot
    T = float(sum(m * s.temperature for m, s in zip(md, streams)) / mdot)
    for _ in range(100):
        h, cp = _nasa7_h_cp(thermo, wt, T)
        dT = (H - float(np.dot(Y, h))) / float(np.dot(Y, cp))
        T += dT
        if abs(dT) <= 1e-10 * T:
            return T, Y, mdot
    raise ReactorError("the mixed inlet temperature did not converge")


class openreactor(ReactorModel, SteadyStateSolver):
    """Generic open reactor model (reference openreactor.py:38-298)."""

    def __init__(self, guessedmixture: Stream, label: Optional[str] = None):
        if not isinstance(guessedmixture, Mixture):
            raise ReactorError("the first argument must be a Mixture object")
        ReactorModel.__init__(self, reactor_condition=guessedmixture, label=label if label is not None else "Reactor")
        SteadyStateSolver.__init__(self)
        Keyword.noFullKeyword = True
        self.numbexternalinlets = 0
        self.externalinlets: Dict[str, Stream] = {}
        self.totalmassflowrate = 0.0
        self.SolverTypes = {"Transient": 1, "SteadyState": 2}
        self.EnergyTypes = {"ENERGY": 1, "GivenT": 2}
        self.ProblemTypes = {"SETVOL": 1, "SETTAU": 2}

    # ------------------------------------------------------------------ inlets
    def set_inlet(self, extinlet: Stream):
        """Connect an external inlet (a Stream with a flow rate) to the reactor."""
        if not isinstance(extinlet, Stream):
            raise ReactorError("the argument must be a Stream object")
        count = self.numbexternalinlets + 1
        name = f"{self.label}_inlet_{count}" if extinlet.label is None else f"{self.label}_{extinlet.label}"
        if name in self.externalinlets:
            name += "_dup"
            logger.info("inlet already connected; the new inlet name is %s", name)
        if extinlet._flowratemode < 0:
            raise ReactorError("inlet flow rate is not set: specify the flow rate of the Stream object")
        flowrate = extinlet.mass_flowrate
        if flowrate <= 0.0:
            raise ReactorError("inlet flow rate must be > 0")
        self.externalinlets[name] = extinlet
        self.numbexternalinlets = count
        self.totalmassflowrate += flowrate
        logger.info("new inlet %s is added", name)

    def reset_inlet(self, new_stream: Stream):
        """Replace the properties of the connected inlet that has new_stream's label."""
        if not isinstance(new_stream, Stream):
            raise ReactorError("the argument must be a Stream")
        name = f"{self.label}_{new_stream.label}"
        if name not in self.externalinlets:
            raise ReactorError(f"inlet {new_stream.label} is not found")
        self.totalmassflowrate += new_stream.mass_flowrate - self.externalinlets[name].mass_flowrate
        self.externalinlets[name] = copy.deepcopy(new_stream)

    def remove_inlet(self, name: str):
        """Disconnect the inlet with this label."""
        if not isinstance(name, str):
            raise ReactorError("the argument must be a string")
        inlet = self.externalinlets.pop(f"{self.label}_{name}", None)
        if inlet is None:
            raise ReactorError(f"inlet {name} is not found")
        self.numbexternalinlets -= 1
        self.totalmassflowrate -= inlet.mass_flowrate
        logger.info("inlet %s is removed from reactor %s", name, self.label)

    @property
    def net_mass_flowrate(self) -> float:
        """Total external mass flow rate into the reactor [g/s]."""
        return self.totalmassflowrate

    @property
    def net_vol_flowrate(self) -> float:
        """Total external volumetric flow rate into the reactor [cm3/s]."""
        return float(sum(s.vol_flowrate for s in self.externalinlets.values()))

    @property
    def number_external_inlets(self) -> int:
        return self.numbexternalinlets

    def effective_inlet(self) -> Tuple[float, np.ndarray, float]:
        """(T [K], Y, mdot [g/s]) of the connected inlets mixed into one (mix_streams)."""
        return mix_streams(self._chem, self.externalinlets.values())
