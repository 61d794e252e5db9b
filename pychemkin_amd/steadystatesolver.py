"""Steady-state solver controls of the open reactors (drop-in for the reference's steadystatesolver.py).

The reference's steady-state reactors are solved by TWOPNT: a damped Newton search that falls back to
pseudo time stepping.  Here a PSR is solved on the GPU by marching its transient equations with the
variable-order BDF integrator until a steady-state rule on the right-hand side is met
(include/ckmi.h ckmi_psr_run), so only two pairs of controls have an effect:

  steady_state_tolerances   (atol, rtol) -> ss_atol, ss_rtol of the steady-state rule
                            tau |f_k| <= ss_rtol |Y_k| + ss_atol, tau |f_T| <= ss_rtol T
  time_stepping_tolerances  (atol, rtol) -> the time integrator's atol, rtol
                            (``timestepping_tolerances``, as the reference's own PSR test spells it,
                            is the same property)

Every TWOPNT tuning setter (iteration limits, Jacobian ages, damping, species floor, pseudo time step
sizes, ...) is accepted with the reference's signature and recorded in ``SSsolverkeywords``, and has
NO effect on this solver.
"""
from __future__ import annotations

from typing import Dict, Tuple, Union

from .logger import logger
from .reactormodel import ReactorError


class SteadyStateSolver:
    """Steady-state solver parameters (reference steadystatesolver.py:35-483)."""

    def __init__(self):
        # the steady-state rule (reference defaults 1e-9 / 1e-4)
        self.SSabsolute_tolerance = 1.0e-9
        self.SSrelative_tolerance = 1.0e-4
        # the time integrator
        self.TRabsolute_tolerance = 1.0e-9
        self.TRrelative_tolerance = 1.0e-4
        # recorded only (no effect on this solver)
        self.SSmaxiteration = 100
        self.SSJacobianage = 20
        self.maxpseudotransient = 100
        self.numbinitialpseudosteps = 0
        self.maxTbound = 5000.0
        self.speciesfloor = -1.0e-14
        self.species_positive = 0.0
        self.use_legacy_technique = False
        self.SSdamping = 1
        self.TRmaxiteration = 25
        self.timestepsizeage = 25
        self.TRminstepsize = 1.0e-10
        self.TRmaxstepsize = 1.0e-2
        self.TRJacobianage = 20
        self.print_level = 1
        self.SSsolverkeywords: Dict[str, Union[int, float, str, bool]] = {}

    # ------------------------------------------------------------------ tolerances (effective)
    @staticmethod
    def _pair(tolerances) -> Tuple[float, float]:
        a, r = float(tolerances[0]), float(tolerances[1])
        if not (a > 0.0 and r > 0.0):
            raise ReactorError("tolerances must be > 0")
        return a, r

    @property
    def steady_state_tolerances(self) -> Tuple[float, float]:
        """(absolute, relative) tolerance of the steady-state rule."""
        return (self.SSabsolute_tolerance, self.SSrelative_tolerance)

    @steady_state_tolerances.setter
    def steady_state_tolerances(self, tolerances: Tuple[float, float]):
        self.SSabsolute_tolerance, self.SSrelative_tolerance = self._pair(tolerances)
        self.SSsolverkeywords["ATOL"] = self.SSabsolute_tolerance
        self.SSsolverkeywords["RTOL"] = self.SSrelative_tolerance

    @property
    def time_stepping_tolerances(self) -> Tuple[float, float]:
        """(absolute, relative) tolerance of the time integrator."""
        return (self.TRabsolute_tolerance, self.TRrelative_tolerance)

    @time_stepping_tolerances.setter
    def time_stepping_tolerances(self, tolerances: Tuple[float, float]):
        self.TRabsolute_tolerance, self.TRrelative_tolerance = self._pair(tolerances)
        self.SSsolverkeywords["ATIM"] = self.TRabsolute_tolerance
        self.SSsolverkeywords["RTIM"] = self.TRrelative_tolerance

    # the spelling the reference's PSRgas test uses
    timestepping_tolerances = time_stepping_tolerances

    # ------------------------------------------------------------------ TWOPNT tuning (recorded, no effect)
    def _record(self, key: str, value, what: str) -> None:
        self.SSsolverkeywords[key] = value
        logger.debug("%s is recorded (%s = %s) and has no effect on the time-marching PSR solver", what, key, value)

    def set_max_pseudo_transient_call(self, maxtime: int):
        """Recorded; no effect on this solver."""
        self.maxpseudotransient = int(maxtime)
        self._record("MAXTIME", int(maxtime), "max pseudo transient calls")

    def set_max_timestep_iteration(self, maxiteration: int):
        """Recorded; no effect on this solver."""
        self.TRmaxiteration = int(maxiteration)
        self._record("TRMAXITER", int(maxiteration), "max iterations per pseudo time step")

    def set_max_search_iteration(self, maxiteration: int):
        """Recorded; no effect on this solver."""
        self.SSmaxiteration = int(maxiteration)
        self._record("SSMAXITER", int(maxiteration), "max iterations per steady-state search")

    def set_initial_timesteps(self, initsteps: int):
        """Recorded; no effect on this solver."""
        self.numbinitialpseudosteps = int(initsteps)
        self._record("ISTP", int(initsteps), "initial pseudo time steps")

    def set_species_floor(self, floor_value: float):
        """Recorded; no effect on this solver."""
        self.speciesfloor = float(floor_value)
        self._record("SFLR", float(floor_value), "species floor")

    def set_temperature_ceiling(self, ceilingvalue: float):
        """Recorded; no effect on this solver."""
        self.maxTbound = float(ceilingvalue)
        self._record("TBND", float(ceilingvalue), "temperature ceiling")

    def set_species_reset_value(self, resetvalue: float):
        """Recorded; no effect on this solver."""
        self.species_positive = float(resetvalue)
        self._record("SPOS", float(resetvalue), "species reset value")

    def set_max_pseudo_timestep_size(self, dtmax: float):
        """Recorded; no effect on this solver."""
        self.TRmaxstepsize = float(dtmax)
        self._record("DTMX", float(dtmax), "max pseudo time step size")

    def set_min_pseudo_timestep_size(self, dtmin: float):
        """Recorded; no effect on this solver."""
        self.TRminstepsize = float(dtmin)
        self._record("DTMN", float(dtmin), "min pseudo time step size")

    def set_pseudo_timestep_age(self, age: int):
        """Recorded; no effect on this solver."""
        self.timestepsizeage = int(age)
        self._record("IRET", int(age), "pseudo time step age")

    def set_Jacobian_age(self, age: int):
        """Recorded; no effect on this solver."""
        self.SSJacobianage = int(age)
        self._record("NJAC", int(age), "steady-state Jacobian age")

    def set_pseudo_Jacobian_age(self, age: int):
        """Recorded; no effect on this solver."""
        self.TRJacobianage = int(age)
        self._record("TJAC", int(age), "pseudo time stepping Jacobian age")

    def set_damping_option(self, ON: bool):
        """Recorded; no effect on this solver."""
        self.SSdamping = 1 if ON else 0
        self._record("TWOPNT_DAMPING", self.SSdamping, "damping option")

    def set_legacy_option(self, ON: bool):
        """Recorded; no effect on this solver."""
        self.use_legacy_technique = bool(ON)
        self._record("LEGACY", bool(ON), "legacy technique")

    def set_print_level(self, level: int):
        """Recorded; no effect on this solver."""
        self.print_level = int(level)
        self._record("PRNT", int(level), "print level")

    def set_pseudo_timestepping_parameters(self, numb_steps: int = 100, step_size: float = 1.0e-6, stage: int = 1):
        """Recorded; no effect on this solver.  stage: 1 fixed temperature, 2 energy equation."""
        if stage not in (1, 2):
            raise ReactorError("the stage must be either 1 or 2")
        self._record(f"TIM{stage}", (int(numb_steps), float(step_size)), "pseudo time stepping parameters")
