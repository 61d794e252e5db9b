"""Steady-state stirred reactors (reference stirreactors/): batched PSRs on the wave-per-reactor kernel.

``stirreactors.openreactor`` and ``stirreactors.PSR`` are the reference's module names; the PSR models are
re-exported here."""
from . import openreactor  # noqa: F401  (the module: stirreactors.openreactor.openreactor is the class)
from .PSR import (PSR_SetResTime_EnergyConservation, PSR_SetResTime_FixedTemperature,
                  PSR_SetVolume_EnergyConservation, PSR_SetVolume_FixedTemperature, perfectlystirredreactor)

__all__ = ["perfectlystirredreactor", "PSR_SetResTime_EnergyConservation", "PSR_SetVolume_EnergyConservation",
           "PSR_SetResTime_FixedTemperature", "PSR_SetVolume_FixedTemperature"]
