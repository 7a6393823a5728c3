"""`genjax.inference.smc` (reference: src/genjax/inference/smc.py:15-27 exports ChangeTarget,
Importance, ImportanceK, SMCAlgorithm), plus what the north star adds on top of the reference:
`ParticleCollection.resample` and the fused bootstrap-SMC driver."""

from .._amd.inference import (ChangeTarget, Importance, ImportanceK, ParticleCollection, SMCAlgorithm,
                              stack_to_first_dim)
from .._amd.smc_fused import (BootstrapSMC, DiscreteHMM, GuidedSMC, LinearGaussianSSM, ParticleGibbs, ParticleGibbsResult,
                              ParticleMH, SMCResult, StateSpaceModel, Trajectories)
from .._amd.temper import PSISLOO, PointwiseLikelihood, PosteriorPredictive, TemperedResult, TemperedSMC

__all__ = ["ChangeTarget", "Importance", "ImportanceK", "SMCAlgorithm", "ParticleCollection", "BootstrapSMC", "GuidedSMC",
           "LinearGaussianSSM", "DiscreteHMM", "StateSpaceModel", "SMCResult", "Trajectories", "stack_to_first_dim", "ParticleMH",
           "ParticleGibbs", "ParticleGibbsResult", "TemperedSMC", "TemperedResult",
           "PointwiseLikelihood", "PosteriorPredictive", "PSISLOO"]
