"""Not in the reference: diversity guidance inside one run, the differentiable DiversityPotential (genie2_amd/smc.py,
csrc/diversity_kernels.hip) that makes the particle systems of one device batch repel each other by TM-score, beside the fold guidance
of genie/sampler/fold.py."""
from genie2_amd.smc import DiversityPotential  # noqa: F401
