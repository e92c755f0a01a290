"""Not in the reference: fold guidance towards a template backbone or away from known ones by TM-score, the differentiable
FoldPotential (genie2_amd/smc.py, csrc/fold_kernels.hip) for references of the design's own length and AlignedFoldPotential
(csrc/fold_align_kernels.hip) for references of any length under gapped alignment, beside the binder guidance of
genie/sampler/binder.py."""
from genie2_amd.smc import AlignedFoldPotential, FoldPotential, check_fold_bounds  # noqa: F401
