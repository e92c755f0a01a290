"""Not in the reference: context guidance, a binding partner given as C-alpha coordinates that follows each particle's placement of the
motif (clashes, contacts), the differentiable ContextPotential (genie2_amd/smc.py, csrc/context_kernels.hip), beside the binder
guidance of genie/sampler/binder.py."""
from genie2_amd.smc import ContextPotential, load_target  # noqa: F401
