"""Not in the reference: binder guidance against a fixed target given as C-alpha coordinates (contacts, hotspot coverage, clashes),
the differentiable BinderPotential (genie2_amd/smc.py, csrc/binder_kernels.hip) with its target helpers, beside the symmetry guidance
of genie/sampler/symmetry.py."""
from genie2_amd.smc import BinderPotential, load_target, parse_hotspots, place_target  # noqa: F401
