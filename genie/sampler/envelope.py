"""Not in the reference: envelope guidance (the design stays inside a given 3D shape -- a solid, an existing protein, the pseudo-atoms
of a low-resolution map -- and fills it), the differentiable EnvelopePotential (genie2_amd/smc.py, csrc/envelope_kernels.hip) with its
helpers, beside the burial guidance of genie/sampler/burial.py."""
from genie2_amd.smc import EnvelopePotential, envelope_shape_points, load_envelope  # noqa: F401
