"""Not in the reference: burial guidance by the half-sphere exposure of the C-alpha chain (which residues lie inside the design and
which on its surface), the differentiable BurialPotential (genie2_amd/smc.py, csrc/burial_kernels.hip) with its helpers, beside the
diversity guidance of genie/sampler/diversity.py."""
from genie2_amd.smc import BurialPotential, check_burial_targets, load_burial_targets, parse_residue_ranges  # noqa: F401
