"""Not in the reference: symmetry guidance for cyclic and dihedral oligomers, closed toroids and open repeats, the differentiable
SymmetryPotential (genie2_amd/smc.py, csrc/symmetry_kernels.hip) with its layout helpers, beside the strand pairing of
genie/sampler/sheet.py."""
from genie2_amd.smc import SymmetryPotential, check_generators, partner_table, symmetry_generators, symmetry_layout  # noqa: F401
