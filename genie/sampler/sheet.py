"""Not in the reference: strand-pairing guidance, the differentiable SheetPotential (genie2_amd/smc.py, csrc/sheet_kernels.hip) with its
ladder reader, beside the secondary-structure control of genie/sampler/secstruct.py."""
from genie2_amd.smc import SheetPotential, check_ladder, ladder_table, load_ladder  # noqa: F401
