"""The reference's module of this name scores secondary structure by writing a PDB and running P-SEA on the host; here the control is
the differentiable SecStructPotential (genie2_amd/smc.py, csrc/secstruct_kernels.hip) and its blueprint reader."""
from genie2_amd.smc import SecStructPotential, load_ss_target, ss_string, ss_target_windows  # noqa: F401
