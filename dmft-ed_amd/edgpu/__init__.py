"""edgpu — MI355X-native Lanczos H·v hot path of dmft-ed (host mirror).

Modules:
  params      EDConfig / bath initialisation / the ed_params C struct
  sectors     symmetry-sector tables (setup_pointers_*)
  hamiltonian Sector handle + build_Hv_sector / spHtimesV_cc mirror; its
              lanc_eigh / lanc_tridiag / eigh methods are the device
              sp_lanc_eigh / sp_lanc_tridiag / sp_eigh replacements
  diag        ed_diag sector loop (single GPU) and the T=0 state list
  farm        sector farm over ranks (torch.distributed / RCCL)
  gf          Green's functions (normal, nonSU2, superc): device seeds
              (Sector.seed_batch / seed_plan when fused), Lanczos, poles;
              seed_fractions, the one path from a seed call to the queued
              fractions, which chi uses too
  chi         spin and density susceptibilities of the kept states: diagonal
              seeds (Sector.seed_diag), Lanczos, bosonic / tau / real-axis poles;
              pair and inter-orbital parts from two-operator seeds
              (Sector.seed_pair)
  sigma       self-energy, Weiss field and bath hybridisation from G (and F):
              ed_sigma_build, one work item per (block, grid point)
  observables impurity observables and local energies of the kept states
              (observables_impurity / local_energy_impurity) from device
              vectors: Sector.nn_moments / Sector.expect
  dist        one sector over ranks (row split + Allgatherv; Kronecker all-to-all)

Importing this package does not touch the GPU; the HIP library is loaded on
first use and its absence is an error (no CPU fallback).
"""
from .params import EDConfig, make_config, init_dmft_bath, random_bath  # noqa: F401
from .sectors import setup_pointers  # noqa: F401
from .chi import Chi, ChiOptions, build_chi  # noqa: F401
from .sigma import Sigma, bath_functions, build_sigma  # noqa: F401

__all__ = ["EDConfig", "make_config", "init_dmft_bath", "random_bath", "setup_pointers", "Chi", "ChiOptions",
           "build_chi", "Sigma", "build_sigma", "bath_functions"]
