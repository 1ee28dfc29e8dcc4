// ed_sigma.hpp — device kernel of the self-energy and the Weiss field
// (build_sigma_normal, ED_GF_NORMAL.f90:656-731; build_sigma_superc,
// ED_GF_SUPERC.f90:826-929; build_sigma_nonsu2, from ED_GF_NONSU2.f90:977;
// DESIGN.md section 14).
//
//   k_sigma<N>   one work item per (block, grid point): blockIdx.y is the
//                block, the Matsubara and the real grid are laid end to end
//                along x as in k_chi_poles.  A block of another size leaves at
//                once, so one launch per distinct N covers a mixed list.  The
//                block's table (one-body matrix, poles) is read through a
//                wave-uniform pointer; the N x N matrix of sigma_point<N>
//                (ed_sigma_host.hpp) lives in registers: every index is an
//                unrolled counter and the pivot moves by selects.
#pragma once
#include <hip/hip_runtime.h>

#include "ed_sigma_host.hpp"

namespace edg {

constexpr int kSigBlock = 64;  // one wave: about 10^4 points spread over the CUs

template <int N>
__global__ void __launch_bounds__(kSigBlock) k_sigma(const SigmaBlock* __restrict__ blocks, SigmaArrays A,
                                                     double beta, int lmats, double wini, double wfin, int lreal,
                                                     double eps, int with_g) {
  const SigmaBlock& B = blocks[blockIdx.y];
  if (B.n != N) return;
  const int t = blockIdx.x * kSigBlock + threadIdx.x;
  if (t >= lmats + lreal) return;
  sigma_item<N>(B, A, t, beta, lmats, wini, wfin, lreal, eps, with_g != 0);
}

}  // namespace edg
