// ed_chi.hpp — device kernels of the spin and density susceptibilities of the
// kept states (buildChi_impurity, ED_GREENS_FUNCTIONS.f90:72-106; DESIGN.md
// section 12).
//
//   k_seed_diag   every seed O_q |vec> of one kept state for operators O_q
//                 diagonal in the Fock basis (Sz_a, n_a and sums of them: the
//                 vvinit loops ED_GF_CHISPIN.f90:98-103 and
//                 ED_GF_CHISPIN.f90:194-199) in one pass: the gather form of
//                 k_seed_plan without the gather.  One thread per row
//                 (grid-strided); map[r] and vec[r] are read once, the
//                 occupations of the call's levels are taken once per row and
//                 every seed is that row's factor (seed_diag_factor: its
//                 weights of the occupied levels, added in level order) times
//                 vec[r].  Every output row is written whole with coalesced
//                 stores at stride dim: no memset.  Each block leaves one
//                 partial of sum |seed_q|^2 per seed (block_partial);
//                 k_seed_scale (ed_seed.hpp) finishes as for the other seeds.
//   k_seed_pair   every seed of one kept state whose images are products of
//                 two ladder operators (the pair seeds ED_GF_CHIPAIR.f90:98-102
//                 and :144-148, the inter-orbital density seeds
//                 ED_GF_CHIDENS.f90:523-586 and :596-659; DESIGN.md section
//                 13): the gather form of k_seed_plan with seed_image2
//                 (ed_seed_pair.hpp) in place of seed_image.
// (k_chi_poles, the pole sums of add_to_lanczos_spinChi, is in ed_poles.hip,
// the unit that launches it.)
#pragma once
#include "ed_chi_host.hpp"
#include "ed_seed.hpp"  // seed_abs2, k_seed_scale
#include "ed_seed_pair.hpp"

namespace edg {

static_assert(kDiagMaxLev == kSeedMaxLev && kDiagMaxSeeds == kSeedMaxSeeds, "one set of seed limits");

// seeds: [T.nseed][dim] (unnormalised on exit); partials: [T.nseed][gridDim.x].
// The table is the same in every lane (scalar loads); the occupations b[] and
// the sums n2[] are only ever indexed by unrolled loop counters, so they stay
// in registers.
template <bool VC>
__global__ void __launch_bounds__(kBlock) k_seed_diag(const uint32_t* __restrict__ map, int64_t dim, DiagTable T,
                                                      const val_t<VC>* __restrict__ x,
                                                      val_t<VC>* __restrict__ seeds,
                                                      double* __restrict__ partials) {
  using V = val_t<VC>;
  double n2[kDiagMaxSeeds];
#pragma unroll
  for (int q = 0; q < kDiagMaxSeeds; q++) n2[q] = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < dim; r += (int64_t)gridDim.x * kBlock) {
    const uint32_t t = map[r];
    const V v = x[r];
    double b[kDiagMaxLev];
#pragma unroll
    for (int l = 0; l < kDiagMaxLev; l++) b[l] = l < T.nlev ? (double)bit(t, T.lev[l]) : 0.0;
#pragma unroll
    for (int q = 0; q < kDiagMaxSeeds; q++) {
      if (q < T.nseed) {
        const V a = scl(seed_diag_factor(T.w[q], b), v);
        seeds[(size_t)q * dim + r] = a;
        n2[q] += seed_abs2(a);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kDiagMaxSeeds; q++)
    if (q < T.nseed) block_partial(n2[q], partials + (size_t)q * gridDim.x);
}

// seeds: [P.nseed][dim] (unnormalised on exit); partials: [P.nseed][gridDim.x].
// The host has checked (seed_pair_compile) that every image maps src into dst,
// so every source state of a hit lies in idx_src's tables; a miss looks
// nothing up.  u_l = (sign1 * sign2) * v_l is what k_apply_op into the
// intermediate sector followed by k_apply_op_acc with coefficient 1 leaves
// (both signs are +-1: the products are exact), u_p + u_q what the second
// chain adds.  The plan is the same in every lane; images and sums are only
// ever indexed by unrolled counters (see k_seed_plan for the opaque zero).
template <bool VC>
__global__ void __launch_bounds__(kBlock) k_seed_pair(const uint32_t* __restrict__ map_dst, int64_t dim,
                                                      DevIndex idx_src, PairPlan P,
                                                      const val_t<VC>* __restrict__ x,
                                                      val_t<VC>* __restrict__ seeds,
                                                      double* __restrict__ partials) {
  using V = val_t<VC>;
  double n2[kPairMaxSeeds];
#pragma unroll
  for (int s = 0; s < kPairMaxSeeds; s++) n2[s] = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < dim; r += (int64_t)gridDim.x * kBlock) {
    const uint32_t t = map_dst[r];
    V u[kPairMaxImg];
#pragma unroll
    for (int l = 0; l < kPairMaxImg; l++) {
      u[l] = vzero<V>();
      if (l < P.nimg) {
        uint32_t s;
        double sg;
        if (seed_image2(t, P.img[l], &s, &sg)) u[l] = scl(sg, x[idx_src(s)]);
      }
    }
    int z = 0;
    asm volatile("" : "+s"(z));
#pragma unroll
    for (int s = 0; s < kPairMaxSeeds; s++) {
      if (s < P.nseed) {
        V a = vzero<V>(), b = vzero<V>();
#pragma unroll
        for (int l = 0; l < kPairMaxImg; l++) {
          if (P.p[s] == l + z) a = u[l];
          if (P.q[s] == l + z) b = u[l];
        }
        if (P.q[s] != kSeedNone) a = add(a, b);
        seeds[(size_t)s * dim + r] = a;
        n2[s] += seed_abs2(a);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < kPairMaxSeeds; s++)
    if (s < P.nseed) block_partial(n2[s], partials + (size_t)s * gridDim.x);
}

}  // namespace edg
