// ed_seed.hpp — the Green's-function seeds of one (kept state, operator type,
// target sector) group in one pass (ed_sector_seed_batch).
//
// The reference builds every seed with its own vvinit loop over the source
// sector (ED_GF_NORMAL.f90:159-174 one term, :312-344 two terms): bdecomp,
// c / cdg, binary_search on the target map, then dot_product and the divide
// by sqrt(norm2).  k_apply_op / k_apply_op_acc restate that loop one term at
// a time (scatter form: a memset, and one read of the state vector and the
// source map per term).  With orbital off-diagonal components a group holds
// Norb^2 seeds of the same operator type into the same target sector, all of
// them linear combinations of the same <= 2*Norb single-level images
//   s_l = op_{level_l} |src_vec>.
//
//   k_seed_gather  gather form: one thread per TARGET row r (grid-strided, as
//                  k_twin_gather).  t = map_dst[r]; level l hits iff bit l of
//                  t is set (c^+) or clear (c); the source state is
//                  t ^ (1 << l), its row comes from src's index tables, the
//                  sign is jw_sign (the bits below l are the same in both
//                  states).  The nlev images are formed once per row and
//                  every seed is their combination in level order — for a
//                  coefficient 1 followed by coef * second that is the
//                  arithmetic of the k_apply_op + k_apply_op_acc chain, bit
//                  for bit.  Every output row is written whole with coalesced
//                  stores at stride dim: no memset, no read-modify-write.
//                  Each block leaves one partial of sum |seed_q|^2 per seed
//                  (block_partial: wave sum, then LDS across the 4 waves).
//   k_seed_scale   every block sums its seed's partials in fixed order
//                  (sum_partials) and scales its rows by 1/sqrt(norm2); a
//                  seed with norm2 == 0 stays all zero.  Block 0 of a seed
//                  stores norm2.  No floating-point atomics: two calls on the
//                  same input give the same bits.
//   k_seed_plan    the same gather form for groups whose images mix operator
//                  types (ed_sector_seed_plan; the superconducting seeds of
//                  ED_GF_SUPERC.f90:119-439): image l is op_l on level_l
//                  (seed_image, ed_seed_plan.hpp), a seed is image p or image
//                  p + image q with unit coefficients.  The kernel argument is
//                  a SeedPlan of about 90 bytes instead of SeedTable's 3 KB.
#pragma once
#include "ed_kernels.hpp"
#include "ed_seed_plan.hpp"  // kSeedMaxLev, kSeedMaxSeeds, SeedPlan, seed_image

namespace edg {

// Levels and coefficients: a kernel argument, the same in every lane (scalar
// loads).  A coefficient (0, 0) means the level is not part of the seed.
// The compiler loads the whole table ahead of the row loop and keeps what
// does not fit the SGPR file in VGPR lanes (no scratch); a device block read
// inside the loop was no faster.
struct SeedTable {
  int32_t nlev, nseed;
  int32_t lev[kSeedMaxLev];
  uint8_t used[kSeedMaxSeeds];  // bit l: coefficient l of the seed is not (0, 0)
  double cr[kSeedMaxSeeds][kSeedMaxLev];
  double ci[kSeedMaxSeeds][kSeedMaxLev];
};

__device__ __forceinline__ double seed_abs2(double a) { return a * a; }
__device__ __forceinline__ double seed_abs2(double2 a) { return a.x * a.x + a.y * a.y; }

// acc + coef * (sg * v), written as k_apply_op_acc writes it.
__device__ __forceinline__ double seed_add(double acc, double cr, double, double sg, double v) {
  return acc + cr * (sg * v);
}
__device__ __forceinline__ double2 seed_add(double2 acc, double cr, double ci, double sg, double2 v) {
  return make_double2(acc.x + sg * (cr * v.x - ci * v.y), acc.y + sg * (cr * v.y + ci * v.x));
}

// seeds: [nseed][dim] (unnormalised on exit); partials: [nseed][gridDim.x].
// The host has checked that every level maps src into dst, so every source
// state of a hit lies in idx_src's tables (DevIndex does not check bounds); a
// miss looks nothing up.
template <bool VC>
__global__ void __launch_bounds__(kBlock) k_seed_gather(const uint32_t* __restrict__ map_dst, int64_t dim,
                                                        DevIndex idx_src, int op, SeedTable T,
                                                        const val_t<VC>* __restrict__ x,
                                                        val_t<VC>* __restrict__ seeds,
                                                        double* __restrict__ partials) {
  using V = val_t<VC>;
  double n2[kSeedMaxSeeds];
#pragma unroll
  for (int q = 0; q < kSeedMaxSeeds; q++) n2[q] = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < dim; r += (int64_t)gridDim.x * kBlock) {
    const uint32_t t = map_dst[r];
    V v[kSeedMaxLev];
    double sg[kSeedMaxLev];
#pragma unroll
    for (int l = 0; l < kSeedMaxLev; l++) {
      v[l] = vzero<V>();
      sg[l] = 1.0;
      if (l < T.nlev) {
        const int lev = T.lev[l];
        if (bit(t, lev) == op) {  // c^+ left the level occupied, c left it empty
          const uint32_t s = t ^ (1u << lev);
          sg[l] = jw_sign(s, lev);
          v[l] = x[idx_src(s)];
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kSeedMaxSeeds; q++) {
      if (q < T.nseed) {
        V acc = vzero<V>();
#pragma unroll
        for (int l = 0; l < kSeedMaxLev; l++)
          if ((T.used[q] >> l) & 1)
            acc = seed_add(acc, T.cr[q][l], T.ci[q][l], sg[l], v[l]);
        seeds[(size_t)q * dim + r] = acc;
        n2[q] += seed_abs2(acc);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kSeedMaxSeeds; q++)
    if (q < T.nseed) block_partial(n2[q], partials + (size_t)q * gridDim.x);
}

// seeds: [P.nseed][dim] (unnormalised on exit); partials: [P.nseed][gridDim.x].
// The host has checked (seed_plan_compile) that every image maps src into
// dst, so every source state of a hit lies in idx_src's tables; a miss looks
// nothing up.  u_l = sg_l * v_l is what k_apply_op stores, u_p + u_q what
// k_apply_op_acc with coefficient 1 leaves: the chain's values.  The plan is
// the same in every lane, so the selects below are on scalar conditions; the
// images are never indexed by a run-time value (that would put them in
// scratch).
template <bool VC>
__global__ void __launch_bounds__(kBlock) k_seed_plan(const uint32_t* __restrict__ map_dst, int64_t dim,
                                                      DevIndex idx_src, SeedPlan P,
                                                      const val_t<VC>* __restrict__ x,
                                                      val_t<VC>* __restrict__ seeds,
                                                      double* __restrict__ partials) {
  using V = val_t<VC>;
  double n2[kSeedMaxSeeds];
#pragma unroll
  for (int s = 0; s < kSeedMaxSeeds; s++) n2[s] = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < dim; r += (int64_t)gridDim.x * kBlock) {
    const uint32_t t = map_dst[r];
    V u[kSeedMaxLev];
#pragma unroll
    for (int l = 0; l < kSeedMaxLev; l++) {
      u[l] = vzero<V>();
      if (l < P.nlev) {
        uint32_t s;
        double sg;
        if (seed_image(t, P.lev[l], P.op[l], &s, &sg)) u[l] = scl(sg, x[idx_src(s)]);
      }
    }
    // A zero the compiler cannot see through, renewed per row: without it the
    // 2 * 6 * 32 comparisons below are loop-invariant, get hoisted as 64-bit
    // lane masks and spill (979 SGPRs); with it they are scalar compares next
    // to their selects.
    int z = 0;
    asm volatile("" : "+s"(z));
#pragma unroll
    for (int s = 0; s < kSeedMaxSeeds; s++) {
      if (s < P.nseed) {
        V a = vzero<V>(), b = vzero<V>();
#pragma unroll
        for (int l = 0; l < kSeedMaxLev; l++) {
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
  for (int s = 0; s < kSeedMaxSeeds; s++)
    if (s < P.nseed) block_partial(n2[s], partials + (size_t)s * gridDim.x);
}

// grid (blocks per seed, nseed).  npart: the gather's grid.
template <bool VC>
__global__ void __launch_bounds__(kBlock) k_seed_scale(val_t<VC>* __restrict__ seeds, int64_t dim,
                                                       const double* __restrict__ partials, int npart,
                                                       double* __restrict__ norm2) {
  const int q = blockIdx.y;
  const double tot = sum_partials(partials + (size_t)q * npart, npart);
  if (blockIdx.x == 0 && threadIdx.x == 0) norm2[q] = tot;
  if (tot == 0.0) return;
  const double inv = 1.0 / sqrt(tot);
  val_t<VC>* y = seeds + (size_t)q * dim;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < dim; r += (int64_t)gridDim.x * kBlock)
    y[r] = scl(inv, y[r]);
}

}  // namespace edg
