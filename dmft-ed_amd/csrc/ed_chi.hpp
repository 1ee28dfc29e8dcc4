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
//   k_chi_poles   the pole sums of add_to_lanczos_spinChi
//                 (ED_GF_CHISPIN.f90:254-323) on the bosonic Matsubara, the
//                 imaginary-time and the real-frequency grids, with both
//                 isign branches of a fraction or one of them.
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

// ------------------------------------------------ susceptibility pole sums
// add_to_lanczos_spinChi (ED_GF_CHISPIN.f90:254-323) for one tridiagonalisation,
// called with isign = +1 and then -1 as the reference's builders do
// (ED_GF_CHISPIN.f90:126-131).  With D = E_j - Ei, peso_j = (peso * z_j) * z_j,
// f_j = 1 - exp(-beta D) and s_j = f_j / D (chi_thermal, staged by the host),
// a fraction adds pole by pole
//   isign +1: iv(0) += peso_j s_j      iv(i) += -peso_j f_j / (i v_i - D)
//             tau(i) += peso_j exp(-tau_i D)
//             w(i)   += -peso_j f_j / (wr_i + i eps - D)
//   isign -1: iv(0) += peso_j s_j      iv(i) += peso_j f_j / (i v_i + D)
//             tau(i) += peso_j exp(-(beta - tau_i) D)
//             w(i)   += peso_j f_j / (wr_i + i eps + D)
// all poles with +1 first, then all with -1.  ChiFrac::sel picks the branches:
// kChiBoth (a Hermitian seed: the two calls above), kChiPlus or kChiMinus (one
// call with that isign: a seed O^+|n> or O|n> of a non-Hermitian O, DESIGN.md
// section 13).  One thread per grid point, the
// three grids laid end to end: iv 0..lmats, tau 0..ltau, w 1..lreal; fraction
// and pole data are wave-uniform; the arrays stay in HBM across flushes.
struct ChiFrac {
  int32_t p0, np, comp, sel;  // sel: kChiBoth / kChiPlus / kChiMinus (ed_chi_host.hpp)
  double peso, ei;  // w_n * norm2 (real), Ei
};

static __global__ void __launch_bounds__(kBlock) k_chi_poles(const ChiFrac* __restrict__ fr, int nfrac,
                                                      const double* __restrict__ E, const double* __restrict__ z,
                                                      const double* __restrict__ fth, const double* __restrict__ sth,
                                                      double beta, const double* __restrict__ vm, int nmats,
                                                      const double* __restrict__ tau, int ntau,
                                                      const double* __restrict__ wr, int lreal, double eps,
                                                      double2* __restrict__ civ, double* __restrict__ ctau,
                                                      double2* __restrict__ cw) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= nmats + ntau + lreal) return;
  // kind 0: iv(0), 1: iv(i >= 1), 2: tau, 3: real axis
  const int kind = t == 0 ? 0 : t < nmats ? 1 : t < nmats + ntau ? 2 : 3;
  const int i = kind < 2 ? t : kind == 2 ? t - nmats : t - nmats - ntau;
  const int L = kind < 2 ? nmats : kind == 2 ? ntau : lreal;
  const double re_w = kind == 3 ? wr[i] : 0.0;  // dcmplx(0, vm(i)); dcmplx(wr(i), eps)
  const double im_w = kind == 1 ? vm[i] : eps;
  const double tp = kind == 2 ? tau[i] : 0.0, tm = beta - tp;
  int cur = -1;
  double2 g = make_double2(0.0, 0.0);
  for (int f = 0; f < nfrac; f++) {
    const ChiFrac q = fr[f];
    if (q.comp != cur) {
      if (cur >= 0) {
        if (kind == 2) ctau[(int64_t)cur * L + i] = g.x;
        else (kind == 3 ? cw : civ)[(int64_t)cur * L + i] = g;
      }
      cur = q.comp;
      g = kind == 2 ? make_double2(ctau[(int64_t)cur * L + i], 0.0) : (kind == 3 ? cw : civ)[(int64_t)cur * L + i];
    }
    for (int sg = 0; sg < 2; sg++) {  // isign = +1, then -1
      if (q.sel == (sg ? kChiPlus : kChiMinus)) continue;  // a one-sign fraction: the other branch is not its
      for (int j = 0; j < q.np; j++) {
        const double zj = z[q.p0 + j];
        const double de = E[q.p0 + j] - q.ei;
        const double peso = (q.peso * zj) * zj;
        if (kind == 0) {
          g.x = g.x + peso * sth[q.p0 + j];
        } else if (kind == 2) {
          g.x = g.x + peso * exp(-(sg ? tm : tp) * de);
        } else {
          const double num = peso * fth[q.p0 + j];
          const double2 c = sg ? cdiv(make_double2(num, 0.0), re_w + de, im_w)
                               : cdiv(make_double2(-num, 0.0), re_w - de, im_w);
          g = make_double2(g.x + c.x, g.y + c.y);
        }
      }
    }
  }
  if (cur >= 0) {
    if (kind == 2) ctau[(int64_t)cur * L + i] = g.x;
    else (kind == 3 ? cw : civ)[(int64_t)cur * L + i] = g;
  }
}

}  // namespace edg
