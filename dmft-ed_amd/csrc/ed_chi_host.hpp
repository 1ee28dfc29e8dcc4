// ed_chi_host.hpp — the host half of the susceptibility kernels of ed_chi.hpp
// (k_seed_diag / ed_sector_seed_diag, k_chi_poles / ed_chi_add_poles): plain
// C++, compiles with g++ alone, as ed_seed_plan.hpp does.
//
// The susceptibility seeds of the reference (lanc_ed_build_spinChi_c,
// ED_GF_CHISPIN.f90:61-141; lanc_ed_build_densChi_diag_c,
// ED_GF_CHIDENS.f90:90-169, and their _tot / _offdiag forms) apply Sz_a, n_a
// and sums of them: operators diagonal in the Fock basis, so a seed is the
// kept state's own vector times one real factor per row,
//   seed_q[r] = (sum_l weight[q][l] * bit(map[r], levels[l])) * vec[r],
// and it stays in the kept state's sector.
//
//   DiagTable          levels and weights: the kernel's by-value argument.
//   seed_diag_compile  validates one call's table.
//   seed_diag_factor   the one definition of a row's factor, shared by the
//                      kernel and the host restatement.
//   seed_diag_host     the kernel's arithmetic, serially in row order.
//   chi_thermal        1 - exp(-beta D) and s(D) = (1 - exp(-beta D)) / D of a
//                      pole, by expm1 (departure 1).
//   kChiBoth / kChiPlus / kChiMinus
//                      the isign branches a fraction of the pole sum takes.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/ed_gpu.h"

#if defined(__HIPCC__)
#define ED_CHI_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ED_CHI_HD inline
#endif

namespace edg {

constexpr int kDiagMaxLev = 2 * ED_MAX_NORB;  // levels of one call (kSeedMaxLev)
constexpr int kDiagMaxSeeds = 32;             // seeds of one call (kSeedMaxSeeds)

// w[q][l] of a level past nlev is 0: the kernel's unrolled sum adds +0.0 for it.
struct DiagTable {
  int32_t nlev, nseed;
  int32_t lev[kDiagMaxLev];
  double w[kDiagMaxSeeds][kDiagMaxLev];
};

// levels: [nlev] distinct 0-based bits below 2*ns; weight: [nseed][nlev].
// ED_ERR_ARG unless 1 <= nlev <= kDiagMaxLev and 1 <= nseed <= kDiagMaxSeeds.
inline int seed_diag_compile(int ns, int nlev, const int32_t* levels, int nseed, const double* weight,
                             DiagTable* out) {
  if (!levels || !weight || !out) return ED_ERR_ARG;
  if (ns < 1 || ns > ED_MAX_NS) return ED_ERR_ARG;
  if (nlev < 1 || nlev > kDiagMaxLev || nseed < 1 || nseed > kDiagMaxSeeds) return ED_ERR_ARG;
  DiagTable T{};
  T.nlev = nlev;
  T.nseed = nseed;
  for (int l = 0; l < nlev; l++) {
    if (levels[l] < 0 || levels[l] >= 2 * ns) return ED_ERR_ARG;
    for (int k = 0; k < l; k++)
      if (levels[k] == levels[l]) return ED_ERR_ARG;
    T.lev[l] = levels[l];
  }
  for (int q = 0; q < nseed; q++)
    for (int l = 0; l < nlev; l++) T.w[q][l] = weight[(size_t)q * nlev + l];
  *out = T;
  return ED_OK;
}

// The factor of one row: the weights of the occupied levels, added in level
// order in double.  b[l] is 0.0 or 1.0, so w * b is w or +-0 exactly.
ED_CHI_HD double seed_diag_factor(const double* w, const double* b) {
  double c = 0.0;
  for (int l = 0; l < kDiagMaxLev; l++) c = c + w[l] * b[l];
  return c;
}

// The unnormalised seeds and their norm2, serially in row order.  x: real(8)
// (vc = false) or complex(8) interleaved, [dim]; seeds: [nseed][dim] of the
// same type; norm2: [nseed].
inline void seed_diag_host(const DiagTable& T, int64_t dim, const uint32_t* map, const double* x, bool vc,
                           double* seeds, double* norm2) {
  const int w = vc ? 2 : 1;
  for (int q = 0; q < T.nseed; q++) norm2[q] = 0.0;
  for (int64_t r = 0; r < dim; r++) {
    double b[kDiagMaxLev];
    for (int l = 0; l < kDiagMaxLev; l++) b[l] = l < T.nlev ? (double)((map[r] >> T.lev[l]) & 1u) : 0.0;
    for (int q = 0; q < T.nseed; q++) {
      const double c = seed_diag_factor(T.w[q], b);
      for (int k = 0; k < w; k++) {
        const double a = c * x[w * r + k];
        seeds[((size_t)q * dim + r) * w + k] = a;
        norm2[q] += a * a;
      }
    }
  }
}

// Which isign branches of add_to_lanczos_spinChi a fraction takes: the value
// is the isign argument of ed_chi_add_poles_signed (0: +1 and then -1).
constexpr int32_t kChiBoth = 0, kChiPlus = 1, kChiMinus = -1;
inline bool chi_sel_valid(int32_t isign) { return isign == kChiBoth || isign == kChiPlus || isign == kChiMinus; }

// f = 1 - exp(-beta D) and s = f / D, with s(0) = beta exactly: -expm1(-x)
// keeps every digit of f for small |x| and is right for D < 0, where the
// reference's cut beta*D < 0.1 (ED_GF_CHISPIN.f90:284-288) puts beta.
inline void chi_thermal(double beta, double D, double* f, double* s) {
  *f = -expm1(-beta * D);
  *s = D == 0.0 ? beta : *f / D;
}

}  // namespace edg
