// ed_obs.hpp — expectation values of the kept states: observables_impurity
// (ED_OBSERVABLES.f90:48-715) and local_energy_impurity (:726-980).
//
// Host half (plain C++, compiles with g++ alone): an operator string
//   T = o_1 o_2 ... o_n,   o_k = c_level (op 0) or c^+_level (op 1),  n = 1..4,
// applied right to left, is compiled for one sector into an ObsTerm: three
// masks and a sign recipe, so that a basis row costs two mask tests and one
// popcount instead of the reference's bdecomp + c/cdg chain + binary_search
// per element (:567-577, :805-812, :891-898).  obs_row is the one definition
// of "state, term -> (hit, target state, sign)" shared by the host evaluator
// and the kernel.
//
// Device half (under hipcc): k_nn_moments (the diagonal quantities of
// :127-158 and :797-943 as pair moments of the level occupations) and
// k_expect (the off-diagonal ones), both one grid-strided pass with the
// two-pass block_partial / sum_partials reduction: no floating-point atomics,
// so two calls on the same input return the same bits.
#pragma once
#include <stdint.h>

#include "../../include/ed_gpu.h"

#if defined(__HIPCC__)
#define ED_OBS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ED_OBS_HD inline
#endif

namespace edg {

constexpr int kObsMaxOps = 4;                    // operators per string
constexpr int kObsMaxLev = 2 * ED_MAX_NORB;      // levels of one nn_moments call
constexpr int kObsMaxMom = kObsMaxLev * (kObsMaxLev + 1) / 2 + 1;  // pair moments + norm
constexpr int kObsTile = 8;                      // terms per register tile of k_expect
constexpr int kObsMaxTerms = 128;                // terms of one k_expect launch (kernel argument)

// One compiled operator string.  A source state m contributes iff
// (m & need1) == need1 and (m & need0) == 0; then T|m> = sign |m ^ flip> with
// sign = (-1)^(popc(m & smask) + s0).
struct ObsTerm {
  uint32_t need1, need0, flip, smask;
  int32_t s0;
};

// What the compile step needs to know of a sector (ed_hxv.hip fills it from
// the sector object, the CPU tests from the model's numbers).
struct ObsSector {
  int32_t ns;           // levels per spin
  int32_t mode;         // ED_MODE_*
  int32_t jz;           // nonsu2 Jz_basis sector
  const int32_t* lz2;   // [ns] 2*Lzdiag per level (jz only)
};

// A term no state contributes to (c_p c_p, padding of a register tile).
ED_OBS_HD ObsTerm obs_null_term() { return ObsTerm{1u, 1u, 0u, 0u, 0}; }

// Compile levels[0..nop) / ops[0..nop) (applied right to left: the LAST entry
// acts first).  ED_ERR_ARG unless the string maps the sector into itself, by
// the rule getCsector / getCDGsector apply per operator (ED_SETUP.f90:464-495
// normal, :590-619 superc, :750-805 nonsu2 and Jz), summed over the string:
//   normal: d(nup) = d(ndw) = 0;  superc: d(nup - ndw) = 0;
//   nonsu2: d(n) = 0, and d(twoJz) = 0 for Jz_basis sectors.
// The kernel's index tables do not bounds-check: this test is what keeps
// every target inside them.
inline int obs_compile(const ObsSector& S, int nop, const int32_t* levels, const int32_t* ops, ObsTerm* out) {
  if (nop < 1 || nop > kObsMaxOps || !levels || !ops || !out) return ED_ERR_ARG;
  if (S.ns < 1 || S.ns > ED_MAX_NS) return ED_ERR_ARG;
  uint32_t need1 = 0, need0 = 0, flip = 0, smask = 0;
  int s0 = 0, dup = 0, ddw = 0, djz = 0;
  bool null = false;
  for (int k = nop - 1; k >= 0; k--) {
    const int p = levels[k], op = ops[k];
    if (p < 0 || p >= 2 * S.ns || (op != 0 && op != 1)) return ED_ERR_ARG;
    const uint32_t b = 1u << p, below = b - 1u;
    const int want = op == 1 ? 0 : 1;  // c^+ needs the level empty, c occupied
    if ((need1 | need0) & b) {
      // touched before: its value in the intermediate state is known
      const int now = ((need1 & b) ? 1 : 0) ^ ((flip & b) ? 1 : 0);
      if (now != want) null = true;
    } else if (want) {
      need1 |= b;
    } else {
      need0 |= b;
    }
    // Jordan-Wigner sign of this step on the intermediate state m ^ flip
    // (c / cdg, ED_SETUP.f90:1080-1106): popc((m ^ flip) & below) has the
    // parity of popc(m & below) + popc(flip & below)
    smask ^= below;
    s0 += __builtin_popcount(flip & below);
    flip ^= b;
    const int d = op == 1 ? 1 : -1, up = p < S.ns;
    if (up) dup += d; else ddw += d;
    if (S.jz && S.lz2) djz += d * (S.lz2[up ? p : p - S.ns] + (up ? 1 : -1));
  }
  bool keeps;
  if (S.mode == ED_MODE_NORMAL) keeps = dup == 0 && ddw == 0;
  else if (S.mode == ED_MODE_SUPERC) keeps = dup - ddw == 0;
  else if (S.mode == ED_MODE_NONSU2) keeps = dup + ddw == 0 && (!S.jz || djz == 0);
  else return ED_ERR_ARG;
  if (!keeps) return ED_ERR_ARG;
  *out = null ? obs_null_term() : ObsTerm{need1, need0, flip, smask, (int32_t)(s0 & 1)};
  return ED_OK;
}

// The per-row function: does state m contribute to the term, and if so to
// which state and with which sign.
ED_OBS_HD bool obs_row(uint32_t m, const ObsTerm& t, uint32_t* target, double* sign) {
  if ((m & t.need1) != t.need1 || (m & t.need0) != 0u) return false;
  *target = m ^ t.flip;
  *sign = ((__builtin_popcount(m & t.smask) + t.s0) & 1) ? -1.0 : 1.0;
  return true;
}

// <v|T|v> = sum_i conj(v_j(i)) * sign * v_i, serially in row order: the
// kernel's arithmetic restated on the host.  v: real(8) (vc = false) or
// complex(8) interleaved; index(state) -> 0-based row of the state.
template <class Index>
inline void obs_expect_host(const ObsTerm& t, int64_t dim, const uint32_t* map, const double* v, bool vc,
                            Index index, double* re, double* im) {
  double ar = 0.0, ai = 0.0;
  for (int64_t i = 0; i < dim; i++) {
    uint32_t k;
    double sg;
    if (!obs_row(map[i], t, &k, &sg)) continue;
    const int64_t j = index(k);
    if (vc) {
      const double xr = v[2 * i], xi = v[2 * i + 1], yr = v[2 * j], yi = v[2 * j + 1];
      ar += sg * (yr * xr + yi * xi);
      ai += sg * (yr * xi - yi * xr);
    } else {
      ar += sg * (v[j] * v[i]);
    }
  }
  *re = ar;
  *im = ai;
}

}  // namespace edg

// ------------------------------------------------------------------ device
#if defined(__HIPCC__)
#include "ed_kernels.hpp"

namespace edg {

struct ObsLevels {
  int32_t lev[kObsMaxLev];
};
struct ObsTermList {
  ObsTerm t[kObsMaxTerms];
};

__device__ __forceinline__ double abs2(double a) { return a * a; }
__device__ __forceinline__ double abs2(double2 a) { return a.x * a.x + a.y * a.y; }

// M[p][q] = sum_i |v_i|^2 n_p(i) n_q(i) (p <= q, packed upper triangle) and
// the norm: what the reference accumulates element by element with gs_weight
// (ED_OBSERVABLES.f90:127-158, :785-943).  One pass over (map, v): 4 + 8 (16)
// bytes per row.  partials: [NL*(NL+1)/2 + 1][gridDim.x].
template <bool VC, int NL>
__global__ void __launch_bounds__(kBlock) k_nn_moments(const uint32_t* __restrict__ map,
                                                       const val_t<VC>* __restrict__ v, int64_t dim,
                                                       ObsLevels L, double* __restrict__ partials) {
  constexpr int NM = NL * (NL + 1) / 2;
  double acc[NM + 1];
#pragma unroll
  for (int k = 0; k <= NM; k++) acc[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < dim; i += (int64_t)gridDim.x * kBlock) {
    const uint32_t m = map[i];
    const double w = abs2(v[i]);
    int k = 0;
#pragma unroll
    for (int p = 0; p < NL; p++) {
      const uint32_t bp = (m >> L.lev[p]) & 1u;
#pragma unroll
      for (int q = p; q < NL; q++, k++) acc[k] += (bp & (m >> L.lev[q])) ? w : 0.0;
    }
    acc[NM] += w;
  }
#pragma unroll
  for (int k = 0; k <= NM; k++) block_partial(acc[k], partials + (size_t)k * gridDim.x);
}

// The instantiation for nlev levels (1..kObsMaxLev; the caller checks).
template <bool VC>
inline void launch_nn_moments(int nlev, int grid, hipStream_t st, const uint32_t* map, const void* v, int64_t dim,
                              const ObsLevels& L, double* partials) {
  using V = val_t<VC>;
#define ED_NN_CASE(N)                                                                                   \
  case N:                                                                                               \
    hipLaunchKernelGGL((k_nn_moments<VC, N>), dim3(grid), dim3(kBlock), 0, st, map, (const V*)v, dim, L, \
                       partials);                                                                       \
    break;
  switch (nlev) {
    ED_NN_CASE(1) ED_NN_CASE(2) ED_NN_CASE(3) ED_NN_CASE(4) ED_NN_CASE(5) ED_NN_CASE(6)
  }
#undef ED_NN_CASE
}

// out[b] = fixed-order sum of row b of partials[nvals][n]: one block per value.
static __global__ void __launch_bounds__(kBlock) k_obs_finish(const double* __restrict__ partials, int n,
                                                       double* __restrict__ out) {
  const double tot = sum_partials(partials + (size_t)blockIdx.x * n, n);
  if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// <v|T_t|v> for nterm (a multiple of kObsTile, padded with null terms)
// compiled strings.  The terms are a kernel argument (scalar loads, the same
// in every lane); they are taken kObsTile at a time, and for one tile a row's
// map[i] and v[i] are loaded once and kept with the tile's accumulators in
// registers.  Per row and term: obs_row (two mask tests, one popcount), one
// DevIndex lookup and one gather v[j].  partials: [nterm][2][gridDim.x]
// (complex) or [nterm][gridDim.x] (real: the imaginary parts are zero).
template <bool VC>
__global__ void __launch_bounds__(kBlock) k_expect(const uint32_t* __restrict__ map,
                                                   const val_t<VC>* __restrict__ v, int64_t dim, DevIndex idx,
                                                   ObsTermList T, int nterm, double* __restrict__ partials) {
  using V = val_t<VC>;
  for (int t0 = 0; t0 < nterm; t0 += kObsTile) {
    double ar[kObsTile], ai[kObsTile];
#pragma unroll
    for (int k = 0; k < kObsTile; k++) ar[k] = ai[k] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < dim; i += (int64_t)gridDim.x * kBlock) {
      const uint32_t m = map[i];
      const V x = v[i];
#pragma unroll
      for (int k = 0; k < kObsTile; k++) {
        uint32_t tg;
        double sg;
        if (obs_row(m, T.t[t0 + k], &tg, &sg)) {
          const V y = v[idx(tg)];
          if constexpr (VC) {
            ar[k] += sg * (y.x * x.x + y.y * x.y);
            ai[k] += sg * (y.x * x.y - y.y * x.x);
          } else {
            ar[k] += sg * (y * x);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kObsTile; k++) {
      if constexpr (VC) {
        block_partial(ar[k], partials + (size_t)(2 * (t0 + k)) * gridDim.x);
        block_partial(ai[k], partials + (size_t)(2 * (t0 + k) + 1) * gridDim.x);
      } else {
        block_partial(ar[k], partials + (size_t)(t0 + k) * gridDim.x);
      }
    }
  }
}

}  // namespace edg
#endif  // __HIPCC__
