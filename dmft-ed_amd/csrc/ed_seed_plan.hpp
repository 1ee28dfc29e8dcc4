// ed_seed_plan.hpp — the host half of the mixed-operator fused seed kernel
// (k_seed_plan in ed_seed.hpp, ed_sector_seed_plan): plain C++, compiles with
// g++ alone, as the host half of ed_obs.hpp does.
//
// The superconducting Green's function (lanc_build_gf_superc_c,
// ED_GF_SUPERC.f90:88-446) seeds one kept state with c^+_{a,up}, c_{a,dw} and
// their sum into sector sz+1, and with c_{a,up}, c^+_{a,dw} and their sum into
// sz-1: the images of one target sector mix operator types, and every seed is
// one image or the sum of two with unit coefficients.  So the kernel argument
// is a plan, not a coefficient table:
//   image l = op_l on level_l of |src_vec>      (l < nlev <= kSeedMaxLev)
//   seed  s = image p_s, or image p_s + image q_s   (s < nseed <= kSeedMaxSeeds)
// about 90 bytes against SeedTable's 3 KB of doubles.
//
//   seed_image          the one definition of "target-row state, (level, op)
//                       -> (hit, source state, sign)" shared by the kernel and
//                       the host restatement.
//   seed_op_target      the sector an operator maps src into (getCsector /
//                       getCDGsector); check_op_target in ed_hxv.hip calls it.
//   seed_terms_compile  validates the (p, q) terms: the encoding SeedPlan and
//                       PairPlan (ed_seed_pair.hpp) share.
//   seed_plan_compile   validates a plan for a (src, dst) pair of sectors.
//   seed_combine_host   the gather kernels' arithmetic, serially in row order,
//                       for any image functor; seed_plan_host and
//                       seed_pair_host are its two uses.
#pragma once
#include <stdint.h>

#include "../../include/ed_gpu.h"

#if defined(__HIPCC__)
#define ED_SEED_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ED_SEED_HD inline
#endif

namespace edg {

constexpr int kSeedMaxLev = 2 * ED_MAX_NORB;  // distinct images (levels) of one call
constexpr int kSeedMaxSeeds = 32;             // seeds of one call
constexpr uint8_t kSeedNone = 0xFF;           // SeedPlan::q of a one-image seed

struct SeedPlan {
  int32_t nlev, nseed;
  uint8_t lev[kSeedMaxLev], op[kSeedMaxLev];   // image l: op[l] (0 c, 1 c^+) on bit lev[l]
  uint8_t p[kSeedMaxSeeds], q[kSeedMaxSeeds];  // seed s: image p[s] (+ image q[s] unless kSeedNone)
};

// What the validation needs to know of the two sectors (ed_hxv.hip fills it
// from the sector objects, the CPU tests from the model's numbers).
struct SeedSectors {
  int32_t ns;            // levels per spin
  int32_t mode;          // ED_MODE_*
  int32_t jz;            // nonsu2 Jz_basis sectors
  const int32_t* lz2;    // [ns] 2*Lzdiag per level (jz only)
  int32_t src_q1, src_q2, dst_q1, dst_q2;
};

// Row state t of the TARGET sector and image (level, op): op left the level
// occupied (c^+) or empty (c), so the image hits iff bit `level` of t equals
// op; the source state is t with that bit flipped, and the Jordan-Wigner sign
// (c / cdg, ED_SETUP.f90:1080-1106) counts the bits below the level, which
// are the same in both states (jw_sign's value).
ED_SEED_HD bool seed_image(uint32_t t, int level, int op, uint32_t* source, double* sign) {
  if ((int)((t >> level) & 1u) != op) return false;
  const uint32_t s = t ^ (1u << level);
  *source = s;
  *sign = (__builtin_popcount(s & ((1u << level) - 1u)) & 1) ? -1.0 : 1.0;
  return true;
}

// Quantum numbers of the sector that op (0 c, 1 c^+) on `level` maps
// (q1, q2) into: getCsector / getCDGsector, ED_SETUP.f90:464-495 normal
// (nup, ndw), :590-619 superc (sz: c^+_up and c_dw raise it), :750-768 nonsu2
// (n) and :769-805 Jz_basis (n, twoJz -/+ (2*Lzdiag(iorb) + Szdiag(ispin))).
inline int seed_op_target(const SeedSectors& S, int op, int level, int32_t* e1, int32_t* e2) {
  if (op != 0 && op != 1) return ED_ERR_ARG;
  if (S.ns < 1 || S.ns > ED_MAX_NS || level < 0 || level >= 2 * S.ns) return ED_ERR_ARG;
  const int d = op == 1 ? 1 : -1, up = level < S.ns;
  *e1 = S.src_q1;
  *e2 = S.src_q2;
  if (S.mode == ED_MODE_NORMAL) {
    if (up) *e1 += d; else *e2 += d;
  } else if (S.mode == ED_MODE_SUPERC) {
    *e1 += up ? d : -d;
  } else if (S.mode == ED_MODE_NONSU2) {
    *e1 += d;
    if (S.jz) {
      if (!S.lz2) return ED_ERR_ARG;
      *e2 += d * (S.lz2[up ? level : level - S.ns] + (up ? 1 : -1));
    }
  } else {
    return ED_ERR_ARG;
  }
  return ED_OK;
}

// The term encoding SeedPlan and PairPlan (ed_seed_pair.hpp) share.  terms:
// [nseed][2] image indices (p, q), q < 0: the seed is image p alone; p, q:
// the plan's [max_seeds] arrays.  ED_ERR_ARG unless 1 <= nseed <= max_seeds
// and every p, q is below nimg with p != q.
inline int seed_terms_compile(int nimg, int nseed, int max_seeds, const int32_t* terms, uint8_t* p, uint8_t* q) {
  if (!terms || nseed < 1 || nseed > max_seeds) return ED_ERR_ARG;
  for (int s = 0; s < nseed; s++) {
    const int32_t ps = terms[2 * s], qs = terms[2 * s + 1];
    if (ps < 0 || ps >= nimg || qs >= nimg || qs == ps) return ED_ERR_ARG;
    p[s] = (uint8_t)ps;
    q[s] = qs < 0 ? kSeedNone : (uint8_t)qs;
  }
  return ED_OK;
}

// levels / ops: [nlev]; terms: as seed_terms_compile takes them.  ED_ERR_ARG
// unless 1 <= nlev <= kSeedMaxLev, every image maps src into dst, the
// (level, op) pairs are distinct, and the terms are valid.  The kernel's index
// tables do not bounds-check: these tests keep every source row inside them.
inline int seed_plan_compile(const SeedSectors& S, int nlev, const int32_t* levels, const int32_t* ops,
                             int nseed, const int32_t* terms, SeedPlan* out) {
  if (!levels || !ops || !out) return ED_ERR_ARG;
  if (nlev < 1 || nlev > kSeedMaxLev) return ED_ERR_ARG;
  SeedPlan P{};
  P.nlev = nlev;
  P.nseed = nseed;
  for (int l = 0; l < nlev; l++) {
    int32_t e1, e2;
    if (seed_op_target(S, ops[l], levels[l], &e1, &e2) != ED_OK) return ED_ERR_ARG;
    if (e1 != S.dst_q1 || e2 != S.dst_q2) return ED_ERR_ARG;
    for (int k = 0; k < l; k++)
      if (levels[k] == levels[l] && ops[k] == ops[l]) return ED_ERR_ARG;
    P.lev[l] = (uint8_t)levels[l];
    P.op[l] = (uint8_t)ops[l];
  }
  if (seed_terms_compile(nlev, nseed, kSeedMaxSeeds, terms, P.p, P.q) != ED_OK) return ED_ERR_ARG;
  *out = P;
  return ED_OK;
}

// The unnormalised seeds and their norm2, serially in row order: the gather
// kernels' arithmetic (u_l = sign_l * v_l per image, then u_p, or u_p + u_q)
// restated on the host.  image(t, l, &source, &sign) is the plan's image l of
// target-row state t (false: a miss); x: real(8) (vc = false) or complex(8)
// interleaved; index(state) -> 0-based row of the state in src; seeds:
// [nseed][dim] of the same type; norm2: [nseed].
template <int MaxImg, class Image, class Index>
inline void seed_combine_host(int nimg, int nseed, const uint8_t* p, const uint8_t* q, Image image, int64_t dim,
                              const uint32_t* map_dst, const double* x, bool vc, Index index, double* seeds,
                              double* norm2) {
  const int w = vc ? 2 : 1;
  for (int s = 0; s < nseed; s++) norm2[s] = 0.0;
  for (int64_t r = 0; r < dim; r++) {
    double u[MaxImg][2];
    for (int l = 0; l < nimg; l++) {
      uint32_t src;
      double sg;
      u[l][0] = u[l][1] = 0.0;
      if (!image(map_dst[r], l, &src, &sg)) continue;
      const int64_t j = index(src);
      for (int c = 0; c < w; c++) u[l][c] = sg * x[w * j + c];
    }
    for (int s = 0; s < nseed; s++)
      for (int c = 0; c < w; c++) {
        double a = u[p[s]][c];
        if (q[s] != kSeedNone) a = a + u[q[s]][c];
        seeds[((size_t)s * dim + r) * w + c] = a;
        norm2[s] += a * a;
      }
  }
}

// k_seed_plan's arithmetic (sg_p * v_p, then + sg_q * v_q) on the host.
template <class Index>
inline void seed_plan_host(const SeedPlan& P, int64_t dim, const uint32_t* map_dst, const double* x, bool vc,
                           Index index, double* seeds, double* norm2) {
  seed_combine_host<kSeedMaxLev>(
      P.nlev, P.nseed, P.p, P.q,
      [&](uint32_t t, int l, uint32_t* src, double* sg) { return seed_image(t, P.lev[l], P.op[l], src, sg); }, dim,
      map_dst, x, vc, index, seeds, norm2);
}

}  // namespace edg
