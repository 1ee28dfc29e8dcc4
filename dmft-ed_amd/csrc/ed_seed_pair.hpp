// ed_seed_pair.hpp — the host half of the two-operator fused seed kernel
// (k_seed_pair in ed_chi.hpp, ed_sector_seed_pair): plain C++, compiles with
// g++ alone, as ed_seed_plan.hpp does.
//
// The pair susceptibility (build_chi_pair, ED_GF_CHIPAIR.f90:98-102 and
// :144-148) seeds one kept state with c_{a,dw} then c_{a,up}, and with
// c^+_{a,up} then c^+_{a,dw}; the inter-orbital density susceptibility
// (lanc_ed_build_densChi_mix_c, ED_GF_CHIDENS.f90:523-586 and :596-659) with
// sum_sigma c^+_{b,sigma} c_{a,sigma}.  Every image is the product of two
// ladder operators on different levels, and every seed is one image or the sum
// of two with unit coefficients:
//   image l = op2_l on lev2_l applied after op1_l on lev1_l of |src_vec>
//                                                   (l < nimg <= kPairMaxImg)
//   seed  s = image p_s, or image p_s + image q_s   (s < nseed <= kPairMaxSeeds)
//
//   seed_image2         "target-row state, image -> (hit, source state, sign)"
//                       as two calls of seed_image (ed_seed_plan.hpp): the one
//                       definition shared by the kernel and the host
//                       restatement.
//   seed_pair_compile   validates a plan for a (src, dst) pair of sectors by
//                       composing seed_op_target twice per image.
//   seed_pair_host      the kernel's arithmetic, serially in row order
//                       (seed_combine_host with seed_image2).
// The (p, q) term encoding and its validation are ed_seed_plan.hpp's.
#pragma once
#include "ed_seed_plan.hpp"

namespace edg {

constexpr int kPairMaxImg = 12;    // 2 * Norb * (Norb - 1) at ED_MAX_NORB: the exc images of one kept state
constexpr int kPairMaxSeeds = 12;  // seeds of one call
static_assert(kPairMaxImg == 2 * ED_MAX_NORB * (ED_MAX_NORB - 1), "the exc images of one kept state fit one call");

struct PairImage {
  uint8_t lev1, op1, lev2, op2;  // op (0 c, 1 c^+) on bit lev; (lev1, op1) acts first
};

struct PairPlan {
  int32_t nimg, nseed;
  PairImage img[kPairMaxImg];
  uint8_t p[kPairMaxSeeds], q[kPairMaxSeeds];  // seed s: image p[s] (+ image q[s] unless kSeedNone)
};

// Row state t of the TARGET sector: (lev2, op2) acted last, so it left its
// level as seed_image tests it and t with that bit flipped is the
// intermediate state; (lev1, op1) left the intermediate state the same way
// and the source state is the intermediate one with bit lev1 flipped.  The
// matrix element <t| op2 op1 |source> is sign1 * sign2.
ED_SEED_HD bool seed_image2(uint32_t t, PairImage im, uint32_t* source, double* sign) {
  uint32_t mid;
  double sign2, sign1;
  if (!seed_image(t, im.lev2, im.op2, &mid, &sign2)) return false;
  if (!seed_image(mid, im.lev1, im.op1, source, &sign1)) return false;
  *sign = sign1 * sign2;
  return true;
}

// images: [nimg][4] (lev1, op1, lev2, op2); terms: as seed_terms_compile
// (ed_seed_plan.hpp) takes them.  ED_ERR_ARG unless 1 <= nimg <= kPairMaxImg,
// lev1 != lev2 in every image, every image maps src into dst exactly
// (seed_op_target composed twice; the intermediate quantum numbers need not
// belong to a sector that exists: such an image never hits), no two images
// are the same, and the terms are valid.  The kernel's index tables do not
// bounds-check: these tests keep every source row of a hit inside them.
inline int seed_pair_compile(const SeedSectors& S, int nimg, const int32_t* images, int nseed,
                             const int32_t* terms, PairPlan* out) {
  if (!images || !out) return ED_ERR_ARG;
  if (nimg < 1 || nimg > kPairMaxImg) return ED_ERR_ARG;
  PairPlan P{};
  P.nimg = nimg;
  P.nseed = nseed;
  for (int l = 0; l < nimg; l++) {
    const int32_t* im = images + 4 * l;
    if (im[0] == im[2]) return ED_ERR_ARG;
    SeedSectors M = S;
    if (seed_op_target(S, im[1], im[0], &M.src_q1, &M.src_q2) != ED_OK) return ED_ERR_ARG;
    int32_t e1, e2;
    if (seed_op_target(M, im[3], im[2], &e1, &e2) != ED_OK) return ED_ERR_ARG;
    if (e1 != S.dst_q1 || e2 != S.dst_q2) return ED_ERR_ARG;
    for (int k = 0; k < l; k++) {
      const int32_t* o = images + 4 * k;
      if (o[0] == im[0] && o[1] == im[1] && o[2] == im[2] && o[3] == im[3]) return ED_ERR_ARG;
    }
    P.img[l] = PairImage{(uint8_t)im[0], (uint8_t)im[1], (uint8_t)im[2], (uint8_t)im[3]};
  }
  if (seed_terms_compile(nimg, nseed, kPairMaxSeeds, terms, P.p, P.q) != ED_OK) return ED_ERR_ARG;
  *out = P;
  return ED_OK;
}

// k_seed_pair's arithmetic ((sign1 * sign2) * v_p, then + the same of q) on
// the host: seed_combine_host (ed_seed_plan.hpp) with seed_image2.
template <class Index>
inline void seed_pair_host(const PairPlan& P, int64_t dim, const uint32_t* map_dst, const double* x, bool vc,
                           Index index, double* seeds, double* norm2) {
  seed_combine_host<kPairMaxImg>(
      P.nimg, P.nseed, P.p, P.q,
      [&](uint32_t t, int l, uint32_t* src, double* sg) { return seed_image2(t, P.img[l], src, sg); }, dim, map_dst,
      x, vc, index, seeds, norm2);
}

}  // namespace edg
