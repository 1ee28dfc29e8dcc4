// ed_poles.hip — the pole sums of the C-ABI (include/ed_gpu.h): the poles of
// one continued fraction on the host, and the Green's function and
// susceptibility sums over all fractions on the device.  No sector is
// involved: the caller's stream orders everything.
#include <string.h>

#include <algorithm>
#include <vector>

#include "ed_host.hpp"
#include "ed_hosteig.hpp"
#include "ed_chi_host.hpp"
#include "ed_kernels.hpp"

using namespace edg;

namespace edg {
// ------------------------------------------------ GF pole sums (device G)
// add_to_lanczos_gf_normal (ED_GF_NORMAL.f90:620-631) / _nonsu2
// (ED_GF_NONSU2.f90:936-950): for every frequency i, fraction by fraction in
// list order and pole by pole (j ascending), exactly the reference's sequence
// of additions into G(i):
//   G(i) = G(i) + peso_j / (iw_i - isign*de_j),  de_j = E_j - Ei,
//   peso_j = (pesoBZ * z_j) * z_j,  iw = (0, wm_i) or (wr_i, eps).
// One thread per frequency (Matsubara then real axis); the fraction and pole
// data are wave-uniform (scalar loads); G stays in HBM across seeds.
struct GfFrac {
  int32_t p0, np, comp, isign;
  double pr, pi, ei;  // pesoBZ (complex), Ei
  double pad;
};

static __global__ void __launch_bounds__(kBlock) k_gf_poles(const GfFrac* __restrict__ fr, int nfrac,
                                                     const double* __restrict__ E, const double* __restrict__ z,
                                                     const double* __restrict__ wm, int lmats,
                                                     const double* __restrict__ wr, int lreal, double eps,
                                                     double2* __restrict__ gm, double2* __restrict__ gr) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= lmats + lreal) return;
  const bool mats = t < lmats;
  const int i = mats ? t : t - lmats;
  const double re_w = mats ? 0.0 : wr[i];   // iw = xi*wm(i) = (0, wm); dcmplx(wr(i), eps)
  const double im_w = mats ? wm[i] : eps;
  double2* G = mats ? gm : gr;
  const int L = mats ? lmats : lreal;
  int cur = -1;
  double2 g = make_double2(0.0, 0.0);
  for (int f = 0; f < nfrac; f++) {
    const GfFrac q = fr[f];
    if (q.comp != cur) {
      if (cur >= 0) G[(int64_t)cur * L + i] = g;
      cur = q.comp;
      g = G[(int64_t)cur * L + i];
    }
    const double sgn = (double)q.isign;
    for (int j = 0; j < q.np; j++) {
      const double zj = z[q.p0 + j];
      const double de = E[q.p0 + j] - q.ei;
      const double2 peso = make_double2((q.pr * zj) * zj, (q.pi * zj) * zj);
      const double d = sgn * de;
      const double2 c = cdiv(peso, re_w - d, im_w);
      g = make_double2(g.x + c.x, g.y + c.y);
    }
  }
  if (cur >= 0) G[(int64_t)cur * L + i] = g;
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

// The staged launch of a pole sum: the host staging block `hb` goes to a
// device block allocated on stream st, `launch` puts its kernel on st with
// that block's base pointer, the block is freed on st, and the stream is
// synchronised before the return (the caller's staging dies with it).
template <class Launch>
static int staged_launch(const std::vector<unsigned char>& hb, hipStream_t st, Launch launch) {
  void* d = nullptr;
  HIPCK(hipMallocAsync(&d, hb.size(), st));
  HIPCK(hipMemcpyAsync(d, hb.data(), hb.size(), hipMemcpyHostToDevice, st));
  launch((const unsigned char*)d);
  const hipError_t le = hipGetLastError();
  (void)hipFreeAsync(d, st);
  // the host staging vector dies on return: the copy must have completed
  HIPCK(hipStreamSynchronize(st));
  HIPCK(le);
  return ED_OK;
}

extern "C" {

// Poles of one GF continued fraction: eigenvalues of tridiag(alfa[0:n],
// beta[1:n]) and the squared first components of the eigenvectors, the
// quantities add_to_lanczos_gf_nonsu2 takes from tql2 (ED_GF_NONSU2.f90:936,
// ED_GF_SHARED.f90:76-214; add_to_lanczos_gf_normal uses eigh,
// ED_GF_NORMAL.f90:612-618).  The EISPACK implicit-QL iteration with the
// rotations applied to the first row of Z only (Z starts as the identity, so
// that row starts as e_1): O(n^2) instead of the O(n^3) full eigenvector
// accumulation; same pythag, shifts and convergence test as tql2
// (ql_implicit's first-row sink, ed_hosteig.hpp).
int ed_tridiag_poles(int32_t n, const double* alfa, const double* beta, double* E, double* z2, double* z1) {
  if (n < 1 || !alfa || !beta || !E || !z2) return fail(ED_ERR_ARG, "bad args");
  if (tridiag_poles(n, alfa, beta, E, z2, z1) != 0) return fail(ED_ERR_NOCONV, "tridiagonal QL: no convergence");
  return ED_OK;
}

int ed_gf_add_poles(int32_t nfrac, const int32_t* npole, const double* E, const double* z, const double* peso_bz,
                    const double* Ei, const int32_t* isign, const int32_t* comp, const double* wm, int32_t lmats,
                    const double* wr, int32_t lreal, double eps, double* gm, double* gr, void* stream) {
  if (nfrac < 0 || lmats < 0 || lreal < 0) return fail(ED_ERR_ARG, "bad sizes");
  if (nfrac == 0 || lmats + lreal == 0) return ED_OK;
  if (!npole || !E || !z || !peso_bz || !Ei || !isign || !comp || (lmats && (!wm || !gm)) ||
      (lreal && (!wr || !gr)))
    return fail(ED_ERR_ARG, "null");
  std::vector<GfFrac> fr(nfrac);
  int64_t np = 0;
  for (int f = 0; f < nfrac; f++) {
    if (npole[f] < 0 || comp[f] < 0 || (isign[f] != 1 && isign[f] != -1)) return fail(ED_ERR_ARG, "bad fraction");
    fr[f].p0 = (int32_t)np;
    fr[f].np = npole[f];
    fr[f].comp = comp[f];
    fr[f].isign = isign[f];
    fr[f].pr = peso_bz[2 * f];
    fr[f].pi = peso_bz[2 * f + 1];
    fr[f].ei = Ei[f];
    fr[f].pad = 0.0;
    np += npole[f];
  }
  // one staging buffer: fractions | E | z
  const size_t bf = fr.size() * sizeof(GfFrac), be = (size_t)std::max<int64_t>(np, 1) * 8;
  std::vector<unsigned char> hb(bf + 2 * be);
  memcpy(hb.data(), fr.data(), bf);
  if (np) {
    memcpy(hb.data() + bf, E, np * 8);
    memcpy(hb.data() + bf + be, z, np * 8);
  }
  hipStream_t st = (hipStream_t)stream;
  const int nt = lmats + lreal;
  return staged_launch(hb, st, [&](const unsigned char* db) {
    hipLaunchKernelGGL(k_gf_poles, dim3((nt + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (const GfFrac*)db, nfrac,
                       (const double*)(db + bf), (const double*)(db + bf + be), wm, lmats, wr, lreal, eps,
                       (double2*)gm, (double2*)gr);
  });
}

// Pole sums of the susceptibilities (k_chi_poles above): every fraction
// is one tridiagonalisation of add_to_lanczos_spinChi (ED_GF_CHISPIN.f90:254-323)
// with both isign calls (isign[f] == 0 or isign == NULL) or with the one named
// by isign[f] = +-1.  The thermal factors of a pole are computed here
// (chi_thermal: expm1), so the kernel's only transcendental is exp on tau.
int ed_chi_add_poles_signed(int32_t nfrac, const int32_t* npole, const double* E, const double* z,
                            const double* peso, const double* Ei, const int32_t* comp, const int32_t* isign,
                            double beta, const double* vm, int32_t lmats, const double* tau, int32_t ltau,
                            const double* wr, int32_t lreal, double eps, double* chi_iv, double* chi_tau,
                            double* chi_w, void* stream) {
  if (nfrac < 0 || lmats < 0 || ltau < 0 || lreal < 0) return fail(ED_ERR_ARG, "bad sizes");
  if (nfrac == 0) return ED_OK;
  if (!npole || !E || !z || !peso || !Ei || !comp || !vm || !tau || !chi_iv || !chi_tau || (lreal && (!wr || !chi_w)))
    return fail(ED_ERR_ARG, "null");
  std::vector<ChiFrac> fr(nfrac);
  int64_t np = 0;
  for (int f = 0; f < nfrac; f++) {
    if (npole[f] < 0 || comp[f] < 0) return fail(ED_ERR_ARG, "bad fraction");
    if (isign && !chi_sel_valid(isign[f])) return fail(ED_ERR_ARG, "isign must be 0 (both), +1 or -1");
    fr[f].p0 = (int32_t)np;
    fr[f].np = npole[f];
    fr[f].comp = comp[f];
    fr[f].sel = isign ? isign[f] : kChiBoth;
    fr[f].peso = peso[f];
    fr[f].ei = Ei[f];
    np += npole[f];
  }
  // one staging buffer: fractions | E | z | 1 - exp(-beta D) | s(D)
  const size_t bf = fr.size() * sizeof(ChiFrac), be = (size_t)std::max<int64_t>(np, 1) * 8;
  std::vector<unsigned char> hb(bf + 4 * be);
  memcpy(hb.data(), fr.data(), bf);
  if (np) {
    memcpy(hb.data() + bf, E, np * 8);
    memcpy(hb.data() + bf + be, z, np * 8);
    double* hf = (double*)(hb.data() + bf + 2 * be);
    double* hs = (double*)(hb.data() + bf + 3 * be);
    for (int f = 0; f < nfrac; f++)
      for (int j = fr[f].p0; j < fr[f].p0 + fr[f].np; j++) chi_thermal(beta, E[j] - fr[f].ei, hf + j, hs + j);
  }
  hipStream_t st = (hipStream_t)stream;
  const int nt = (lmats + 1) + (ltau + 1) + lreal;
  return staged_launch(hb, st, [&](const unsigned char* db) {
    hipLaunchKernelGGL(k_chi_poles, dim3((nt + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (const ChiFrac*)db, nfrac,
                       (const double*)(db + bf), (const double*)(db + bf + be), (const double*)(db + bf + 2 * be),
                       (const double*)(db + bf + 3 * be), beta, vm, lmats + 1, tau, ltau + 1, wr, lreal, eps,
                       (double2*)chi_iv, chi_tau, (double2*)chi_w);
  });
}

int ed_chi_add_poles(int32_t nfrac, const int32_t* npole, const double* E, const double* z, const double* peso,
                     const double* Ei, const int32_t* comp, double beta, const double* vm, int32_t lmats,
                     const double* tau, int32_t ltau, const double* wr, int32_t lreal, double eps, double* chi_iv,
                     double* chi_tau, double* chi_w, void* stream) {
  return ed_chi_add_poles_signed(nfrac, npole, E, z, peso, Ei, comp, nullptr, beta, vm, lmats, tau, ltau, wr, lreal,
                                 eps, chi_iv, chi_tau, chi_w, stream);
}

}  // extern "C"
