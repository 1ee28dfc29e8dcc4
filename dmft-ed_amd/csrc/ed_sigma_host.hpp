// ed_sigma_host.hpp — the host half of the self-energy kernel of ed_sigma.hpp
// (k_sigma / ed_sigma_build): plain C++, compiles with g++ alone, as
// ed_chi_host.hpp and ed_seed_pair.hpp do.
//
// build_sigma_normal (ED_GF_NORMAL.f90:656-731), build_sigma_superc
// (ED_GF_SUPERC.f90:826-929) and build_sigma_nonsu2 (from ED_GF_NONSU2.f90:977)
// take the impurity G, the non-interacting inverse invG0 = z + mu - impHloc -
// Delta(z) of the bath (invg0_bath_mats_main, ED_BATH_FUNCTIONS.f90:1784-1901;
// invf0_bath_mats_main, ED_BATH_FUNCTIONS.f90:1980-2029; delta_bath_mats_main,
// ED_BATH_FUNCTIONS.f90:221-399) and leave Sigma = invG0 - G^-1.  Here that
// is done block by block: a block is an ordered list of
// n <= 6 impurity indices, its bath a pole table
//   Delta_ij(z) = sum_p c_p W_ip conj(W_jp) / (z - e_p),
// c_p = 1 for every bath whose H is Hermitian.
//
//   SigmaBlock      one block: indices, one-body matrix, pole table.
//   sigma_blocks    the block list and pole tables of an ed_params.
//   sigma_compile   validates a block list and the grids of one call.
//   sigma_grid      the frequency of one work item (the grids of gf.matsubara
//                   and gf.realaxis, bit for bit).
//   sigma_point<N>  the work at one (block, grid point), shared by the kernel
//                   and the host restatement.
//   sigma_host      the kernel's arithmetic, serially.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/ed_gpu.h"
#include "ed_hosteig.hpp"

#if defined(__HIPCC__)
#define ED_SIG_HD __host__ __device__ inline __attribute__((always_inline))
#define ED_SIG_UNROLL _Pragma("unroll")
#else
#define ED_SIG_HD inline
#define ED_SIG_UNROLL
#endif

namespace edg {

constexpr int kSigMaxN = ED_SIGMA_MAX_N;          // indices of one block
constexpr int kSigMaxPoles = ED_SIGMA_MAX_POLES;  // poles of one block
constexpr int kSigMaxBlocks = ED_MAX_NSPIN * ED_MAX_NORB;

struct SigC {
  double x, y;
};

// comp[i][j]: the flat component of entry (i, j) in the (Nspin, Nspin, Norb,
// Norb) layout of build_gf; a Nambu block (nambu = 1, n = 2: particle and hole
// of one orbital) reads and writes comp[0][0] only.
struct SigmaBlock {
  int32_t n, np, nambu, pad;
  int32_t comp[kSigMaxN][kSigMaxN];
  SigC h[kSigMaxN][kSigMaxN];  // impHloc - mu on the block (Nambu: diag(h - mu, -(h - mu)))
  double e[kSigMaxPoles];
  SigC c[kSigMaxPoles];
  SigC w[kSigMaxPoles][kSigMaxN];
};

// ------------------------------------------------------------ complex helpers
ED_SIG_HD SigC sig_c(double x, double y) {
  SigC r;
  r.x = x;
  r.y = y;
  return r;
}
ED_SIG_HD SigC sig_add(SigC a, SigC b) { return sig_c(a.x + b.x, a.y + b.y); }
ED_SIG_HD SigC sig_sub(SigC a, SigC b) { return sig_c(a.x - b.x, a.y - b.y); }
ED_SIG_HD SigC sig_mul(SigC a, SigC b) { return sig_c(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
ED_SIG_HD SigC sig_mulc(SigC a, SigC b) { return sig_c(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }  // a conj(b)
// p / (a + i b): Smith's division, the arithmetic of cdiv (ed_kernels.hpp),
// which a g++ build cannot include
ED_SIG_HD SigC sig_cdiv(SigC p, double a, double b) {
  if (fabs(b) <= fabs(a)) {
    const double r = b / a, den = a + b * r;
    return sig_c((p.x + p.y * r) / den, (p.y - p.x * r) / den);
  }
  const double r = a / b, den = a * r + b;
  return sig_c((p.x * r + p.y) / den, (p.y * r - p.x) / den);
}

// In-place inverse by Gauss-Jordan with partial pivoting on |re| + |im|.  Every
// matrix index is an unrolled counter; the pivot row (and, at the end, the
// column permutation it leaves) moves by selects, so the matrix stays in
// registers on the device.
template <int N>
ED_SIG_HD void sig_invert(SigC (&a)[N][N]) {
  if (N == 1) {
    a[0][0] = sig_cdiv(sig_c(1.0, 0.0), a[0][0].x, a[0][0].y);
    return;
  }
  int piv[N];
  ED_SIG_UNROLL
  for (int k = 0; k < N; k++) {
    int p = k;
    double best = fabs(a[k][k].x) + fabs(a[k][k].y);
    ED_SIG_UNROLL
    for (int r = k + 1; r < N; r++) {
      const double m = fabs(a[r][k].x) + fabs(a[r][k].y);
      if (m > best) {
        best = m;
        p = r;
      }
    }
    piv[k] = p;
    ED_SIG_UNROLL
    for (int r = k + 1; r < N; r++) {
      const bool hit = p == r;
      ED_SIG_UNROLL
      for (int j = 0; j < N; j++) {
        const SigC t = a[r][j], u = a[k][j];
        a[r][j] = hit ? u : t;
        a[k][j] = hit ? t : u;
      }
    }
    const SigC d = sig_cdiv(sig_c(1.0, 0.0), a[k][k].x, a[k][k].y);
    a[k][k] = sig_c(1.0, 0.0);
    ED_SIG_UNROLL
    for (int j = 0; j < N; j++) a[k][j] = sig_mul(a[k][j], d);
    ED_SIG_UNROLL
    for (int r = 0; r < N; r++) {
      if (r == k) continue;
      const SigC f = a[r][k];
      a[r][k] = sig_c(0.0, 0.0);
      ED_SIG_UNROLL
      for (int j = 0; j < N; j++) a[r][j] = sig_sub(a[r][j], sig_mul(f, a[k][j]));
    }
  }
  ED_SIG_UNROLL
  for (int k = N - 1; k >= 0; k--) {
    ED_SIG_UNROLL
    for (int c = k + 1; c < N; c++) {
      const bool hit = piv[k] == c;
      ED_SIG_UNROLL
      for (int i = 0; i < N; i++) {
        const SigC t = a[i][c], u = a[i][k];
        a[i][c] = hit ? u : t;
        a[i][k] = hit ? t : u;
      }
    }
  }
}

// Work item t of lmats + lreal: t < lmats is i w_n = (0, pi/beta (2t + 1)),
// the rest w + i eps on linspace(wini, wfin, lreal).  *mirror is the index of
// -w on a symmetric real grid and t itself on the Matsubara axis.
ED_SIG_HD void sigma_grid(int t, double beta, int lmats, double wini, double wfin, int lreal, double eps, double* zr,
                          double* zi, int* i, int* mirror) {
  if (t < lmats) {
    *zr = 0.0;
    *zi = (M_PI / beta) * (2.0 * (double)(t + 1) - 1.0);
    *i = *mirror = t;
    return;
  }
  const int k = t - lmats;
  const double step = lreal > 1 ? (wfin - wini) / (double)(lreal - 1) : 0.0;
  *zr = (k == lreal - 1 && lreal > 1) ? wfin : (double)k * step + wini;
  *zi = eps;
  *i = k;
  *mirror = lreal - 1 - k;
}

// The work at one (block, grid point).  One N x N matrix is live per phase:
//   1. Delta from the poles -> io.delta;  invG0 = z - h - Delta -> io.stash
//   2. G0 = invG0^-1 in place -> io.g0
//   3. (with_g) G from io.g, inverted in place
//   4. Sigma = io.unstash - G^-1 -> io.sigma
// IO: SigC g(i, j); void delta / g0 / sigma / stash (i, j, SigC); SigC unstash(i, j),
// called with unrolled (i, j) only.
template <int N, class IO>
ED_SIG_HD void sigma_point(const SigmaBlock& B, double zr, double zi, bool with_g, IO& io) {
  SigC m[N][N];
  ED_SIG_UNROLL
  for (int i = 0; i < N; i++) {
    ED_SIG_UNROLL
    for (int j = 0; j < N; j++) m[i][j] = sig_c(0.0, 0.0);
  }
  for (int p = 0; p < B.np; p++) {
    const SigC c = sig_cdiv(B.c[p], zr - B.e[p], zi);
    ED_SIG_UNROLL
    for (int i = 0; i < N; i++) {
      ED_SIG_UNROLL
      for (int j = 0; j < N; j++) m[i][j] = sig_add(m[i][j], sig_mul(sig_mulc(B.w[p][i], B.w[p][j]), c));
    }
  }
  ED_SIG_UNROLL
  for (int i = 0; i < N; i++) {
    ED_SIG_UNROLL
    for (int j = 0; j < N; j++) {
      io.delta(i, j, m[i][j]);
      const SigC zh = i == j ? sig_c(zr - B.h[i][j].x, zi - B.h[i][j].y) : sig_c(-B.h[i][j].x, -B.h[i][j].y);
      m[i][j] = sig_sub(zh, m[i][j]);
      if (with_g) io.stash(i, j, m[i][j]);
    }
  }
  sig_invert<N>(m);
  ED_SIG_UNROLL
  for (int i = 0; i < N; i++) {
    ED_SIG_UNROLL
    for (int j = 0; j < N; j++) io.g0(i, j, m[i][j]);
  }
  if (!with_g) return;
  ED_SIG_UNROLL
  for (int i = 0; i < N; i++) {
    ED_SIG_UNROLL
    for (int j = 0; j < N; j++) m[i][j] = io.g(i, j);
  }
  sig_invert<N>(m);
  ED_SIG_UNROLL
  for (int i = 0; i < N; i++) {
    ED_SIG_UNROLL
    for (int j = 0; j < N; j++) io.sigma(i, j, sig_sub(io.unstash(i, j), m[i][j]));
  }
}

// The arrays of one call: G (and F) in, Sigma, G0, Delta (and Sigma_A, F0)
// out; index 0 the Matsubara axis, 1 the real axis.  Complex, (ncomp, L).
struct SigmaArrays {
  const SigC* g[2];
  const SigC* f[2];
  SigC* s[2];
  SigC* g0[2];
  SigC* d[2];
  SigC* sa[2];
  SigC* f0[2];
};

// The IO of sigma_point on those arrays at grid index i of axis ax (L points).
// A block of n >= 3 stashes invG0 in Sigma's own slots, which the same work
// item reads back; n <= 2 (every Nambu block, whose Sigma keeps only its first
// row) holds it in registers.
template <int N>
struct SigmaIO {
  const SigmaBlock& B;
  const SigmaArrays& A;
  int ax, i, mirror;
  int64_t L;
  SigC st[N <= 2 ? N : 1][N <= 2 ? N : 1];
  ED_SIG_HD SigmaIO(const SigmaBlock& b, const SigmaArrays& a, int ax_, int i_, int mirror_, int64_t L_)
      : B(b), A(a), ax(ax_), i(i_), mirror(mirror_), L(L_) {}
  ED_SIG_HD int64_t at(int r, int c) const { return (int64_t)B.comp[B.nambu ? 0 : r][B.nambu ? 0 : c] * L + i; }
  ED_SIG_HD SigC g(int r, int c) const {
    if (!B.nambu) return A.g[ax][at(r, c)];
    if (r != c) return A.f[ax][at(0, 0)];
    if (r == 0) return A.g[ax][at(0, 0)];
    const SigC v = A.g[ax][(int64_t)B.comp[0][0] * L + mirror];
    return sig_c(-v.x, v.y);  // -conj(G) at the mirrored frequency
  }
  ED_SIG_HD void delta(int r, int c, SigC v) const {
    if (!B.nambu || (r == 0 && c == 0)) A.d[ax][at(r, c)] = v;
  }
  ED_SIG_HD void g0(int r, int c, SigC v) const {
    if (!B.nambu || (r == 0 && c == 0)) A.g0[ax][at(r, c)] = v;
    else if (r == 0) A.f0[ax][at(0, 0)] = v;
  }
  ED_SIG_HD void sigma(int r, int c, SigC v) const {
    if (!B.nambu || (r == 0 && c == 0)) A.s[ax][at(r, c)] = v;
    else if (r == 0) A.sa[ax][at(0, 0)] = v;
  }
  ED_SIG_HD void stash(int r, int c, SigC v) {
    if (N <= 2) st[N <= 2 ? r : 0][N <= 2 ? c : 0] = v;
    else A.s[ax][at(r, c)] = v;
  }
  ED_SIG_HD SigC unstash(int r, int c) const {
    if (N <= 2) return st[N <= 2 ? r : 0][N <= 2 ? c : 0];
    return A.s[ax][at(r, c)];
  }
};

template <int N>
ED_SIG_HD void sigma_item(const SigmaBlock& B, const SigmaArrays& A, int t, double beta, int lmats, double wini,
                          double wfin, int lreal, double eps, bool with_g) {
  double zr, zi;
  int i, mirror;
  sigma_grid(t, beta, lmats, wini, wfin, lreal, eps, &zr, &zi, &i, &mirror);
  const int ax = t < lmats ? 0 : 1;
  SigmaIO<N> io(B, A, ax, i, mirror, ax ? lreal : lmats);
  sigma_point<N>(B, zr, zi, with_g, io);
}

// ------------------------------------------------------------------ validation
inline bool sigma_n_valid(int n) { return n == 1 || n == 2 || n == 3 || n == 4 || n == 6; }

// Do [a, a + na) and [b, b + nb) share a byte?
inline bool sigma_overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || !na || !nb) return false;
  const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
  return p < q + nb && q < p + na;
}

// One call's blocks and grids.  ED_ERR_ARG unless every n is one of 1, 2, 3,
// 4, 6, every pole count lies in 1..64, no two blocks share an index, a Nambu
// block has n = 2 and its real grid is symmetric (wini == -wfin: the hole
// entry is read at the mirrored index), and no output shares a byte with an
// input or with another output.  why: the refusal in words.
inline int sigma_compile(int nblk, const ed_sigma_block* blk, int nspin, int norb, double beta, int lmats, double wini,
                         double wfin, int lreal, const SigmaArrays& A, std::vector<SigmaBlock>* out,
                         const char** why) {
  const char* dummy;
  if (!why) why = &dummy;
  *why = "";
  if (!blk || !out) return *why = "null", ED_ERR_ARG;
  if (nspin < 1 || nspin > ED_MAX_NSPIN || norb < 1 || norb > ED_MAX_NORB) return *why = "nspin / norb", ED_ERR_ARG;
  if (nblk < 1 || nblk > kSigMaxBlocks) return *why = "block count", ED_ERR_ARG;
  if (lmats < 0 || lreal < 0 || lmats + lreal == 0 || (lmats && !(beta > 0.0))) return *why = "grid", ED_ERR_ARG;
  const int nso = nspin * norb, ncomp = nso * nso;
  bool used[ED_MAX_NSPIN * ED_MAX_NORB] = {};
  bool nambu = false;
  out->assign(nblk, SigmaBlock{});
  for (int b = 0; b < nblk; b++) {
    const ed_sigma_block& s = blk[b];
    SigmaBlock& B = (*out)[b];
    if (!sigma_n_valid(s.n)) return *why = "block size outside {1, 2, 3, 4, 6}", ED_ERR_ARG;
    if (s.np < 1 || s.np > kSigMaxPoles) return *why = "pole count outside 1..64", ED_ERR_ARG;
    if (s.nambu != 0 && s.nambu != 1) return *why = "nambu flag", ED_ERR_ARG;
    if (s.nambu && (s.n != 2 || nspin != 1 || s.idx[0] != s.idx[1])) return *why = "Nambu block", ED_ERR_ARG;
    nambu = nambu || s.nambu;
    B.n = s.n;
    B.np = s.np;
    B.nambu = s.nambu;
    for (int i = 0; i < s.n; i++) {
      if (s.idx[i] < 0 || s.idx[i] >= nso) return *why = "index outside the impurity", ED_ERR_ARG;
      if (s.nambu && i) continue;  // particle and hole of one orbital
      if (used[s.idx[i]]) return *why = "overlapping blocks", ED_ERR_ARG;
      used[s.idx[i]] = true;
    }
    for (int i = 0; i < s.n; i++)
      for (int j = 0; j < s.n; j++) {
        const int si = s.idx[i] / norb, oi = s.idx[i] % norb, sj = s.idx[j] / norb, oj = s.idx[j] % norb;
        B.comp[i][j] = ((si * nspin + sj) * norb + oi) * norb + oj;
        B.h[i][j] = sig_c(s.h[i][j][0], s.h[i][j][1]);
      }
    for (int p = 0; p < s.np; p++) {
      B.e[p] = s.e[p];
      B.c[p] = sig_c(s.c[p][0], s.c[p][1]);
      for (int i = 0; i < s.n; i++) B.w[p][i] = sig_c(s.w[p][i][0], s.w[p][i][1]);
    }
  }
  if (nambu && lreal && wini != -wfin) return *why = "superc real axis: the grid must be symmetric (wini = -wfin)", ED_ERR_ARG;
  const bool with_g = A.g[0] || A.g[1];
  const void* in[4];
  const void* o[10];
  size_t nin[4], no[10];
  int ni = 0, nout = 0;
  for (int ax = 0; ax < 2; ax++) {
    const size_t L = ax ? lreal : lmats, nb = (size_t)ncomp * L * sizeof(SigC);
    if (!L) continue;
    if (!A.g0[ax] || !A.d[ax]) return *why = "null output", ED_ERR_ARG;
    if (with_g && (!A.g[ax] || !A.s[ax])) return *why = "null G or Sigma", ED_ERR_ARG;
    if (nambu && (!A.f0[ax] || (with_g && (!A.f[ax] || !A.sa[ax]))))
      return *why = "superc: null F, Sigma_A or F0", ED_ERR_ARG;
    const void* i2[2] = {A.g[ax], A.f[ax]};
    const void* o5[5] = {A.s[ax], A.g0[ax], A.d[ax], A.sa[ax], A.f0[ax]};
    for (int k = 0; k < 2; k++) in[ni] = i2[k], nin[ni++] = nb;
    for (int k = 0; k < 5; k++) o[nout] = o5[k], no[nout++] = nb;
  }
  for (int a = 0; a < nout; a++) {
    for (int k = 0; k < ni; k++)
      if (sigma_overlap(o[a], no[a], in[k], nin[k])) return *why = "an output aliases an input", ED_ERR_ARG;
    for (int k = 0; k < a; k++)
      if (sigma_overlap(o[a], no[a], o[k], no[k])) return *why = "two outputs alias", ED_ERR_ARG;
  }
  return ED_OK;
}

// -------------------------------------------------- block list of an ed_params
// The poles of one Hermitian replica block M = A + i B (n x n, row-major pairs)
// scaled by c: a real block through sym_eigh, a complex one through the real
// symmetric 2n x 2n embedding [[A, -B], [B, A]], whose eigenvectors (x; y) come
// in pairs spanning {u, i u} of every eigenvector u = x + i y of M: all 2n are
// taken with half the weight.
inline int sigma_replica_poles(int n, const double* mre, const double* mim, SigC c, ed_sigma_block* blk) {
  bool real = true;
  for (int i = 0; i < n * n; i++) real = real && mim[i] == 0.0;
  const int m = real ? n : 2 * n;
  if (blk->np + m > kSigMaxPoles) return ED_ERR_ARG;
  std::vector<double> a((size_t)m * m), w, z;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      // Hermitian part: the lower triangle as given
      const double re = i >= j ? mre[i * n + j] : mre[j * n + i];
      const double im = i >= j ? mim[i * n + j] : -mim[j * n + i];
      a[i + (size_t)m * j] = re;
      if (!real) {
        a[(i + n) + (size_t)m * (j + n)] = re;
        a[(i + n) + (size_t)m * j] = im;
        a[i + (size_t)m * (j + n)] = -im;
      }
    }
  sym_eigh(m, a, w, z);
  for (int p = 0; p < m; p++) {
    const int q = blk->np++;
    blk->e[q] = w[p];
    blk->c[q][0] = real ? c.x : 0.5 * c.x;
    blk->c[q][1] = real ? c.y : 0.5 * c.y;
    for (int i = 0; i < n; i++) {
      blk->w[q][i][0] = z[i + (size_t)m * p];
      blk->w[q][i][1] = real ? 0.0 : z[(i + n) + (size_t)m * p];
    }
  }
  return ED_OK;
}

// The blocks of (ed_mode, bath_type) with the pole
// table of the bath as this library's H couples it.  blk: [kSigMaxBlocks].
// ED_ERR_UNSUPPORTED for superc with a hybrid or replica bath.
inline int sigma_blocks(const ed_params& p, ed_sigma_block* blk, int* nblk, const char** why) {
  const char* dummy;
  if (!why) why = &dummy;
  *why = "";
  const int No = p.norb, Nsp = p.nspin, Nb = p.nbath;
  if (No < 1 || No > ED_MAX_NORB || Nsp < 1 || Nsp > ED_MAX_NSPIN || Nb < 1 || Nb > ED_MAX_NBATH)
    return *why = "norb / nspin / nbath", ED_ERR_ARG;
  if (p.ed_mode == ED_MODE_NONSU2 && Nsp != 2) return *why = "nonsu2 needs nspin = 2", ED_ERR_ARG;
  if (p.ed_mode == ED_MODE_SUPERC && Nsp != 1) return *why = "superc needs nspin = 1", ED_ERR_ARG;
  int nb = 0;
  auto fresh = [&](int n) -> ed_sigma_block& {
    ed_sigma_block& B = blk[nb++];
    B = ed_sigma_block{};
    B.n = n;
    return B;
  };
  auto hloc = [&](ed_sigma_block& B, int i, int j, int si, int sj, int oi, int oj) {
    B.h[i][j][0] = p.imphloc_re[si][sj][oi][oj] - (i == j ? p.xmu : 0.0);
    B.h[i][j][1] = p.imphloc_im[si][sj][oi][oj];
  };
  auto pole = [&](ed_sigma_block& B, double e) -> int {
    if (B.np >= kSigMaxPoles) return -1;
    B.e[B.np] = e;
    B.c[B.np][0] = 1.0;
    return B.np++;
  };
  if (p.ed_mode == ED_MODE_SUPERC) {
    if (p.bath_type != ED_BATH_NORMAL)
      return *why = "superc with a hybrid or replica bath: its orbital off-diagonal G and F are not built",
             ED_ERR_UNSUPPORTED;
    for (int o = 0; o < No; o++) {
      ed_sigma_block& B = fresh(2);
      B.nambu = 1;
      B.idx[0] = B.idx[1] = o;
      const double h = p.imphloc_re[0][0][o][o] - p.xmu;
      B.h[0][0][0] = h;
      B.h[1][1][0] = -h;
      for (int k = 0; k < Nb; k++) {
        // bath level k in Psi = (c_up, c+_dw): [[e, d], [d, -e]], coupled by V to
        // the particle and by -V to the hole; its Bogoliubov pair +-E
        const double e = p.bath_e[0][o][k], d = p.bath_d[0][o][k], v = p.bath_v[0][o][k];
        const double E = pythag(e, d);
        double u1 = 1.0, u2 = 0.0;  // eigenvector of +E
        if (E != 0.0) {
          const double a = e >= 0.0 ? e + E : d, b = e >= 0.0 ? d : E - e, nrm = pythag(a, b);
          if (nrm != 0.0) u1 = a / nrm, u2 = b / nrm;
        }
        const int q = pole(B, E), r = pole(B, -E);
        if (q < 0 || r < 0) return *why = "pole count outside 1..64", ED_ERR_ARG;
        B.w[q][0][0] = v * u1;
        B.w[q][1][0] = -v * u2;
        B.w[r][0][0] = v * -u2;
        B.w[r][1][0] = -v * u1;
      }
    }
  } else if (p.ed_mode == ED_MODE_NORMAL && p.bath_type == ED_BATH_NORMAL) {
    for (int s = 0; s < Nsp; s++)
      for (int o = 0; o < No; o++) {
        ed_sigma_block& B = fresh(1);
        B.idx[0] = s * No + o;
        hloc(B, 0, 0, s, s, o, o);
        for (int k = 0; k < Nb; k++) {
          const int q = pole(B, p.bath_e[s][o][k]);
          if (q < 0) return *why = "pole count outside 1..64", ED_ERR_ARG;
          B.w[q][0][0] = p.bath_v[s][o][k];
        }
      }
  } else if (p.ed_mode == ED_MODE_NONSU2 && p.bath_type == ED_BATH_NORMAL) {
    for (int o = 0; o < No; o++) {
      ed_sigma_block& B = fresh(2);
      for (int s = 0; s < 2; s++) {
        B.idx[s] = s * No + o;
        for (int t = 0; t < 2; t++) hloc(B, s, t, s, t, o, o);
      }
      for (int k = 0; k < Nb; k++)
        for (int sb = 0; sb < 2; sb++) {  // bath spin: v to its own impurity spin, u to the other
          const int q = pole(B, p.bath_e[sb][o][k]);
          if (q < 0) return *why = "pole count outside 1..64", ED_ERR_ARG;
          for (int s = 0; s < 2; s++) B.w[q][s][0] = s == sb ? p.bath_v[s][o][k] : p.bath_u[s][o][k];
        }
    }
  } else {
    // hybrid and replica baths: one block per spin (normal) or one in all (nonsu2)
    const bool ns2 = p.ed_mode == ED_MODE_NONSU2;
    const int n = ns2 ? 2 * No : No;
    for (int sblk = 0; sblk < (ns2 ? 1 : Nsp); sblk++) {
      ed_sigma_block& B = fresh(n);
      for (int i = 0; i < n; i++) {
        const int si = ns2 ? i / No : sblk, oi = i % No;
        B.idx[i] = si * No + oi;
        for (int j = 0; j < n; j++) hloc(B, i, j, si, ns2 ? j / No : sblk, oi, j % No);
      }
      for (int k = 0; k < Nb; k++) {
        if (p.bath_type == ED_BATH_HYBRID) {
          for (int sb = ns2 ? 0 : sblk; sb < (ns2 ? 2 : sblk + 1); sb++) {
            const int q = pole(B, p.bath_e[sb][0][k]);
            if (q < 0) return *why = "pole count outside 1..64", ED_ERR_ARG;
            for (int i = 0; i < n; i++) {
              const int si = ns2 ? i / No : sblk, oi = i % No;
              B.w[q][i][0] = si == sb ? p.bath_v[si][oi][k] : p.bath_u[si][oi][k];
            }
          }
        } else {
          // H couples every impurity level to its replica by conj(vr) in both
          // directions (ed_model.hpp): Delta = conj(vr)^2 (z - h_k)^-1
          double mre[kSigMaxN * kSigMaxN], mim[kSigMaxN * kSigMaxN];
          for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) {
              const int si = ns2 ? i / No : sblk, sj = ns2 ? j / No : sblk;
              mre[i * n + j] = p.bath_h_re[si][sj][i % No][j % No][k];
              mim[i * n + j] = p.bath_h_im[si][sj][i % No][j % No][k];
            }
          const double vr = p.bath_vr_re[k], vi = -p.bath_vr_im[k];
          if (sigma_replica_poles(n, mre, mim, sig_c(vr * vr - vi * vi, 2.0 * vr * vi), &B) != ED_OK)
            return *why = "pole count outside 1..64", ED_ERR_ARG;
        }
      }
    }
  }
  *nblk = nb;
  return ED_OK;
}

// ------------------------------------------------------------ host restatement
template <int N>
inline void sigma_host_n(const SigmaBlock& B, const SigmaArrays& A, double beta, int lmats, double wini, double wfin,
                         int lreal, double eps, bool with_g) {
  for (int t = 0; t < lmats + lreal; t++) sigma_item<N>(B, A, t, beta, lmats, wini, wfin, lreal, eps, with_g);
}

// The kernel's arithmetic, block by block and point by point.  The outputs
// must be zero on entry (ed_sigma_build clears them).
inline void sigma_host(const std::vector<SigmaBlock>& blocks, const SigmaArrays& A, double beta, int lmats,
                       double wini, double wfin, int lreal, double eps) {
  const bool with_g = A.g[0] || A.g[1];
  for (const SigmaBlock& B : blocks) {
    switch (B.n) {
      case 1: sigma_host_n<1>(B, A, beta, lmats, wini, wfin, lreal, eps, with_g); break;
      case 2: sigma_host_n<2>(B, A, beta, lmats, wini, wfin, lreal, eps, with_g); break;
      case 3: sigma_host_n<3>(B, A, beta, lmats, wini, wfin, lreal, eps, with_g); break;
      case 4: sigma_host_n<4>(B, A, beta, lmats, wini, wfin, lreal, eps, with_g); break;
      case 6: sigma_host_n<6>(B, A, beta, lmats, wini, wfin, lreal, eps, with_g); break;
      default: break;
    }
  }
}

}  // namespace edg
