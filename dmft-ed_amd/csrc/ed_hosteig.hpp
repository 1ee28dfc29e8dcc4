// ed_hosteig.hpp — the host half of the Lanczos solvers, each piece once:
// the start-vector hash, the implicit-QL tridiagonal eigen-solver (EISPACK
// tql2) with its rotation sinks, the dense eigenproblem of a restart (tred2 +
// QL, cyclic Jacobi behind it), the thick-restart cycle's decisions and the
// degeneracy screen's set-up and decision.
//
// No HIP header: plain g++ -std=c++17 compiles it (tests/test_hosteig_cpu.py);
// only the hash is also device code, under hipcc.  The operation order of the
// floating-point expressions is pinned: the GF poles and the plain-Lanczos
// Ritz values are bit-identical to the oracle's (-ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/ed_gpu.h"

#ifdef __HIPCC__
#define ED_HOST_DEVICE __host__ __device__
#else
#define ED_HOST_DEVICE
#endif

namespace edg {

// ------------------------------------------------------- start-vector hash
// splitmix64 of x -> uniform double in [-1, 1).  Default start vector:
// element i = splitmix_unit(i + 1) (documented in DESIGN.md; tests reproduce
// it).  The batch and lockstep solves fill it on the host and rely on the
// value being bit-identical to the kernels'.
ED_HOST_DEVICE inline double splitmix_unit(uint64_t x) {
  uint64_t z = x * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (double)(z >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
}
// element i of the hash vector of `seed` (k_hash_vec, the screens' start)
ED_HOST_DEVICE inline double hash_vec_unit(int64_t i, uint64_t seed) {
  return splitmix_unit((uint64_t)(i + 1 + seed * 0x632BE59BD9B4E019ull));
}

// ------------------------------------------------------------ implicit QL
// Host tridiagonal eigen-solver (tql2, EISPACK; the same algorithm the
// reference uses for Ritz values, .repo/PLAIN_LANCZOS.f90:427-565).
inline double pythag(double a, double b) {
  double p = std::max(fabs(a), fabs(b));
  if (p != 0.0) {
    double r = std::min(fabs(a), fabs(b)) / p;
    r = r * r;
    for (;;) {
      double t = 4.0 + r;
      if (t == 4.0) break;
      double s = r / t, u = 1.0 + 2.0 * s;
      p = u * p;
      double su = s / u;
      r = (su * su) * r;
    }
  }
  return p;
}

// Rotation sinks of ql_implicit: what the plane rotations (columns i, i + 1
// of Z) and the final ordering's column swaps are applied to.
struct QlNoZ {  // eigenvalues only
  void rotate(int, double, double) {}
  void swap(int, int) {}
};
struct QlFullZ {  // z: n x n, column-major
  double* z;
  int n;
  void rotate(int i, double c, double s) {
    double* const zi = z + (size_t)n * i;
    double* const zj = z + (size_t)n * (i + 1);
    for (int k = 0; k < n; k++) {
      const double h = zj[k];
      zj[k] = s * zi[k] + c * h;
      zi[k] = c * zi[k] - s * h;
    }
  }
  void swap(int i, int k) {
    for (int j = 0; j < n; j++) std::swap(z[j + (size_t)n * i], z[j + (size_t)n * k]);
  }
};
struct QlRowZ {  // z[n]: the first row of Z only, O(n^2) instead of O(n^3)
  double* z;
  void rotate(int i, double c, double s) {
    const double h = z[i + 1];
    z[i + 1] = s * z[i] + c * h;
    z[i] = c * z[i] - s * h;
  }
  void swap(int i, int k) { std::swap(z[i], z[k]); }
};

// d[n] diagonal, e[i] = T(i, i+1) with e[n-1] = 0 (both overwritten); on
// return d ascending and the sink's Z rotated and ordered with it.  Returns 0,
// or l + 1 when eigenvalue l took more than 30 iterations.
// FAST: hypot in place of EISPACK's iterative pythag (the restart
// eigenproblem of the thick-restart solver; Ritz values of the plain
// Lanczos and the GF poles keep the reference's pythag)
template <bool FAST, class Sink>
inline int ql_implicit(int n, double* d, double* e, Sink zs) {
  double f = 0.0, tst1 = 0.0;
  for (int l = 0; l < n; l++) {
    tst1 = std::max(tst1, fabs(d[l]) + fabs(e[l]));
    int m = l;
    while (m < n && tst1 + fabs(e[m]) != tst1) m++;
    if (m >= n) m = n - 1;  // e[n-1] == 0 stops the scan at n-1 (NaN input: stay in bounds)
    if (m != l) {
      for (int it = 0;; it++) {
        if (it >= 30) return l + 1;
        const int l1 = l + 1, l2 = l1 + 1;
        double g = d[l];
        double p = (d[l1] - g) / (2.0 * e[l]);
        double r = FAST ? hypot(p, 1.0) : pythag(p, 1.0);
        const double sr = p >= 0.0 ? fabs(r) : -fabs(r);
        d[l] = e[l] / (p + sr);
        d[l1] = e[l] * (p + sr);
        const double dl1 = d[l1];
        double h = g - d[l];
        for (int i = l2; i < n; i++) d[i] -= h;
        f += h;
        p = d[m];
        double c = 1.0, c2 = c, c3 = c, s = 0.0, s2 = 0.0;
        const double el1 = e[l1];
        for (int i = m - 1; i >= l; i--) {
          c3 = c2;
          c2 = c;
          s2 = s;
          g = c * e[i];
          h = c * p;
          r = FAST ? hypot(p, e[i]) : pythag(p, e[i]);
          e[i + 1] = s * r;
          s = e[i] / r;
          c = p / r;
          p = c * d[i] - s * g;
          d[i + 1] = h + s * (c * g + s * d[i]);
          zs.rotate(i, c, s);
        }
        p = -s * s2 * c3 * el1 * e[l] / dl1;
        e[l] = s * p;
        d[l] = c * p;
        if (!(tst1 + fabs(e[l]) > tst1)) break;
      }
    }
    d[l] += f;
  }
  // ascending order (selection sort)
  for (int i = 0; i + 1 < n; i++) {
    int k = i;
    for (int j = i + 1; j < n; j++)
      if (d[j] < d[k]) k = j;
    if (k != i) {
      std::swap(d[i], d[k]);
      zs.swap(i, k);
    }
  }
  return 0;
}

// EISPACK's convention: d[n] diag, e[n] with e[0] ignored (e[i] couples i-1, i);
// z column-major n x n (the matrix to rotate: the identity, tred2's Q) or null.
template <bool FAST = false>
inline int tql2(int n, double* d, double* e, double* z) {
  if (n == 1) return 0;
  for (int i = 1; i < n; i++) e[i - 1] = e[i];
  e[n - 1] = 0.0;
  return z ? ql_implicit<FAST>(n, d, e, QlFullZ{z, n}) : ql_implicit<FAST>(n, d, e, QlNoZ{});
}

// Poles of one GF continued fraction (ed_tridiag_poles): eigenvalues E of
// tridiag(alfa[0:n], beta[1:n]), the first components z1 of the eigenvectors
// (may be null) and their squares z2.  Returns 0, or nonzero when the QL
// iteration did not converge.
inline int tridiag_poles(int n, const double* alfa, const double* beta, double* E, double* z2, double* z1) {
  std::vector<double> e(n, 0.0), z(n, 0.0);
  for (int i = 0; i < n; i++) E[i] = alfa[i];
  for (int i = 0; i + 1 < n; i++) e[i] = beta[i + 1];  // e[i] = T(i, i+1); e[n-1] = 0
  z[0] = 1.0;  // Z starts as the identity: its first row as e_1
  const int rc = ql_implicit<false>(n, E, e.data(), QlRowZ{z.data()});
  if (rc != 0) return rc;
  for (int i = 0; i < n; i++) z2[i] = z[i] * z[i];
  if (z1)
    for (int i = 0; i < n; i++) z1[i] = z[i];
  return 0;
}

inline double lowest_ritz(const std::vector<double>& a, const std::vector<double>& b, int n) {
  std::vector<double> d(a.begin(), a.begin() + n), e(n, 0.0);
  for (int q = 1; q < n; q++) e[q] = b[q];
  tql2(n, d.data(), e.data(), nullptr);
  return d[0];
}

// ------------------------------------------ thick-restart Lanczos (ARPACK)
// Cyclic Jacobi for a small real symmetric matrix (host): A (n x n, column-
// major) -> ascending eigenvalues w, eigenvectors Z (column-major).
inline void jacobi_eigh(int n, std::vector<double> A, std::vector<double>& w, std::vector<double>& Z) {
  Z.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; i++) Z[i + (size_t)n * i] = 1.0;
  auto a = [&](int i, int j) -> double& { return A[i + (size_t)n * j]; };
  for (int sweep = 0; sweep < 100; sweep++) {
    double off = 0.0, tot = 0.0;
    for (int j = 0; j < n; j++)
      for (int i = 0; i < n; i++) {
        tot += a(i, j) * a(i, j);
        if (i != j) off += a(i, j) * a(i, j);
      }
    if (off <= 1e-30 * tot || off == 0.0) break;
    for (int p = 0; p < n - 1; p++)
      for (int q = p + 1; q < n; q++) {
        const double apq = a(p, q);
        if (apq == 0.0) continue;
        const double theta = (a(q, q) - a(p, p)) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < n; k++) {  // A <- A J
          const double akp = a(k, p), akq = a(k, q);
          a(k, p) = c * akp - sn * akq;
          a(k, q) = sn * akp + c * akq;
        }
        for (int k = 0; k < n; k++) {  // A <- J^T A
          const double apk = a(p, k), aqk = a(q, k);
          a(p, k) = c * apk - sn * aqk;
          a(q, k) = sn * apk + c * aqk;
        }
        for (int k = 0; k < n; k++) {
          const double zkp = Z[k + (size_t)n * p], zkq = Z[k + (size_t)n * q];
          Z[k + (size_t)n * p] = c * zkp - sn * zkq;
          Z[k + (size_t)n * q] = sn * zkp + c * zkq;
        }
      }
  }
  std::vector<int> idx(n);
  for (int i = 0; i < n; i++) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](int x, int y) { return a(x, x) < a(y, y); });
  std::vector<double> Zs((size_t)n * n);
  w.assign(n, 0.0);
  for (int k = 0; k < n; k++) {
    w[k] = a(idx[k], idx[k]);
    for (int i = 0; i < n; i++) Zs[i + (size_t)n * k] = Z[i + (size_t)n * idx[k]];
  }
  Z.swap(Zs);
}

// Householder reduction of a real symmetric matrix to tridiagonal form with
// the transformation accumulated (EISPACK tred2 / Numerical Recipes §11.2):
// A (n x n, column-major, A(i,j) = A[i + n*j]) is overwritten by Q with
// Q^T A Q = tridiag(d, e), e[i] coupling i-1 and i (e[0] = 0).  With tql2
// (same z convention) the projected matrix of a restart costs O(n^3) with a
// small constant: the cyclic Jacobi took ~0.5 ms per 23 x 23 restart on the
// host, most of a small sector's solve.
inline void tred2(int n, double* A, double* d, double* e) {
#define TA(i, j) A[(i) + (size_t)n * (j)]
  for (int i = n - 1; i > 0; i--) {
    const int l = i - 1;
    double h = 0.0, scale = 0.0;
    if (l > 0) {
      for (int k = 0; k <= l; k++) scale += fabs(TA(i, k));
      if (scale == 0.0) {
        e[i] = TA(i, l);
      } else {
        for (int k = 0; k <= l; k++) {
          TA(i, k) /= scale;
          h += TA(i, k) * TA(i, k);
        }
        double f = TA(i, l);
        double g = f >= 0.0 ? -sqrt(h) : sqrt(h);
        e[i] = scale * g;
        h -= f * g;
        TA(i, l) = f - g;
        f = 0.0;
        for (int j = 0; j <= l; j++) {
          TA(j, i) = TA(i, j) / h;
          g = 0.0;
          for (int k = 0; k <= j; k++) g += TA(j, k) * TA(i, k);
          for (int k = j + 1; k <= l; k++) g += TA(k, j) * TA(i, k);
          e[j] = g / h;
          f += e[j] * TA(i, j);
        }
        const double hh = f / (h + h);
        for (int j = 0; j <= l; j++) {
          f = TA(i, j);
          e[j] = g = e[j] - hh * f;
          for (int k = 0; k <= j; k++) TA(j, k) -= (f * e[k] + g * TA(i, k));
        }
      }
    } else {
      e[i] = TA(i, l);
    }
    d[i] = h;
  }
  d[0] = 0.0;
  e[0] = 0.0;
  for (int i = 0; i < n; i++) {
    const int l = i - 1;
    if (d[i] != 0.0) {
      for (int j = 0; j <= l; j++) {
        double g = 0.0;
        for (int k = 0; k <= l; k++) g += TA(i, k) * TA(k, j);
        for (int k = 0; k <= l; k++) TA(k, j) -= g * TA(k, i);
      }
    }
    d[i] = TA(i, i);
    TA(i, i) = 1.0;
    for (int j = 0; j <= l; j++) TA(j, i) = TA(i, j) = 0.0;
  }
#undef TA
}

// Symmetric eigenproblem of the projected matrix: ascending w, eigenvectors
// as the columns of Z (column-major).  tred2 + tql2; the cyclic Jacobi only if
// the QL iteration does not converge.
inline void sym_eigh(int n, const std::vector<double>& A, std::vector<double>& w, std::vector<double>& Z) {
  Z = A;
  w.assign(n, 0.0);
  std::vector<double> e(n, 0.0);
  tred2(n, Z.data(), w.data(), e.data());
  if (tql2<true>(n, w.data(), e.data(), Z.data()) != 0) jacobi_eigh(n, A, w, Z);
}

// --------------------------------------------- one restart cycle's decisions
// A solve on the basis columns [k0, m) has the ma x ma (ma = m - k0) projected
// matrix Tm (column-major); alpha/beta are indexed by basis column.  Used by
// trlan_core (any k0) and by the batch and lockstep solves (k0 = 0).
constexpr double kBreakdownRel = 1e-13;  // beta_j under this x the local scale of T: invariant subspace
constexpr double kRitzEps23 = 3.6e-11;   // ARPACK's floor eps^(2/3) of the relative convergence test
constexpr int kTrlanMaxCols = 64;        // columns of the coefficient buffers (ncv + probe columns)

// ARPACK-style test of a Ritz pair: resid <= tol * max(eps^(2/3), |theta|)
inline bool ritz_converged(double resid, double theta, double tol) {
  return resid <= tol * std::max(kRitzEps23, fabs(theta));
}
// Tm <- the sweep's columns [j0, m) of alpha/beta.  Returns the first column
// whose beta broke down (Tm filled up to and including it), else -1.
inline int trl_fill(double* Tm, int ma, int k0, int j0, int m, const double* al, const double* be) {
  auto tm = [&](int i, int j) -> double& { return Tm[i + (size_t)ma * j]; };
  for (int j = j0; j < m; j++) {
    const int l = j - k0;
    tm(l, l) = al[j];
    if (l + 1 < ma) tm(l, l + 1) = tm(l + 1, l) = be[j];
    const double scale = fabs(al[j]) + (l > 0 ? fabs(tm(l - 1, l)) : 0.0) + 1e-300;
    if (l + 1 < ma && be[j] < kBreakdownRel * scale) return j;
  }
  return -1;
}
// how many of the lowest nev Ritz pairs have converged: residual |beta_m * Z(ma-1, i)|
inline int trl_nconv(int ma, int nev, double beta, const double* theta, const double* Z, double tol) {
  int conv = 0;
  for (int i = 0; i < nev; i++)
    if (ritz_converged(fabs(beta * Z[(ma - 1) + (size_t)ma * i]), theta[i], tol)) conv++;
  return conv;
}
// thick restart: keep nkeep Ritz vectors + the residual direction
// (kept beyond nev: (ma - nev) / 2 — within 5 % of the best of 16
// restart-length variants on configs[3])
inline int trl_nkeep(int ma, int nev) { return std::max(nev, std::min(ma - 2, nev + (ma - nev) / 2)); }
// the restarted Tm: diag(theta[0, nkeep)) + the residual's couplings in row and column nkeep
inline void trl_arrowhead(double* Tm, int ma, int nkeep, double beta, const double* theta, const double* Z) {
  std::fill(Tm, Tm + (size_t)ma * ma, 0.0);
  for (int i = 0; i < nkeep; i++) {
    Tm[i + (size_t)ma * i] = theta[i];
    Tm[i + (size_t)ma * nkeep] = Tm[nkeep + (size_t)ma * i] = beta * Z[(ma - 1) + (size_t)ma * i];
  }
}

// ------------------- degeneracy screen (described above probe_screen, ed_eigh.hip)
constexpr int kScreenChunk = 10;  // steps between two decisions
constexpr int kScreenMaxSteps = 400;
// a copy missed within the margin below ev[nev-1] stays missed, so the
// margin sits under the 1e-10 Ritz-value bar (round 5: 1e-9, which let
// a pair 3e-10 below the top through; tests/golden/adversarial_probe.json)
constexpr double kProbeMargin = 1e-11;
// the screen's "none" needs only a loose tolerance on top of its
// residual-interval test (Ritz values approach the lowest from above)
constexpr double kProbeTol = 1e-5;  // 1e-3 misses copies; 1e-4 and 1e-5 find them
constexpr int kProbeNcv = 20;       // active columns of a deflated solve

inline double screen_cut(double evtop) { return evtop - kProbeMargin * std::max(1.0, fabs(evtop)); }

struct ScreenPlan {
  int mp;        // active columns of the deflated solves, behind the nev locked ones
  bool verify;   // run the degeneracy probe at all
  bool hint;     // the first screen's start vector carries the next Ritz vector
  double cut, tprobe;
  int maxsteps;
};
// After a main solve of m columns that converged conv of nev values, the
// highest of them evtop (before it, with conv = nev: may the probe run?).
inline ScreenPlan screen_setup(int m, int nev, int64_t dim, int opts, int conv, double evtop, double tol) {
  ScreenPlan p;
  p.mp = (int)std::min<int64_t>(std::min(std::min(m, kProbeNcv), kTrlanMaxCols - nev), dim - nev);
  // (dim > nev + 2 is a no-op for the batch and lockstep solves: their eligibility tests have it)
  p.verify = !(opts & ED_OPT_EIGH_NO_VERIFY) && dim > (int64_t)nev + 2 && p.mp >= 3 && conv == nev;
  p.hint = p.verify && nev + 1 < m && !(opts & ED_OPT_EIGH_NOHINT);
  p.cut = screen_cut(evtop);
  p.tprobe = std::max(tol, kProbeTol);
  p.maxsteps = (int)std::min<int64_t>(dim - nev, kScreenMaxSteps);
  return p;
}

enum ScreenVerdict : int { kScreenUndecided = -1, kScreenNone = 0, kScreenBelow = 1, kScreenQlFailed = 2 };
// The screen's recurrence so far, al[0, K) and be[0, K) (be[k] = |w_k|): the
// lowest Ritz value theta and the last component of its vector are the
// reversed tridiagonal's first components.  Below: theta < cut.  None: an
// invariant Krylov space (theta is an exact eigenvalue of the complement
// restricted to it; the hash start vector reaches every eigenvector), or theta
// converged to tol AND its whole residual interval above the cut.
inline ScreenVerdict screen_decide(const std::vector<double>& al, const std::vector<double>& be, double cut,
                                   double tol) {
  const int K = (int)al.size();
  std::vector<double> ar(K), br(K, 0.0), E(K), z2(K), z1(K);
  for (int i = 0; i < K; i++) ar[i] = al[K - 1 - i];
  for (int i = 1; i < K; i++) br[i] = be[K - 1 - i];
  if (tridiag_poles(K, ar.data(), br.data(), E.data(), z2.data(), z1.data()) != 0) return kScreenQlFailed;
  const double theta = E[0], resid = fabs(be[K - 1] * z1[0]);
  if (theta < cut) return kScreenBelow;
  const bool invariant = be[K - 1] < kBreakdownRel * (fabs(theta) + 1e-300);
  if (invariant || (ritz_converged(resid, theta, tol) && theta - resid > cut)) return kScreenNone;
  return kScreenUndecided;
}

}  // namespace edg
