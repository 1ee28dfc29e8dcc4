// ed_multi.hpp — stored H applied to a block of NV vectors at once, and the
// kernels of the Lanczos recurrence that advances NV start vectors in
// lockstep (driver: ed_lanczos.hip, ed_sector_lanc_tridiag_lockstep).
//
//   k_spmv_mv       Y = H X, X and Y row-interleaved      spMatVec_cc STORED_HxV.f90:132-143
//   k_lanc_init_mv  seeds -> interleaved R, P = 0, b_1     .repo/PLAIN_LANCZOS.f90:96-101
//   k_lanc_b_mv     part B of one step for NV vectors      .repo/PLAIN_LANCZOS.f90:111-113
//   k_lanc_fin_mv   the NV scalars of a pass from its block partials
//
// Layout: element (row i, vector v) of a block is at i*NV + v.  The gather of
// column c is then one contiguous run of NV values, read with 16-byte loads
// wherever NV values fill 16 bytes; every matrix word is loaded once per row
// and serves all NV columns.  Per vector the kernel forms exactly the products
// and additions of k_spmv, in its order (diagonal first, then the slots), with
// the same helpers: column v of Y is bit-identical to the one-pass kernel's Hv.
#pragma once
#include "ed_kernels.hpp"

namespace edg {

// Slots of a row fetched together.  The gathered values in flight are
// CH * NV * (complex ? 2 : 1) doubles; the chunk shrinks with the block so
// that they stay at 32 doubles (64 VGPRs), the budget k_spmv_pk's complex
// form already lives with (kChunk = 16 double2).  No instantiation uses
// scratch (-Rpass-analysis=kernel-resource-usage; table in DESIGN.md §15).
template <bool VC, int NV>
struct MvChunk {
  static constexpr int d = NV * (VC ? 2 : 1);
  static constexpr int value = 32 / d > kChunk ? kChunk : 32 / d;
};
static_assert(MvChunk<false, 8>::value == 4 && MvChunk<true, 8>::value == 2 && MvChunk<false, 1>::value == 16, "");

// NV consecutive values of a row-interleaved block, 16 bytes per load where
// NV * sizeof(V) >= 16 (blocks are 16-byte aligned: checked at the entry)
template <bool VC, int NV>
__device__ __forceinline__ void ld_blk(const val_t<VC>* __restrict__ p, val_t<VC> (&o)[NV]) {
  if constexpr (VC || NV == 1) {
#pragma unroll
    for (int v = 0; v < NV; v++) o[v] = p[v];
  } else {
    const double2* q = (const double2*)p;
#pragma unroll
    for (int v = 0; v < NV / 2; v++) {
      const double2 t = q[v];
      o[2 * v] = t.x;
      o[2 * v + 1] = t.y;
    }
  }
}
template <bool VC, int NV>
__device__ __forceinline__ void st_blk(val_t<VC>* __restrict__ p, const val_t<VC> (&a)[NV]) {
  if constexpr (VC || NV == 1) {
#pragma unroll
    for (int v = 0; v < NV; v++) p[v] = a[v];
  } else {
    double2* q = (double2*)p;
#pragma unroll
    for (int v = 0; v < NV / 2; v++) q[v] = make_double2(a[2 * v], a[2 * v + 1]);
  }
}

// --------------------------------------------------------------- epilogues
// row(i, acc, xi, part) receives the NV values (H X)_i and X_i and adds the
// row's contribution to the NV fused reductions; finish(part) runs once per
// thread after the loop.  all_done(): nothing to do for any vector (uniform
// over the grid, so the whole launch returns together).
template <bool VC, int NV>
struct EpiStoreMV {
  using V = val_t<VC>;
  V* hv;
  __device__ __forceinline__ bool all_done() const { return false; }
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ void row(int64_t i, const V (&acc)[NV], const V (&)[NV], double (&)[NV]) {
    st_blk<VC, NV>(hv + i * NV, acc);
  }
  __device__ __forceinline__ void finish(const double (&)[NV]) {}
};

// Lanczos step, part A, for NV runs (EpiLancA per vector): v = R*invb,
// w = (H R)*invb - b*P, P <- v, W <- w, partial of Re<v|w>.  A run that has
// broken down takes invb = b = 0 by a select: its LancState, alpha and beta
// stay as they are, its columns of P and W become zeros (no extra read, no
// divergent branch), and its partial sums are dropped by k_lanc_fin_mv.
template <bool VC, int NV>
struct EpiLancAMV {
  using V = val_t<VC>;
  const LancState* st;  // [NV]
  V* P;
  V* W;
  double* partials;     // [NV][gridDim.x]
  double invb[NV], b[NV];
  __device__ __forceinline__ bool all_done() const {
    int d = 1;
#pragma unroll
    for (int v = 0; v < NV; v++) d &= st[v].done != 0;
    return d != 0;
  }
  __device__ __forceinline__ void prepare() {
#pragma unroll
    for (int v = 0; v < NV; v++) {
      const bool dn = st[v].done != 0;
      invb[v] = dn ? 0.0 : st[v].invb;
      b[v] = dn ? 0.0 : st[v].beta;
    }
  }
  __device__ __forceinline__ void row(int64_t i, const V (&acc)[NV], const V (&xi)[NV], double (&part)[NV]) {
    V p[NV], vv[NV], ww[NV];
    ld_blk<VC, NV>(P + i * NV, p);
#pragma unroll
    for (int v = 0; v < NV; v++) {
      vv[v] = scl(invb[v], xi[v]);
      const V h = scl(invb[v], acc[v]);
      ww[v] = sub(h, scl(b[v], p[v]));
      part[v] += redot(vv[v], ww[v]);
    }
    st_blk<VC, NV>(P + i * NV, vv);
    st_blk<VC, NV>(W + i * NV, ww);
  }
  __device__ __forceinline__ void finish(const double (&part)[NV]) {
#pragma unroll
    for (int v = 0; v < NV; v++) {
      const double s = block_sum(part[v]);
      if (threadIdx.x == 0) partials[(size_t)v * gridDim.x + blockIdx.x] = s;
    }
  }
};

// ------------------------------------------------------------ block H·X
// k_spmv / k_spmv_pk for NV vectors: one thread per row, wave-uniform slice
// pointer and width, LDS dictionary (PK), XCD row remap, and every load of a
// chunk issued before its first use.  PK: cw = {col:24 | dictionary index:8}
// words and hv the 256-entry dictionary; otherwise cw = the SELL columns and
// hv the SELL values.  Slots past the slice width reload the last slot and
// are dropped by a select (k_spmv_pk's branch-free chunk).
template <bool HC, bool VC, int NT, int NV, bool PK, class Epi>
__global__ void __launch_bounds__(kBlock) k_spmv_mv(const val_t<HC>* __restrict__ diag,
                                                    const int64_t* __restrict__ sptr,
                                                    const uint32_t* __restrict__ cw,
                                                    const val_t<HC>* __restrict__ hv,
                                                    const val_t<VC>* __restrict__ x, int64_t dim,
                                                    int64_t nslice, Epi epi, int xcd) {
  using V = val_t<VC>;
  using H = val_t<HC>;
  constexpr int CH = MvChunk<VC, NV>::value;
  if (epi.all_done()) return;
  epi.prepare();
  double part[NV];
#pragma unroll
  for (int v = 0; v < NV; v++) part[v] = 0.0;
  __shared__ H sdict[PK ? 256 : 1];
  if constexpr (PK) {
    sdict[threadIdx.x] = hv[threadIdx.x];  // kBlock == 256 == dictionary capacity
    __syncthreads();
  }
  auto body = [&](int64_t i) {
    const int64_t s = (int64_t)__builtin_amdgcn_readfirstlane((int)(i >> 6));  // one slice per wavefront
    const int64_t s0 = sptr[s];
    const int w = (int)((sptr[s + 1] - s0) >> 6);
    const uint32_t* wp = cw + s0 + (i & 63);
    const H* vp = hv + s0 + (i & 63);  // (plain SELL only)
    V xi[NV], acc[NV];
    ld_blk<VC, NV>(x + i * NV, xi);
    const H dg = ldh<NT>(diag + i);
    if (w == 0) {
#pragma unroll
      for (int v = 0; v < NV; v++) acc[v] = add(vzero<V>(), mul(dg, xi[v]));
    } else {
      const int wm = w - 1;
      for (int k0 = 0; k0 < w; k0 += CH) {
        uint32_t c[CH];
        H h[CH];
        V g[CH][NV];
#pragma unroll
        for (int k = 0; k < CH; k++) c[k] = ldm<NT>(wp + 64 * min(k0 + k, wm));
        if constexpr (!PK) {
#pragma unroll
          for (int k = 0; k < CH; k++) h[k] = ldh<NT>(vp + 64 * min(k0 + k, wm));
        }
#pragma unroll
        for (int k = 0; k < CH; k++) {
          const int64_t col = PK ? (int64_t)(c[k] & kPackColMask) : (int64_t)c[k];
          ld_blk<VC, NV>(x + col * NV, g[k]);
          if constexpr (PK) h[k] = sdict[c[k] >> kPackShift];
        }
        asm volatile("" ::: "memory");  // every gather in flight before the first use
        if (k0 == 0) {
#pragma unroll
          for (int v = 0; v < NV; v++) acc[v] = add(vzero<V>(), mul(dg, xi[v]));
        }
#pragma unroll
        for (int k = 0; k < CH; k++) {
#pragma unroll
          for (int v = 0; v < NV; v++) acc[v] = sel(k0 + k < w, add(acc[v], mul(h[k], g[k][v])), acc[v]);
        }
      }
    }
    epi.row(i, acc, xi, part);
  };
  // xcd: each XCD sweeps one contiguous range of rows (k_spmv_pk)
  int64_t b = blockIdx.x;
  if (xcd) b = (b & 7) * (gridDim.x >> 3) + (b >> 3);
  for (int64_t i = b * kBlock + threadIdx.x; i < nslice * 64; i += (int64_t)gridDim.x * kBlock)
    if (i < dim) body(i);
  epi.finish(part);
}

// ------------------------------------------------- lockstep Lanczos passes
// Passes over the interleaved block with one thread per element: element e
// belongs to vector e % NV, and the grid stride is a multiple of NV (kBlock
// is), so a thread stays with one vector and lane l of a wave with vector
// l % NV.  Block partial of vector v -> partials[v * gridDim.x + blockIdx.x].
template <int NV>
__device__ __forceinline__ void mv_block_partials(double part, double* __restrict__ partials) {
  static_assert(kBlock % NV == 0 && 64 % NV == 0, "a lane keeps its vector");
  __shared__ double ws[kBlock / 64][NV];
#pragma unroll
  for (int o = 32; o >= NV; o >>= 1) part += __shfl_xor(part, o, 64);
  const int lane = threadIdx.x & 63;
  if (lane < NV) ws[threadIdx.x >> 6][lane] = part;
  __syncthreads();
  if (threadIdx.x < NV) {
    double t = 0.0;
#pragma unroll
    for (int wv = 0; wv < kBlock / 64; wv++) t = t + ws[wv][threadIdx.x];
    partials[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
  }
}

// Start: seeds[v*dim + i] (the nseed x dim layout of the batch entry, v the
// vector's place in its group) -> R[i*NV + v]; P <- 0; partials of ||seed_v||^2.
// One thread per row: each of the NV reads is coalesced over the wave's rows,
// the interleaved row is stored whole.
template <bool VC, int NV>
__global__ void __launch_bounds__(kBlock) k_lanc_init_mv(const val_t<VC>* __restrict__ seeds,
                                                         val_t<VC>* __restrict__ R,
                                                         val_t<VC>* __restrict__ P, int64_t dim,
                                                         double* __restrict__ partials) {
  using V = val_t<VC>;
  double part[NV];
  V zero[NV];
#pragma unroll
  for (int v = 0; v < NV; v++) {
    part[v] = 0.0;
    zero[v] = vzero<V>();
  }
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < dim; i += (int64_t)gridDim.x * kBlock) {
    V r[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) {
      r[v] = seeds[(int64_t)v * dim + i];
      part[v] += redot(r[v], r[v]);
    }
    st_blk<VC, NV>(R + i * NV, r);
    st_blk<VC, NV>(P + i * NV, zero);
  }
#pragma unroll
  for (int v = 0; v < NV; v++) {
    const double s = block_sum(part[v]);
    if (threadIdx.x == 0) partials[(size_t)v * gridDim.x + blockIdx.x] = s;
  }
}

// Part B for NV runs: w = W - alpha_v * P, R <- w, partials of ||w||^2.  A
// run that is done takes alpha = 0 by a select (its columns are zeros).
template <bool VC, int NV>
__global__ void __launch_bounds__(kBlock) k_lanc_b_mv(const val_t<VC>* __restrict__ W,
                                                      const val_t<VC>* __restrict__ P,
                                                      val_t<VC>* __restrict__ R, int64_t n,
                                                      const LancState* __restrict__ st,
                                                      double* __restrict__ partials) {
  using V = val_t<VC>;
  int d = 1;
#pragma unroll
  for (int v = 0; v < NV; v++) d &= st[v].done != 0;
  if (d) return;  // every run of the group is done: uniform over the grid
  const int v = threadIdx.x % NV;
  const double a = st[v].done ? 0.0 : st[v].alpha;
  double part = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += (int64_t)gridDim.x * kBlock) {
    const V w = sub(W[e], scl(a, P[e]));
    R[e] = w;
    part += redot(w, w);
  }
  mv_block_partials<NV>(part, partials);
}

// The scalars of one pass: block v (of NV, kBlock threads) sums vector v's
// nblk partials in fixed order (sum_partials, as k_lanc_fin_a / k_lanc_fin_b).
//   MODE 0: start    b_1 = sqrt(tot), done = (b == 0)          (k_lanc_init)
//   MODE 1: part A   alpha                                      (k_lanc_fin_a)
//   MODE 2: part B   lanc_set_beta                              (k_lanc_fin_b)
// Run v keeps alpha at ab + v*ldab and beta at ab + v*ldab + boff.
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_lanc_fin_mv(const double* __restrict__ partials, int nblk,
                                                        LancState* st, double* ab, int64_t ldab, int64_t boff,
                                                        double thresh) {
  LancState* s = st + blockIdx.x;
  if (MODE != 0 && s->done) return;  // the whole block belongs to one run
  const double tot = sum_partials(partials + (size_t)blockIdx.x * nblk, nblk);
  if (threadIdx.x != 0) return;
  double* alpha = ab + (int64_t)blockIdx.x * ldab;
  if (MODE == 0) {
    const double b = sqrt(tot);
    s->beta = b;
    s->invb = 1.0 / b;
    s->alpha = 0.0;
    s->thresh = thresh;
    s->tmp = 0.0;
    s->iter = 0;
    s->done = (b == 0.0) ? 1 : 0;
  } else if (MODE == 1) {
    s->alpha = tot;
    alpha[s->iter] = tot;
  } else {
    lanc_set_beta(tot, s, alpha + boff);
  }
}

}  // namespace edg
