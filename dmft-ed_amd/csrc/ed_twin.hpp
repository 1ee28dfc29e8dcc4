// Twin-sector vectors (ed_sector_twin_vector): the vector of a twin entry of
// the state list, rebuilt from its partner's vector that already lies in HBM.
//
// The reference keeps a twin entry without a vector and returns
//   vector(i) = partner%cvec(Order(i))                 (ED_EIGENSPACE.f90:414-445)
// with Order the flipped partner states put in ascending order
// (twin_sector_order / flip_state, ED_SETUP.f90:1123-1186): row i of the twin
// sector holds state s, and its value is the partner's value at the row of
// flip_state(s).  No sign, no conjugation.
//
//   k_twin_gather     every mode: one thread per twin row, the partner row
//                     from the partner's index tables (coalesced store,
//                     gathered load).
//   k_twin_transpose  normal mode: rows are ordered idw-outer / iup-inner
//                     (DESIGN.md §1), so exchanging the spin halves turns
//                     row idw*DimUp + iup of the partner into row
//                     iup*DimDw + idw of the twin: the transpose of the
//                     partner's DimDw x DimUp view.  LDS-tiled, loads and
//                     stores both coalesced along the fast index.
#pragma once
#include "ed_kernels.hpp"

namespace edg {

// flip_state (ED_SETUP.f90:1162-1186): normal / superc exchange the two
// Ns-bit halves; nonsu2 complements all 2*Ns bits (`full`: those bits).
__device__ __forceinline__ uint32_t twin_flip(uint32_t s, int mode, int ns, uint32_t half, uint32_t full) {
  if (mode == ED_MODE_NONSU2) return ~s & full;
  return ((s & half) << ns) | (s >> ns);
}

// One thread per row of dst, grid-strided.  idx_src is the partner's index;
// the host has checked that dst is the twin of src, so every flipped state
// lies in src (DevIndex does not check bounds).
template <bool VC>
__global__ void __launch_bounds__(kBlock) k_twin_gather(const uint32_t* __restrict__ map_dst, int64_t dim,
                                                        DevIndex idx_src, int mode, uint32_t full,
                                                        const val_t<VC>* __restrict__ x,
                                                        val_t<VC>* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < dim; i += (int64_t)gridDim.x * kBlock)
    y[i] = x[idx_src(twin_flip(map_dst[i], mode, idx_src.ns, idx_src.mask, full))];
}

// y (C x R, row-major) = transpose of x (R x C, row-major); R = DimDw and
// C = DimUp of the partner.  256 threads move one 32 x 32 tile: 32 lanes
// along the fast index of the load and of the store (256 or 512 contiguous
// bytes per tile row), 8 tile rows per pass.  A tile row is padded by one
// element, so the column read has a stride of 33 elements: 66 (real) or 132
// (complex) dwords, i.e. 2 or 4 banks from lane to lane, which spreads the 32
// lanes of an 8-byte read and the 16 lanes of a 16-byte read over all 64
// banks.  Partial tiles at both edges are guarded on load and on store.
constexpr int kTwinTile = 32;
constexpr int kTwinRows = kBlock / kTwinTile;

template <bool VC>
__global__ void __launch_bounds__(kBlock) k_twin_transpose(int64_t R, int64_t C, const val_t<VC>* __restrict__ x,
                                                           val_t<VC>* __restrict__ y) {
  __shared__ val_t<VC> tile[kTwinTile][kTwinTile + 1];
  const int tx = threadIdx.x % kTwinTile, ty = threadIdx.x / kTwinTile;
  const int64_t tr = (R + kTwinTile - 1) / kTwinTile, tc = (C + kTwinTile - 1) / kTwinTile;
  for (int64_t t = blockIdx.x; t < tr * tc; t += gridDim.x) {
    const int64_t r0 = (t / tc) * kTwinTile, c0 = (t % tc) * kTwinTile;
#pragma unroll
    for (int j = 0; j < kTwinTile; j += kTwinRows) {
      const int64_t r = r0 + ty + j, c = c0 + tx;
      if (r < R && c < C) tile[ty + j][tx] = x[r * C + c];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kTwinTile; j += kTwinRows) {
      const int64_t c = c0 + ty + j, r = r0 + tx;
      if (c < C && r < R) y[c * R + r] = tile[tx][ty + j];
    }
    __syncthreads();  // the next tile overwrites the LDS image
  }
}

}  // namespace edg
